// eb_policy_logp.h — host-visible launch interface of the log-probability of given actions (eb_policy_logp.hip), next to
// eb_policy_sample.h's.  The arithmetic contract is stated in include/envbuild_policy_logp.h.
#pragma once
#include "eb_kernels.h"

namespace eb {

// what the epilogue takes besides the logits; every pointer is a DEVICE pointer
struct PolicyLogpHead {
    const float* actions;      // [n, act_dim]
    float action_range;        // <= 0: the action is x itself
    float log_ar;              // (float)log((double)action_range), formed on the host; unused with action_range <= 0
    float* logp;               // [n]
    float* z_out;              // [n, act_dim] or NULL
};

// the fused launch: fwd.out is logits_out ([n, out_dim] or NULL), fwd.head is ignored
struct PolicyLogpArgs {
    MlpArgs fwd;
    PolicyLogpHead head;
};
hipError_t launch_policy_logp(const PolicyLogpArgs& A, hipStream_t s);

// the epilogue alone, one lane per row
struct PolicyLogpLogitsArgs {
    const float* logits;       // [n, out_dim]
    int n, out_dim;
    PolicyLogpHead head;
};
hipError_t launch_policy_logp_from_logits(const PolicyLogpLogitsArgs& A, hipStream_t s);

// the reverse pass, one lane per (row, a)
struct PolicyLogpVjpArgs {
    const float* logits;       // [n, out_dim]
    const float* z;            // [n, act_dim]
    const float* g_logp;       // [n]
    float* g_logits;           // [n, out_dim]
    int n, out_dim;
};
hipError_t launch_policy_logp_vjp(const PolicyLogpVjpArgs& A, hipStream_t s);

}  // namespace eb
