// eb_policy_sample.h — host-visible launch interface of the stochastic policy head (eb_policy_sample.hip), next to eb_kernels.h's
// forward one.  The arithmetic contract is stated in include/envbuild_policy_sample.h.
#pragma once
#include "eb_kernels.h"

namespace eb {

// what the epilogue takes besides the logits; every pointer is a DEVICE pointer
struct PolicySampleHead {
    const float* eps;          // [n, act_dim], or NULL: drawn from (seed, counter, row id)
    const int32_t* row_ids;    // [n], or NULL: the row index
    uint64_t seed, counter;
    float action_range;        // <= 0: the action is x itself
    float log_ar;              // (float)log((double)action_range), formed on the host; unused with action_range <= 0
    float* actions;            // [n, act_dim]
    float* logp;               // [n] or NULL
    float* eps_out;            // [n, act_dim] or NULL
};

// the fused launch: fwd.out is logits_out ([n, out_dim] or NULL), fwd.head is ignored
struct PolicySampleArgs {
    MlpArgs fwd;
    PolicySampleHead head;
};
hipError_t launch_policy_sample(const PolicySampleArgs& A, hipStream_t s);

// the epilogue alone, one lane per row
struct PolicySampleLogitsArgs {
    const float* logits;       // [n, out_dim]
    int n, out_dim;
    PolicySampleHead head;
};
hipError_t launch_policy_sample_from_logits(const PolicySampleLogitsArgs& A, hipStream_t s);

// the reverse pass, one lane per (row, a)
struct PolicySampleVjpArgs {
    const float* logits;       // [n, out_dim]
    const float* eps;          // [n, act_dim]
    const float* g_actions;    // [n, act_dim] or NULL (zeros)
    const float* g_logp;       // [n] or NULL (zeros)
    float* g_logits;           // [n, out_dim]
    int n, out_dim;
    float action_range;
};
hipError_t launch_policy_sample_vjp(const PolicySampleVjpArgs& A, hipStream_t s);

}  // namespace eb
