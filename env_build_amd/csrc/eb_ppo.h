// eb_ppo.h — host-visible launch interface of the PPO update's kernels (eb_ppo.hip), next to eb_policy_logp.h's.  The arithmetic
// contract is stated in include/envbuild_ppo.h.
#pragma once
#include "eb_kernels.h"

namespace eb {

// what the surrogate row takes besides the logits; every pointer is a DEVICE pointer
struct PpoHead {
    const float* actions;      // [n, act_dim]
    const float* logp_old;     // [n]
    const float* adv;          // [n]
    const float* adv_norm;     // [2]: (mean, 1 / std), or NULL
    float action_range;        // <= 0: the action is x itself
    float log_ar;              // (float)log((double)action_range), formed on the host; unused with action_range <= 0
    float lo, hi;              // 1.0f - clip, 1.0f + clip
    float w;                   // -scale
    float g_ent;               // -(scale * ent_coef)
    float* logp;               // [n]
    float* ratio;              // [n] or NULL
    float* surr;               // [n] or NULL
    float* ent;                // [n] or NULL
    float* g_logits;           // [n, out_dim] or NULL
    float* z_out;              // [n, act_dim] or NULL
};

// the fused launch: fwd.out is logits_out ([n, out_dim] or NULL), fwd.head is ignored
struct PpoArgs {
    MlpArgs fwd;
    PpoHead head;
};
hipError_t launch_ppo_surrogate(const PpoArgs& A, hipStream_t s);

// the surrogate row alone, one lane per row
struct PpoLogitsArgs {
    const float* logits;       // [n, out_dim]
    int n, out_dim;
    PpoHead head;
};
hipError_t launch_ppo_surrogate_from_logits(const PpoLogitsArgs& A, hipStream_t s);

// generalised advantage estimation, one lane per env; arrays [T, n], t-major
struct GaeArgs {
    const float* rewards;
    const float* values;
    const float* v_last;       // [n]; not read when next_values is given
    const float* nonterminal;
    const float* next_values;  // or NULL
    const float* carry;        // or NULL: nonterminal
    float gamma, gl;           // gl = (float)((double)gamma * (double)lam)
    float* adv;
    float* ret;                // or NULL
    int T, n;
};
hipError_t launch_gae(const GaeArgs& A, hipStream_t s);

}  // namespace eb
