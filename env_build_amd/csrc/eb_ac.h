// eb_ac.h — host-visible launch interface of the shared-trunk actor-critic kernels (eb_ac.hip), the only translation unit of
// libenvbuild_ac.so.  The contract is stated in include/envbuild_ac.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/envbuild_ac.h"

namespace eb {

// eb_ac_loss; every pointer is a DEVICE pointer.  The scalars are what eb_ppo.h's PpoHead and eb_value_loss hold, formed on the host
// the way those entries form them.
struct AcLossArgs {
    const float* y;            // [n, W]
    const float* actions;      // [n, act_dim]
    const float* logp_old;     // [n]
    const float* adv;          // [n]
    const float* adv_norm;     // [2] or NULL
    const float* ret;          // [n]
    const float* v_old;        // [n] or NULL
    float action_range, log_ar;
    float lo, hi;              // 1.0f - clip, 1.0f + clip
    float w;                   // -scale
    float g_ent;               // -(scale * ent_coef)
    float clip_v, v_scale;
    float* logp;               // [n]
    float* ratio;              // [n] or NULL
    float* surr;               // [n] or NULL
    float* ent;                // [n] or NULL
    float* vloss;              // [n] or NULL
    float* g_y;                // [n, W] or NULL
    float* z_out;              // [n, act_dim] or NULL
    int n, act_dim;
};
hipError_t launch_ac_loss(const AcLossArgs& A, hipStream_t s);          // one launch

// eb_ac_sample
struct AcSampleArgs {
    const float* y;            // [n, W]
    const float* eps;          // [n, act_dim] or NULL
    const int32_t* row_ids;    // [n] or NULL
    uint64_t seed, counter;
    float action_range, log_ar;
    float* actions;            // [n, act_dim] or NULL: split only
    float* logits_out;         // [n, 2 * act_dim] or NULL
    float* values;             // [n] or NULL
    float* logp;               // [n] or NULL
    float* eps_out;            // [n, act_dim] or NULL
    int n, act_dim;
};
hipError_t launch_ac_sample(const AcSampleArgs& A, hipStream_t s);      // one launch

}  // namespace eb
