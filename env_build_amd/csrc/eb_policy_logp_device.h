// eb_policy_logp_device.h — the log-probability of GIVEN actions under the tanh-Gaussian policy, written once: the inverse squash, one
// row's epilogue (called by the fused kernel and by the elementwise one of eb_policy_logp.hip) and one element of the reverse pass.  The
// arithmetic contract is the header comment of include/envbuild_policy_logp.h: every line there is one fp32 rounding here.  The
// logarithm is eb_policy_sample_device.h's, the exponential eb_mlp_device.h's: they are only called.  Everything is EB_DEV.
#pragma once
#include "eb_policy_sample_device.h"

#pragma clang fp contract(off)

namespace eb {
namespace plogp {

constexpr float U_MAX = 0x1.fffffep-1f;      // 1 - 2^-24: the largest float below 1

// ---- the inverse of tanh on [-U_MAX, U_MAX]: 1 +- u lies in [2^-24, 2), inside log_det's domain; a NaN travels ----
EB_DEV float artanh_log(float u) {
    return 0.5f * (psample::log_det(1.0f + u) - psample::log_det(1.0f - u));
}

// ---- one row forward.  y: the row's activated logits [2 * act_dim] (LDS or global); actions: the row's given actions [act_dim].
//      Writes *logp and z_out[act_dim] (if given), in ascending a. ----
EB_DEV void logp_row(const float* y, int act_dim, const float* actions, float action_range, float log_ar, float* logp, float* z_out) {
    float sum = 0.0f;
    for (int a = 0; a < act_dim; ++a) {
        const float mean = y[a], ls = y[act_dim + a];
        float x = actions[a];
        if (action_range > 0.0f) {
            float u = x / action_range;                                  // correctly rounded (the compiler's default for HIP)
            u = u > U_MAX ? U_MAX : (u < -U_MAX ? -U_MAX : u);           // a NaN falls through both compares
            x = artanh_log(u);
        }
        const float inv = mlp::exp_det(-ls);
        const float z = (x - mean) * inv;
        float n_a = ((-0.5f * z) * z - ls) - 0.9189385332f;
        if (action_range > 0.0f) {
            const float ax = __builtin_fabsf(x);
            const float c_a = 2.0f * ((0.6931471806f - ax) - psample::log_det(1.0f + mlp::exp_det(-2.0f * ax)));
            n_a = n_a - (log_ar + c_a);
        }
        sum = sum + n_a;
        if (z_out) z_out[a] = z;
    }
    *logp = sum;
}

// ---- one element of the reverse pass: the action is data, so the cotangents of mean[a] and ls[a] come from that of the row's logp ----
EB_DEV void logp_vjp_elem(float ls, float z, float g_lp, float& g_mean, float& g_ls) {
    const float inv = mlp::exp_det(-ls);
    g_mean = g_lp * (z * inv);
    g_ls = g_lp * (z * z - 1.0f);
}

}  // namespace plogp
}  // namespace eb
