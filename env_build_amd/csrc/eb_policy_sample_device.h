// eb_policy_sample_device.h — the stochastic head of the policy, written once: the deterministic logarithm, the counter-based Gaussian
// pair and one row's epilogue (tanh-Gaussian action, its log-probability, the noise it used), called by the fused kernel and by the
// elementwise one of eb_policy_sample.hip, and the row's reverse pass.  The arithmetic contract is the header comment of
// include/envbuild_policy_sample.h: every line there is one fp32 rounding here.  The exponential and the hyperbolic tangent are
// eb_mlp_device.h's, sin / cos eb_device.h's, the counter hash eb_env_device.h's: they are only called.  Everything is EB_DEV (forced
// inline): a translation unit's machine code depends on what it calls, not on what else this header holds.
#pragma once
#include "eb_env_device.h"
#include "eb_mlp_device.h"

#pragma clang fp contract(off)

namespace eb {
namespace psample {

// ---- deterministic natural logarithm (Cephes logf scheme, explicit fma, selects only) ----
// x = m * 2^e with m in [sqrt(1/2), sqrt(2)); log x = log1p(m - 1) + e * log 2, log 2 split as 0.693359375 - 2.12194440e-4.
// Defined for finite positive normal x; a NaN travels through it.
EB_DEV float log_det(float x0) {
    const unsigned bits = __builtin_bit_cast(unsigned, x0);
    const int e0 = (int)((bits >> 23) & 0xffu) - 126;
    const float m = __builtin_bit_cast(float, (bits & 0x807fffffu) | 0x3f000000u);   // frexp: [0.5, 1)
    const bool low = m < 0.707106781186547524f;
    const float fe = (float)(low ? e0 - 1 : e0);
    const float x = low ? (m + m) - 1.0f : m - 1.0f;
    const float z = x * x;
    float p = 7.0376836292e-2f;
    p = __builtin_fmaf(p, x, -1.1514610310e-1f);
    p = __builtin_fmaf(p, x, 1.1676998740e-1f);
    p = __builtin_fmaf(p, x, -1.2420140846e-1f);
    p = __builtin_fmaf(p, x, 1.4249322787e-1f);
    p = __builtin_fmaf(p, x, -1.6668057665e-1f);
    p = __builtin_fmaf(p, x, 2.0000714765e-1f);
    p = __builtin_fmaf(p, x, -2.4999993993e-1f);
    p = __builtin_fmaf(p, x, 3.3333331174e-1f);
    float y = (p * x) * z;
    y = __builtin_fmaf(-2.12194440e-4f, fe, y);
    y = __builtin_fmaf(-0.5f, z, y);
    const float r = __builtin_fmaf(0.693359375f, fe, x + y);
    return (x0 == x0) ? r : x0;
}

// ---- pair p of row id `id`: two unit normals from two uniforms of the counter (Box-Muller) ----
EB_DEV void normal_pair(uint64_t key, uint64_t id, int p, int P, float& e0, float& e1) {
    const uint64_t idx = 2ull * ((uint64_t)p + (uint64_t)P * id);
    const float u = 1.0f - u01(key, idx);                                // exact, in (0, 1]
    const float v = u01(key, idx + 1);
    const float r = __builtin_sqrtf(-2.0f * log_det(u));                 // correctly rounded (the compiler's default for HIP)
    float sn, cs;
    sincos_det(6.2831855f * v, sn, cs);
    e0 = r * cs;
    e1 = r * sn;
}

// ---- one row forward.  y: the row's activated logits [2 * act_dim] (LDS or global); eps: the row's noise or NULL to draw it with
//      (key, id).  Writes actions[act_dim], *logp (if given) and eps_out[act_dim] (if given), in ascending a. ----
EB_DEV void sample_row(const float* y, int act_dim, const float* eps, uint64_t key, uint64_t id, float action_range, float log_ar,
                       float* actions, float* logp, float* eps_out) {
    const int P = (act_dim + 1) >> 1;
    float sum = 0.0f, e_odd = 0.0f;
    for (int a = 0; a < act_dim; ++a) {
        float e;
        if (eps) {
            e = eps[a];
        } else if (a & 1) {
            e = e_odd;
        } else {
            normal_pair(key, id, a >> 1, P, e, e_odd);
        }
        const float mean = y[a], ls = y[act_dim + a];
        const float std = mlp::exp_det(ls);
        const float x = __builtin_fmaf(std, e, mean);
        float n_a = ((-0.5f * e) * e - ls) - 0.9189385332f;
        float action = x;
        if (action_range > 0.0f) {
            action = action_range * mlp::tanh_det(x);
            const float ax = __builtin_fabsf(x);
            const float c_a = 2.0f * ((0.6931471806f - ax) - log_det(1.0f + mlp::exp_det(-2.0f * ax)));
            n_a = n_a - (log_ar + c_a);
        }
        sum = sum + n_a;
        actions[a] = action;
        if (eps_out) eps_out[a] = e;
    }
    if (logp) *logp = sum;
}

// ---- one element of the reverse pass: the cotangents of mean[a] and ls[a] from those of action[a] and of the row's logp ----
EB_DEV void sample_vjp_elem(float mean, float ls, float e, float action_range, float g_a, float g_lp, float& g_mean, float& g_ls) {
    const float std = mlp::exp_det(ls);
    float s = g_a;
    if (action_range > 0.0f) {
        const float t = mlp::tanh_det(__builtin_fmaf(std, e, mean));
        const float da = action_range * (1.0f - t * t);
        s = g_a * da + g_lp * (2.0f * t);
    }
    g_mean = s;
    g_ls = s * (std * e) - g_lp;
}

}  // namespace psample
}  // namespace eb
