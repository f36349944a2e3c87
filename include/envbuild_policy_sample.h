/*
 * envbuild_policy_sample.h — C-ABI of the stochastic policy head: tanh-Gaussian actions and their log-probabilities from the fp32
 * policy network in ONE launch (csrc/eb_policy_sample.hip), the same epilogue alone on given logits, and its reparameterised reverse
 * pass.  It is the stochastic branch of the reference's Policy4Toyota (utils/policy.py:71-96): a sample of
 * MultivariateNormalDiag(mean, exp(log_std)) under Affine(action_range) o Tanh, returned with its log_prob.
 *
 * A header of its own next to envbuild.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle of
 * envbuild.h has none of them), EB_ABI_VERSION is untouched, and a binding looks them up on demand.  Conventions (return codes,
 * eb_last_error, device pointers, `stream`) are those of envbuild.h.  Nothing here synchronises, allocates or uses atomics.
 *
 * The contract.  y [n, out_dim] is what eb_mlp_forward returns, that is, after the output activation; act_dim = out_dim / 2;
 * mean = y[:, :act_dim]; ls = y[:, act_dim:].  Every line below is one fp32 rounding (-ffp-contract=off, an explicit fmaf only where
 * written):
 *
 *   std = exp_det(ls)                       x = fmaf(std, eps, mean)
 *   action_range > 0:  t = tanh_det(x)      action = action_range * t
 *   action_range <= 0: action = x           (the reference's action_range=None)
 *   n_a  = ((-0.5f * eps) * eps - ls) - 0.9189385332f                  # log N(eps) - ls
 *   action_range > 0:  ax = |x|
 *        c_a = 2.0f * ((0.6931471806f - ax) - log_det(1.0f + exp_det(-2.0f * ax)))   # log(1 - tanh(x)^2), stable, even in x
 *        n_a = n_a - (log_ar + c_a)                                     # log_ar = (float)log((double)action_range), formed on the host
 *   logp = sum of n_a over a = 0 .. act_dim-1, ascending, from +0.0f
 *
 * Reverse pass.  eps is held fixed.  The cotangents are g_a [n, act_dim] and g_lp [n]; either may be NULL, which means zeros.
 *
 *   action_range > 0:  da = action_range * (1.0f - t * t);  s = g_a * da + g_lp * (2.0f * t)
 *   action_range <= 0: s = g_a
 *   g_y[:, a]           = s
 *   g_y[:, act_dim + a] = s * (std * eps) - g_lp
 *
 * g_y is the cotangent of y: what eb_mlp_backward(head = 0) takes as g_out (that entry applies the derivative of the output
 * activation itself).
 *
 * exp_det, tanh_det and sincos_det are the functions every other policy and env entry uses.  log_det is a Cephes logf: frexp to
 * [sqrt(1/2), sqrt(2)), the degree-8 polynomial, explicit fused multiply-adds, selects and no branches; it is defined for finite
 * positive normal x, and a NaN travels through it.
 *
 * Noise, used when eps == NULL.  key = splitmix64(seed + GOLDEN * counter), with splitmix64, u01 and GOLDEN = 0x9E3779B97F4A7C15
 * those of eb_traffic_respawn / eb_rollout_tape_sample.  For row id i (row_ids[e] as an unsigned 32-bit number; NULL means the row
 * index e) and pair p = a >> 1 with P = (act_dim + 1) / 2:
 *   idx = 2 * (p + P * i) in uint64;  u = 1.0f - u01(key, idx), exact and in (0, 1];  v = u01(key, idx + 1);
 *   r = sqrt(-2.0f * log_det(u)) with a correctly rounded square root;  sincos_det(6.2831855f * v, sn, cs);
 *   eps[2p] = r * cs;  eps[2p + 1] = r * sn, dropped when act_dim is odd.
 * |eps| <= 5.77 by construction.  A row's draw depends on its id and (seed, counter) only: not on n, its position or its neighbours.
 *
 * Rows are independent; n = 0 is a no-op; inf and NaN travel as IEEE arithmetic carries them and poison their own row only; repeated
 * calls repeat their bits.  eb_policy_sample equals eb_mlp_forward followed by eb_policy_sample_from_logits bit for bit, and its
 * logits_out equals eb_mlp_forward.  With eps = 0 the actions equal eb_policy_run_batch's as numbers (mean = -0.0 becomes +0.0:
 * fmaf(std, 0, -0.0) is +0.0).
 * The Python package restates this contract in NumPy: env_build_amd.policy_sample.policy_sample_reference / policy_noise_reference.
 */
#ifndef ENVBUILD_POLICY_SAMPLE_H
#define ENVBUILD_POLICY_SAMPLE_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_POLICY_SAMPLE_ABI_VERSION 1

int eb_policy_sample_abi_version(void);

/* ok = 1 when eb_policy_sample accepts this handle as it stands: precision EB_MLP_PRECISION_F32 (envbuild_mlp_f16.h), every layer set,
 * out_dim even and >= 2 (any hidden width eb_mlp_create takes: the four instantiations of the forward kernel, 64 to 512).  Else 0 with
 * the first unmet condition in eb_last_error; an fp16 handle is refused by name: eb_policy_sample_from_logits serves it.
 * EB_EINVAL: NULL handle or NULL ok. */
int eb_policy_sample_supported(eb_mlp m, int32_t* ok);

/* The fused launch: the network of eb_mlp_forward and the contract above, ALWAYS exactly one launch on `stream`.
 * obs [n, obs_dim]; eps [n, act_dim] or NULL to draw from (seed, counter, row id); row_ids [n] int32 or NULL; actions [n, act_dim];
 * logp [n], logits_out [n, out_dim] and eps_out [n, act_dim] may each be NULL (that output is not written).
 * EB_EINVAL (nothing written): NULL handle, an unsupported handle, n < 0, NULL obs or actions with n > 0, action_range NaN.
 * EB_ESTATE: a layer was never set. */
int eb_policy_sample(eb_mlp m, int32_t n, const float* obs, const float* eps, const int32_t* row_ids, uint64_t seed, uint64_t counter,
                     float action_range, float* actions, float* logp, float* logits_out, float* eps_out, void* stream);

/* The epilogue alone on logits [n, out_dim] (what eb_mlp_forward wrote, on a handle of either precision, or any other policy's
 * output): an elementwise kernel, one lane per row, no handle.  Runs on the current device.
 * EB_EINVAL: n < 0, out_dim odd, < 2 or > 32, NULL logits or actions with n > 0, action_range NaN. */
int eb_policy_sample_from_logits(int32_t n, int32_t out_dim, const float* logits, const float* eps, const int32_t* row_ids, uint64_t seed,
                                 uint64_t counter, float action_range, float* actions, float* logp, float* eps_out, void* stream);

/* The reverse pass above, elementwise: g_logits [n, out_dim] from logits [n, out_dim], the eps the forward used [n, act_dim] and the
 * cotangents g_actions [n, act_dim] / g_logp [n] (either may be NULL: zeros).  Runs on the current device.
 * EB_EINVAL: n < 0, out_dim odd, < 2 or > 32, NULL logits, eps or g_logits with n > 0, action_range NaN. */
int eb_policy_sample_vjp(int32_t n, int32_t out_dim, const float* logits, const float* eps, float action_range, const float* g_actions,
                         const float* g_logp, float* g_logits, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_POLICY_SAMPLE_H */
