/*
 * envbuild_policy_logp.h — C-ABI of the log-probability of GIVEN actions under the tanh-Gaussian policy: the fp32 policy network and
 * the epilogue in ONE launch (csrc/eb_policy_logp.hip), the same epilogue alone on given logits, and its reverse pass.  It is what a
 * trainer does with the distribution the reference's Policy4Toyota._logits2dist returns (utils/policy.py:71-82): log_prob(actions) of
 * actions it stored earlier — old samples under new weights — for likelihood ratios (PPO, off-policy corrections) and for
 * maximum-likelihood fitting of the policy to given actions.  envbuild_policy_sample.h returns the log-probability of its own draw only,
 * and its reverse pass is the reparameterised one (the noise fixed, the action moving).  Here the action is data: the derivatives go to
 * mean and log_std only.
 *
 * A header of its own next to envbuild_policy_sample.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY,
 * EB_ABI_VERSION and every other family's version are untouched, and a binding looks them up on demand.  Conventions (return codes,
 * eb_last_error, device pointers) are those of envbuild.h.  Nothing here synchronises, allocates or uses atomics.
 *
 * The three working entries take ONE struct.  Their stream is therefore a field, not a parameter, and the table of stream-taking
 * prototypes (tests/test_stream_census.py) does not count them: this family's own tests hold each of them to that table's obligations
 * (a side stream, capture, replay).  Every scalar and every pointer of the struct is read AT CALL TIME: under stream capture those
 * values are baked into the graph, and the device buffers they point to are read at every replay (envbuild.h's capture bullet).
 *
 * The contract.  y [n, out_dim] is what eb_mlp_forward returns, that is, after the output activation; act_dim = out_dim / 2;
 * mean = y[:, :act_dim]; ls = y[:, act_dim:]; a is the given action.  Every line below is one fp32 rounding (-ffp-contract=off, an
 * explicit fmaf only where written):
 *
 *   action_range > 0:  u = a / action_range                              # IEEE division, correctly rounded
 *                      u = u > U ? U : (u < -U ? -U : u)                  # U = 0x1.fffffep-1f = 1 - 2^-24; selects, so a NaN travels
 *                      x = 0.5f * (log_det(1.0f + u) - log_det(1.0f - u)) # atanh(u); 1 +- u lies in [2^-24, 2), inside log_det's domain
 *   action_range <= 0: x = a                                              # the reference's action_range=None
 *   inv = exp_det(-ls)            z = (x - mean) * inv
 *   n_a = ((-0.5f * z) * z - ls) - 0.9189385332f                          # log N(z) - ls
 *   action_range > 0:  ax = |x|
 *        c_a = 2.0f * ((0.6931471806f - ax) - log_det(1.0f + exp_det(-2.0f * ax)))   # envbuild_policy_sample.h's expression
 *        n_a = n_a - (log_ar + c_a)                                       # log_ar = (float)log((double)action_range), formed on the host
 *   logp = sum of n_a over a = 0 .. act_dim-1, ascending, from +0.0f      z_out[:, a] = z
 *
 * The clamp makes an action at or beyond +-action_range finite: it is taken as +-U * action_range, |x| = atanh(U) ~ 8.664.  The
 * sampler produces exactly +-action_range once tanh_det saturates, so such actions are ordinary input here.  c_a is the sampler's
 * expression, so given x the two Jacobian terms agree.
 *
 * Reverse pass.  The action is data; the one cotangent is g_lp [n], and it is required.
 *
 *   g_y[:, a]           = g_lp * (z * inv)
 *   g_y[:, act_dim + a] = g_lp * (z * z - 1.0f)
 *
 * g_y is the cotangent of y: what eb_mlp_backward(head = 0) takes as g_out.  The reverse pass reads z and the logits only: not the
 * actions, and it does not depend on action_range.
 *
 * What is NOT promised: logp of the sampler's own action does not reproduce the sampler's logp bit for bit.  The action was rounded
 * after tanh, atanh amplifies that rounding by 1 / (1 - u^2) and the standardisation by 1 / std: with log_std down to -4 the two differ
 * by up to 1.6e-4 on rows with |x| < 3.  A trainer that wants a ratio of exactly 1 on its first pass takes logp_old from this entry,
 * not from the sampler: calls repeat their bits.
 *
 * exp_det and log_det are the functions envbuild_policy_sample.h names.  Rows are independent; n = 0 is a no-op that needs no pointer;
 * a refusal writes nothing; inf and NaN travel as IEEE arithmetic carries them and poison their own row only; repeated calls repeat
 * their bits.  eb_policy_logp equals eb_mlp_forward followed by eb_policy_logp_from_logits bit for bit, and its logits_out equals
 * eb_mlp_forward.
 * The Python package restates this contract in NumPy: env_build_amd.policy_logp.policy_logp_reference.
 */
#ifndef ENVBUILD_POLICY_LOGP_H
#define ENVBUILD_POLICY_LOGP_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_POLICY_LOGP_ABI_VERSION 1

/* Which entry reads which field is on the right; a field an entry does not read may hold anything. */
typedef struct eb_policy_logp_args {
    int32_t n, out_dim;        /* out_dim: read by from_logits / vjp only (the fused entry takes the handle's) */
    const float* obs;          /* [n, obs_dim]          fused entry */
    const float* logits;       /* [n, out_dim]          from_logits, vjp */
    const float* actions;      /* [n, act_dim]          fused, from_logits */
    float action_range;        /* > 0: squashed; <= 0: the reference's action_range=None; NaN refused */
    float* logp;               /* [n]                   fused, from_logits */
    float* logits_out;         /* [n, out_dim] or NULL  fused */
    float* z_out;              /* [n, act_dim] or NULL  fused, from_logits: the standardised pre-squash value */
    const float* z;            /* [n, act_dim]          vjp */
    const float* g_logp;       /* [n]                   vjp */
    float* g_logits;           /* [n, out_dim]          vjp */
    void* stream;
} eb_policy_logp_args;

int eb_policy_logp_abi_version(void);

/* ok = 1 when eb_policy_logp accepts this handle as it stands: the conditions of eb_policy_sample_supported (precision
 * EB_MLP_PRECISION_F32, every layer set, out_dim even and >= 2).  Else 0 with the first unmet condition in eb_last_error; an fp16
 * handle is refused by name: eb_policy_logp_from_logits serves it.  EB_EINVAL: NULL handle or NULL ok. */
int eb_policy_logp_supported(eb_mlp m, int32_t* ok);

/* The fused launch: the network of eb_mlp_forward and the contract above, ALWAYS exactly one launch on a->stream.
 * Reads n, obs, actions, action_range, logp, logits_out, z_out, stream.
 * EB_EINVAL (nothing written): NULL handle or args, an unsupported handle, n < 0, NULL obs, actions or logp with n > 0, action_range
 * NaN.  EB_ESTATE: a layer was never set. */
int eb_policy_logp(eb_mlp m, const eb_policy_logp_args* a);

/* The epilogue alone on logits [n, out_dim] (what eb_mlp_forward wrote, on a handle of either precision, or any other policy's
 * output): an elementwise kernel, one lane per row, no handle.  Runs on the current device.
 * Reads n, out_dim, logits, actions, action_range, logp, z_out, stream.
 * EB_EINVAL: NULL args, n < 0, out_dim odd, < 2 or > 32, NULL logits, actions or logp with n > 0, action_range NaN. */
int eb_policy_logp_from_logits(const eb_policy_logp_args* a);

/* The reverse pass above, elementwise, one lane per (row, a): g_logits [n, out_dim] from g_logp [n], the z the forward wrote
 * [n, act_dim] and the logits [n, out_dim].  Runs on the current device.  Reads n, out_dim, logits, z, g_logp, g_logits, stream.
 * EB_EINVAL: NULL args, n < 0, out_dim odd, < 2 or > 32, NULL logits, z, g_logp or g_logits with n > 0. */
int eb_policy_logp_vjp(const eb_policy_logp_args* a);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_POLICY_LOGP_H */
