/*
 * envbuild_ppo.h — C-ABI of the PPO update's arithmetic: generalised advantage estimation over [T, n] arrays in ONE launch (eb_gae),
 * and the clipped surrogate with its entropy bonus and the cotangent of the logits in ONE launch with the fp32 policy network
 * (eb_ppo_surrogate), or alone on given logits (eb_ppo_surrogate_from_logits): csrc/eb_ppo.hip.  envbuild_policy_logp.h gives a
 * trainer log pi(a | obs) of stored actions; what a PPO minibatch does with it — the ratio to logp_old, the clamp, the minimum, the
 * entropy of the Gaussian before the squash, and the derivative of all that with respect to the logits — is a closed-form function of
 * one row, and it is evaluated here in the epilogue that already holds the row's logits.  g_logits leaves the forward launch finished:
 * the backward of a minibatch is eb_mlp_backward(head = 0) alone.
 *
 * A header of its own next to envbuild_policy_logp.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY,
 * EB_ABI_VERSION and every other family's version are untouched, and a binding looks them up on demand.  Conventions (return codes,
 * eb_last_error, device pointers) are those of envbuild.h.  Nothing here synchronises, allocates or uses atomics.
 *
 * The three working entries take ONE struct.  Their stream is therefore a field, not a parameter, and the table of stream-taking
 * prototypes (tests/test_stream_census.py) does not count them: this family's own tests hold each of them to that table's obligations
 * (a side stream, capture, replay).  Every scalar and every pointer of a struct is read AT CALL TIME: under stream capture those
 * values are baked into the graph, and the device buffers they point to — adv_norm's two floats included — are read at every replay
 * (envbuild.h's capture bullet).
 *
 * The surrogate row.  y [n, out_dim] is what eb_mlp_forward returns, that is, after the output activation; act_dim = out_dim / 2;
 * ls = y[:, act_dim:].  Every line below is one fp32 rounding (-ffp-contract=off, an explicit fmaf only inside the named functions):
 *
 *   logp, z, inv                                    # envbuild_policy_logp.h's contract, line by line: the SAME device function is
 *                                                   # called, so logp and z are eb_policy_logp's bits
 *   A    = adv_norm ? (adv - adv_norm[0]) * adv_norm[1] : adv     # adv_norm: DEVICE pointer to (mean, 1 / std), or NULL; the host
 *                                                                 # never reads it
 *   d    = logp - logp_old           r = exp_det(d)                # the ratio
 *   s1   = r * A                     rc = r < lo ? lo : (r > hi ? hi : r)     # lo = 1.0f - clip, hi = 1.0f + clip, formed on the host
 *   s2   = rc * A                    surr = s2 < s1 ? s2 : s1                 # selects: a NaN travels
 *   ent  = (sum of ls over a = 0 .. act_dim-1, ascending, from +0.0f) + (float)act_dim * 1.4189385332f
 *                                                   # 0.5 log(2 pi e) per dimension: the entropy of the Gaussian BEFORE the squash
 *   blocked = (r < lo || r > hi) && (s2 <= s1)
 *   g_lp = blocked ? 0.0f : (w * A) * r             # w = -scale
 *   g_y[:, a]           = g_lp * (z * inv)          # envbuild_policy_logp.h's reverse pass, the same device function
 *   g_y[:, act_dim + a] = g_lp * (z * z - 1.0f) + g_ent            # g_ent = -(scale * ent_coef), ONE product formed on the host
 *
 * g_y is the cotangent of y for the objective  -scale * sum(surr) - scale * ent_coef * sum(ent)  with A held constant: what
 * eb_mlp_backward(head = 0) takes as g_out.  scale = 1 / n makes it the PPO policy loss -mean(surr) - ent_coef * mean(ent).  surr and
 * ent are written unscaled.
 *
 * The ratio is what exp_det returns, beyond its clamps too: exp_det takes d > 88 as 88 and d < -87 as -87, so r lies in
 * [exp_det(-87), exp_det(88)] ~ [1.6e-38, 1.65e38] for every finite or infinite d, never 0 and never inf; a NaN d gives a NaN r.
 * logp - logp_old = 0 gives r = 1.0f exactly (exp_det(0) is 1): with logp_old taken from eb_policy_logp on the same weights the
 * first pass over a batch has ratio 1.0 on every row.
 *
 * `blocked` with finite values is autograd's torch.min(ratio * A, ratio.clamp(lo, hi) * A), ties included: the clamp passes its
 * gradient on the closed interval [lo, hi], and where the two products are equal torch.min gives each argument half of the cotangent.
 *   r inside [lo, hi] (r == lo, r == hi and r == 1 included): rc == r, s2 == s1, the clamp passes: the full gradient (half + half).
 *   r outside, s2 < s1: the clamped product is the minimum and its derivative is 0: blocked.
 *   r outside, s2 > s1: the unclamped product is the minimum: the full gradient.
 *   r outside, s2 == s1 (A == 0, or both products rounded to the same number): torch gives HALF of (w * A) * r, here it is 0.
 *     With A == 0 both are 0.  With A != 0 it needs r * A and rc * A to round to the same float with r != rc, which takes an |A|
 *     small enough for the products to leave the normal range (below about 1e-37 / hi): the one tie split otherwise than torch.  The
 *     tests stay off it.
 * A NaN in r or A makes every comparison false: the row is NOT blocked, g_lp is NaN, and the row poisons itself only.
 *
 * clip = 0 gives lo = hi = 1: every r != 1 is outside.  The entropy term does not depend on the actions.
 *
 * Generalised advantage estimation.  Arrays are [T, n], t-major (element (t, i) at t * n + i); one lane per env walks t = T-1 .. 0.
 * Each line is one rounding, in exactly this order:
 *
 *   vn    = next_values ? next_values[t] : (t == T - 1 ? v_last : values[t + 1])
 *   delta = (rewards[t] + (gamma * vn) * nonterminal[t]) - values[t]
 *   run   = delta + (gl * carry[t]) * run           # run starts at +0.0f; gl = (float)((double)gamma * (double)lam), on the host;
 *                                                   # gamma in the line above is (float)gamma
 *   adv[t] = run                     ret[t] = run + values[t]      # ret or NULL
 *
 * carry NULL means nonterminal.  nonterminal and carry are FLOATS (1.0f where the episode goes on, 0.0f where the step ended it), v_last
 * is [n].  With next_values = NULL and carry = NULL the lines are the torch loop of examples/ppo_env_loop.py operation for operation,
 * and eb_gae equals it bit for bit.  Separate next_values and carry let a trainer bootstrap a time-limit truncation from the value of
 * info['final_observation'] (nonterminal = 1, carry = 0 at that step) without a second entry.
 *
 * Rows (envs) are independent; n = 0 is a no-op that needs no pointer; a refusal names its entry in eb_last_error and writes nothing;
 * a NaN scalar is refused; inf and NaN in the arrays travel as IEEE arithmetic carries them and poison their own row (env) only;
 * repeated calls repeat their bits.  eb_ppo_surrogate equals eb_mlp_forward followed by eb_ppo_surrogate_from_logits bit for bit, its
 * logits_out equals eb_mlp_forward, its logp and z_out equal eb_policy_logp's.
 * The Python package restates this contract in NumPy: env_build_amd.ppo.ppo_reference and gae_reference.
 */
#ifndef ENVBUILD_PPO_H
#define ENVBUILD_PPO_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_PPO_ABI_VERSION 1

/* Which entry reads which field is on the right; a field an entry does not read may hold anything. */
typedef struct eb_ppo_args {
    int32_t n, out_dim;        /* out_dim: read by from_logits only (the fused entry takes the handle's) */
    const float* obs;          /* [n, obs_dim]          fused entry */
    const float* logits;       /* [n, out_dim]          from_logits */
    const float* actions;      /* [n, act_dim] */
    const float* logp_old;     /* [n] */
    const float* adv;          /* [n] */
    const float* adv_norm;     /* [2] on the DEVICE: (mean, 1 / std), or NULL: adv is used as it is */
    float action_range;        /* > 0: squashed; <= 0: the reference's action_range=None; NaN refused */
    float clip;                /* >= 0; NaN refused */
    float ent_coef;            /* NaN refused */
    float scale;               /* the weight of a row in the objective, 1 / n for a mean; NaN refused */
    float* logp;               /* [n]                   required */
    float* ratio;              /* [n] or NULL */
    float* surr;               /* [n] or NULL           unscaled */
    float* ent;                /* [n] or NULL           unscaled */
    float* g_logits;           /* [n, out_dim] or NULL  NULL: evaluation only */
    float* logits_out;         /* [n, out_dim] or NULL  fused entry */
    float* z_out;              /* [n, act_dim] or NULL  the standardised pre-squash value */
    void* stream;
} eb_ppo_args;

typedef struct eb_gae_args {
    int32_t T, n;              /* T in 1..65535, n >= 0 */
    const float* rewards;      /* [T, n] */
    const float* values;       /* [T, n] */
    const float* v_last;       /* [n]: the value after the last step; not read when next_values is given */
    const float* nonterminal;  /* [T, n]: 1.0f / 0.0f */
    const float* next_values;  /* [T, n] or NULL */
    const float* carry;        /* [T, n] or NULL: nonterminal */
    double gamma, lam;         /* finite.  DOUBLES, what a Python trainer holds: the kernel multiplies by (float)gamma, and gl is the
                                  product of the two doubles rounded once, which is what torch makes of `gamma * lam * tensor` */
    float* adv;               /* [T, n] */
    float* ret;                /* [T, n] or NULL */
    void* stream;
} eb_gae_args;

int eb_ppo_abi_version(void);

/* ok = 1 when eb_ppo_surrogate accepts this handle as it stands: the conditions of eb_policy_logp_supported (precision
 * EB_MLP_PRECISION_F32, every layer set, out_dim even and >= 2).  Else 0 with the first unmet condition in eb_last_error; an fp16
 * handle is refused by name: eb_ppo_surrogate_from_logits serves it.  EB_EINVAL: NULL handle or NULL ok. */
int eb_ppo_surrogate_supported(eb_mlp m, int32_t* ok);

/* The fused launch: the network of eb_mlp_forward and the surrogate row above, ALWAYS exactly one launch on a->stream.
 * Reads every field but out_dim and logits.
 * EB_EINVAL (nothing written): NULL handle or args, an unsupported handle, n < 0, NULL obs, actions, logp_old, adv or logp with n > 0,
 * action_range, clip, ent_coef or scale NaN, clip < 0.  EB_ESTATE: a layer was never set. */
int eb_ppo_surrogate(eb_mlp m, const eb_ppo_args* a);

/* The surrogate row alone on logits [n, out_dim] (what eb_mlp_forward wrote, on a handle of either precision, or any other policy's
 * output): an elementwise kernel, one lane per row, no handle.  Runs on the current device.  Reads every field but obs and logits_out.
 * EB_EINVAL: NULL args, n < 0, out_dim odd, < 2 or > 32, NULL logits, actions, logp_old, adv or logp with n > 0, action_range, clip,
 * ent_coef or scale NaN, clip < 0. */
int eb_ppo_surrogate_from_logits(const eb_ppo_args* a);

/* Generalised advantage estimation as stated above: one launch, one lane per env.  Runs on the current device.
 * EB_EINVAL: NULL args, T < 1 or > 65535, n < 0, gamma or lam not finite, NULL rewards, values, nonterminal or adv with n > 0, NULL
 * v_last with n > 0 and next_values NULL. */
int eb_gae(const eb_gae_args* a);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_PPO_H */
