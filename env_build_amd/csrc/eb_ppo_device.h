// eb_ppo_device.h — the PPO update's row functions, written once: the clipped surrogate of one row (called by the fused kernel and by
// the elementwise one of eb_ppo.hip) and one step of generalised advantage estimation.  The arithmetic contract is the header comment
// of include/envbuild_ppo.h: every line there is one fp32 rounding here.  The log-probability and its reverse pass are
// eb_policy_logp_device.h's, the exponential eb_mlp_device.h's: they are only called.  Everything is EB_DEV.
#pragma once
#include "eb_policy_logp_device.h"
#include "eb_ppo.h"

#pragma clang fp contract(off)

namespace eb {
namespace ppo {

// ---- one row.  y: the row's activated logits [2 * act_dim] in LDS, owned by this lane and OVERWRITTEN: plogp::logp_row is handed y as
//      its z_out, so y[a] (the mean, which nothing reads after z is formed) becomes z[a] and y[act_dim + a] stays ls[a].  That keeps the
//      act_dim z values the reverse pass needs out of a register array indexed by a run-time a (scratch memory).  e: the row's index in
//      the batch.  Writes what S names, in ascending a. ----
EB_DEV void surrogate_row(float* y, int act_dim, size_t e, const PpoHead& S) {
    float logp;
    plogp::logp_row(y, act_dim, S.actions + e * act_dim, S.action_range, S.log_ar, &logp, y);
    float A = S.adv[e];
    if (S.adv_norm) A = (A - S.adv_norm[0]) * S.adv_norm[1];
    const float d = logp - S.logp_old[e];
    const float r = mlp::exp_det(d);
    const float s1 = r * A;
    const float rc = r < S.lo ? S.lo : (r > S.hi ? S.hi : r);            // a NaN falls through both compares
    const float s2 = rc * A;
    const float surr = s2 < s1 ? s2 : s1;
    const bool blocked = (r < S.lo || r > S.hi) && (s2 <= s1);           // a NaN in r or A: not blocked
    const float g_lp = blocked ? 0.0f : (S.w * A) * r;
    S.logp[e] = logp;
    if (S.ratio) S.ratio[e] = r;
    if (S.surr) S.surr[e] = surr;
    float sum = 0.0f;
    float* g = S.g_logits ? S.g_logits + e * (size_t)(2 * act_dim) : nullptr;
    for (int a = 0; a < act_dim; ++a) {
        const float z = y[a], ls = y[act_dim + a];
        sum = sum + ls;
        if (S.z_out) S.z_out[e * act_dim + a] = z;
        if (g) {
            float g_mean, g_ls;
            plogp::logp_vjp_elem(ls, z, g_lp, g_mean, g_ls);
            g[a] = g_mean;
            g[act_dim + a] = g_ls + S.g_ent;
        }
    }
    if (S.ent) S.ent[e] = sum + (float)act_dim * 1.4189385332f;
}

// ---- one step of generalised advantage estimation: run is the recursion's state ----
EB_DEV float gae_step(float reward, float value, float vn, float nonterminal, float carry, float gamma, float gl, float run) {
    const float delta = (reward + (gamma * vn) * nonterminal) - value;
    return delta + (gl * carry) * run;
}

}  // namespace ppo
}  // namespace eb
