/*
 * envbuild_ilqr.h — C-ABI of one iLQR / Gauss-Newton DDP iteration on the model rollout in one launch: try the previous feedback
 * gains at several step lengths, keep the best trajectory, linearise along it, sweep backwards to the next gains.
 *
 * A header of its own next to envbuild.h, envbuild_grad.h, envbuild_cand.h, envbuild_cand_grad.h and envbuild_sample.h: these symbols
 * are exported by env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle of envbuild.h has none of them), the five older ABI
 * numbers are untouched, and a binding looks the symbols up on demand.  Conventions (return codes, eb_last_error, device pointers,
 * `stream`) are those of envbuild_sample.h.
 *
 * Why the entry exists: the open-loop problem min_u J(u), J = sum_t <w5, out5_t> (EnvironmentModel.rollout_out, DAM:118-126), has six
 * ego numbers of state and two of control, closed-form dynamics (f_xu), vehicles that do not depend on the ego and a closest path
 * point that is a constant of the derivative (envbuild_grad.h).  Its cost is a non-negatively weighted sum of squares of smooth
 * residuals (DAM:198-207, 218-229, 231-298), so its Gauss-Newton Hessian is positive semi-definite by construction and Q_uu is
 * positive definite whenever w5[0] < 0.  That is the textbook case for a second-order method.
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.  fp32 obs rows only.
 */
#ifndef ENVBUILD_ILQR_H
#define ENVBUILD_ILQR_H

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_ILQR_ABI_VERSION 1

int eb_ilqr_abi_version(void);

/* One iteration (csrc/eb_rollout_tape_ilqr.hip).  One launch; no atomics to global memory.
 *
 * Candidates.  Candidate 0 is u_nom clamped to the box: x < -1 ? -1 : x > 1 ? 1 : x (two compares: a NaN stays a NaN).  Candidate
 *   j >= 1 exists only when gains (and x_nom) are given and is rolled out closed-loop.  At step t, with x the candidate's pre-step obs
 *   columns 0..5:
 *       du_a = alphas[j-1] * k[t][a];   for c = 0..5 in order:  du_a = du_a + K[t][a][c] * (x[c] - x_nom[t][c][e]);
 *       u_a = clamp(u_nom[t][e][a] + du_a).
 *   One fp32 rounding per operation, no contraction: NumPy float32 reproduces every bit.  Gains rows: 0-1 hold k, row 2 + 6 a + c
 *   holds K[a][c].  Without gains n_alpha must be 0.
 * Cost.    cost[j][e] is, bit for bit, what eb_rollout_tape_cand (include/envbuild_cand.h) returns as `cost` for that candidate's
 *   tape on the env's path without retrack.  Best is the first minimum over j; a NaN never wins; all NaN gives candidate 0.
 *   Candidate 0 is always in the set, so an accepted cost never rises.  u_out / x_out are the best candidate's tape and its pre-step
 *   obs columns 0..5; best_cost its cost's bits.
 * Quadratic model along the best candidate, in the step VJP's own space: z = obs columns 0..8, u = the raw action.
 *   A (9 x 9), B (9 x 2): row i is what eb_rollout_step_vjp returns for g_obs_out = e_i, g_out5 = 0 (columns 6..8 of A are zero);
 *   l_z, l_u: what it returns for g_obs_out = 0, g_out5 = w5;
 *   l_zz, l_uu: the Gauss-Newton Hessian 2 sum_i c_i grad(r_i) grad(r_i)^T over the residuals of DAM:198-207, 227-229, 233-295 that
 *   are ACTIVE in the forward, by the branch decisions of the reverse pass; a circle distance of exactly zero contributes zero;
 *   l_uz = 0; l_uu is diagonal, -w5[0] * (2 * 5 * 0.4^2, 2 * 0.05 * 2.25^2) where the action passes the +-1.05 clip, else 0.
 *   lq_out rows: A 81 (row-major), B 18 (row-major), l_z 9, l_u 2, l_zz 45 (upper triangle, row-major), l_uu 2.
 * Backward sweep.  V_H = 0.  Per step, last first, with V' the value of the step after:
 *       Q_z = l_z + A^T V'_z     Q_u = l_u + B^T V'_z     Q_zz = l_zz + A^T V'_zz A     Q_uz = B^T V'_zz A     Q_uu = l_uu + B^T V'_zz B
 *       Qt_uu = Q_uu + mu[e] I.
 *   k solves  min 1/2 d^T Qt_uu d + Q_u^T d  s.t.  -1 <= u_out + d <= 1  exactly, by enumeration.  A component is free (F), at its
 *   lower (L) or at its upper (U) bound; the nine sets are tried in the order (u_0, u_1) = FF, LF, UF, FL, FU, LL, LU, UL, UU and
 *   the first one is taken whose free block of Qt_uu is finite and positive definite, whose free components lie within the bounds and
 *   whose gradient Qt_uu d + Q_u is >= 0 on every L and <= 0 on every U component.  K = -Qt_uu,ff^-1 Q_uz,f on the free components;
 *   the rows of clamped components are zero.  When no set is taken (a free block that is not positive definite, or values that are
 *   not finite) the step gets k = K = 0.
 *       V_z = Q_z + K^T Q_uu k + K^T Q_u + Q_uz^T k      V_zz = Q_zz + K^T Q_uu K + K^T Q_uz + Q_uz^T K, symmetric
 *       dv = (sum_t k^T Q_u, sum_t k^T Q_uu k).
 *   The working precision of the sweep (at least fp32) and the order of its sums are the kernel's own and fixed (two launches repeat
 *   their bits); they are not part of the ABI.  gains_out and dv are rounded to fp32 once, when they are stored.
 * Independence.  An env's outputs depend only on its row, its tapes, its gains, its path, its mu and the scalars.
 *
 * Every output may be NULL; gains_out == dv == lq_out == NULL is the value-only form (no backward sweep).
 * Return codes: n_env == 0 is a no-op.  EB_EINVAL, with the reason in eb_last_error: horizon or n_alpha beyond
 * eb_rollout_tape_ilqr_max; alphas NULL with n_alpha > 0, or an entry that is not finite and > 0; w5 NULL, w5[0] > 0 or one of
 * w5[1..4] < 0 (or a NaN); one of x_nom / gains without the other; n_alpha > 0 without gains; an output pointer equal to an input
 * pointer; training mode without ref_idx; a path_id out of range in selecting mode. */
int eb_rollout_tape_ilqr(eb_handle h, int32_t n_env, int32_t horizon, int32_t n_alpha,
        const float* obs0,                 /* [n_env, D] */
        const float* u_nom,                /* [horizon, n_env, 2] raw actions */
        const float* x_nom,                /* [horizon, 6, n_env] or NULL */
        const float* gains,                /* [horizon, 14, n_env] or NULL (both or neither) */
        const int32_t* ref_idx, int32_t path_id,
        const float* alphas,               /* HOST, n_alpha floats, finite, > 0 */
        const float* mu,                   /* [n_env] device or NULL (= 0); >= 0 */
        const float* w5,                   /* HOST, 5 floats */
        float* cost, int32_t* best_index, float* best_cost,   /* [1+n_alpha, n_env], [n_env], [n_env] */
        float* u_out, float* x_out, float* gains_out,         /* layouts of u_nom / x_nom / gains */
        float* dv,                         /* [2, n_env] */
        float* cand_out,                   /* [1+n_alpha, horizon, n_env, 2]: tapes as scored (tests) */
        float* lq_out,                     /* [horizon, 157, n_env]: the quadratic model (tests) */
        void* stream);

/* The most step lengths and the longest horizon one eb_rollout_tape_ilqr launch takes on this handle (the sweep's per-step record
 * stays in the block's LDS).  `horizon` is the caller's (any value; it does not change the answer today).  max_alpha >= 7 and
 * max_horizon >= 25 for every n_veh <= 64. */
int eb_rollout_tape_ilqr_max(eb_handle h, int32_t horizon, int32_t* max_alpha, int32_t* max_horizon);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_ILQR_H */
