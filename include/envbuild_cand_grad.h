/*
 * envbuild_cand_grad.h — C-ABI of the candidate-tape value-and-gradient rollout: cost AND gradient of K open-loop action tapes per env
 * from ONE shared scene, in one launch.
 *
 * A fourth header next to envbuild.h, envbuild_grad.h and envbuild_cand.h: these symbols are exported by
 * env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle of envbuild.h has none of them), EB_ABI_VERSION, EB_GRAD_ABI_VERSION and
 * EB_CAND_ABI_VERSION are untouched, and a binding looks them up on demand.  Conventions (return codes, eb_last_error, device
 * pointers, `stream`) are those of envbuild.h.
 *
 * Why the entry exists: eb_rollout_tape_cand ranks K tapes; a planner that improves them — the starts of a multi-start solver on the
 * non-convex collision cost, one tape per path of the task before the decision loop compares the paths (hier_decision.py:113-121) —
 * needs dJ/du of every one.  The vehicles of a scene do not depend on the ego (tf.stop_gradient on the vehicle columns, DAM:195, 331,
 * 402), so the K rollouts share one vehicle trajectory, computed once per env; the ego's forward chain (DAM:128-132, 186-320, 386-392,
 * 735-770) and its reverse run per (env, candidate).
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.  fp32 obs rows only.
 */
#ifndef ENVBUILD_CAND_GRAD_H
#define ENVBUILD_CAND_GRAD_H

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_CAND_GRAD_ABI_VERSION 1

int eb_cand_grad_abi_version(void);

/* Open-loop rollout of n_cand action tapes per env over `horizon` model steps (EnvironmentModel.rollout_out, DAM:118-126, chained as
 * the MPC callers' cost_function chains it, mpc/main.py:470-479), every candidate from the same row of obs0, with the gradient of
 *     J[k][e] = sum_t  w5 . out5_t[k][e]
 * with respect to candidate k's raw actions and to its private copy of the row (csrc/eb_rollout_tape_cand_vjp.hip).  One launch; no
 * atomics to global memory.
 *   obs0          [n_env, D], shared by the candidates; never written;
 *   action_tapes  [n_cand, horizon, n_env, 2] raw actions (DAM:128-132): slice k is an eb_rollout_tape tape;
 *   ref_idx, ref_ld   training mode (DAM:340-347): candidate k follows path ref_idx[k * ref_ld + env].  ref_ld == 0: one [n_env] array
 *                 for all candidates; otherwise ref_ld >= n_env.  An id out of range keeps zero tracking (DAM:342, 352);
 *   path_ids, path_id   selecting mode (DAM:348-353): path_ids is a HOST array of n_cand path ids, or NULL: path_id for all;
 *   retrack       != 0: before step 0 every (env, candidate) replaces the tracking triple of its private copy of the row (columns
 *                 6-8) by the tracking error of the row's own pose on the candidate's path (tracking_error_vector, DAM:735-760), as
 *                 eb_rollout_tape_cand does (hier_decision.py:113-117 builds one obs per path);
 *   w5            HOST pointer to 5 floats, required: the weights of `cost` AND the cotangent — row r of out5 at every step, env and
 *                 candidate gets w5[r], eb_rollout_tape_vjp's w5 form (the J of mpc/main.py:470-479 is such a sum).  Per-step
 *                 cotangent arrays (eb_rollout_tape_vjp's g_out5_steps) and a cotangent of the final obs (g_obs_final) are NOT
 *                 part of this entry: use eb_rollout_tape_vjp per candidate for those;
 *   out5_steps    [n_cand, horizon, 5, n_env] or NULL: the bits of eb_rollout_tape_cand's (hence of eb_rollout_tape's) out5_steps;
 *   cost          [n_cand, n_env] or NULL: the bits of eb_rollout_tape_cand's cost (the order include/envbuild_cand.h fixes);
 *   g_obs0        [n_cand, n_env, nd] or NULL: cotangent of each candidate's PRIVATE COPY of the row's first nd columns — with
 *                 retrack != 0 that is the row after its tracking triple was replaced; the chain through the replacement (columns
 *                 3-5 and 0 into the new triple) is not taken.  Columns 9.. are zero (DAM:189-207, 322-333);
 *   g_action_tapes  [n_cand, horizon, n_env, 2], required: dJ[k] / d action_tapes[k] (through action_transform, DAM:128-132).
 * g_action_tapes[k] and g_obs0[k] are, bit for bit, what eb_rollout_tape_vjp gives for (obs0 — its columns 6-8 replaced as above when
 * retrack != 0 —, action_tapes[k], candidate k's path, the same w5, no g_out5_steps, no g_obs_final).  A (row, candidate)'s bits do
 * not depend on the row's position in the batch, on the other rows, or on the other candidates of the set, and a launch repeats its
 * bits.
 * Return codes: n_env == 0 or n_cand == 0 is a no-op.  EB_EINVAL: g_action_tapes == NULL (the value-only form is
 * eb_rollout_tape_cand); w5 == NULL; 0 < ref_ld < n_env or ref_ld < 0; training mode without ref_idx; a path id out of range in
 * selecting mode; horizon < 1 or > 128; n_cand above eb_rollout_tape_cand_vjp_max, with the limit in eb_last_error (evaluate the
 * set in chunks: candidates are independent). */
int eb_rollout_tape_cand_vjp(eb_handle h, int32_t n_env, int32_t n_cand, int32_t horizon, const float* obs0, const float* action_tapes,
                             const int32_t* ref_idx, int32_t ref_ld, const int32_t* path_ids, int32_t path_id, int32_t retrack,
                             const float* w5, float* out5_steps, float* cost, float* g_obs0, float* g_action_tapes, void* stream);

/* The most candidates one eb_rollout_tape_cand_vjp launch takes on this handle for `horizon` steps.  A block keeps, per (env,
 * candidate), 22 bytes of queue per vehicle slot and 48 bytes of tape per step in 64 KB of LDS, 8 envs at least, 64 (env, candidate)
 * lanes at most: max_cand = min(8, 65536 / (176 * n_veh + 384 * horizon)).  At horizon 25 that is 4 for n_veh <= 32 and 3 — one per
 * path of a task — for n_veh <= 64.  0 when the horizon leaves room for no candidate; eb_rollout_tape_cand_vjp then refuses. */
int eb_rollout_tape_cand_vjp_max(eb_handle h, int32_t horizon, int32_t* max_cand);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_CAND_GRAD_H */
