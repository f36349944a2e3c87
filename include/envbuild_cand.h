/*
 * envbuild_cand.h — C-ABI of the candidate-tape rollout: the value of K open-loop action tapes per env from ONE shared scene, in one
 * launch.
 *
 * A third header next to envbuild.h and envbuild_grad.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY (the
 * CPU oracle of envbuild.h has none of them), EB_ABI_VERSION and EB_GRAD_ABI_VERSION are untouched, and a binding looks them up on
 * demand.  Conventions (return codes, eb_last_error, device pointers, `stream`) are those of envbuild.h.
 *
 * Why the entry exists: everything that plans on the model scores several action sequences from one state — the reference's decision
 * loop scores one candidate per path of the task (hier_decision.py:113-121), a line search several step lengths, a multi-start solver
 * its starts.  The vehicles of a scene do not depend on the ego (tf.stop_gradient on the vehicle columns, DAM:195, 331, 402, and
 * predict_for_a_mode, DAM:405-427, reads the vehicle's own record only), so the K rollouts share one vehicle trajectory: it is
 * computed once per env, and only the ego's chain (DAM:128-132, 186-320, 386-392, 735-770) runs per candidate.
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.  fp32 obs rows only: the fp16-state kernels (eb_rollout_step_f16 /
 * eb_rollout_tape_f16) have no candidate form.
 */
#ifndef ENVBUILD_CAND_H
#define ENVBUILD_CAND_H

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_CAND_ABI_VERSION 1

int eb_cand_abi_version(void);

/* Value-only open-loop rollout of n_cand action tapes per env over `horizon` model steps (EnvironmentModel.rollout_out, DAM:118-126,
 * chained as the MPC callers' cost_function chains it, mpc/main.py:470-479), every candidate starting from the same row of obs0
 * (csrc/eb_rollout_tape_cand.hip).  One launch; no atomics to global memory.
 *   obs0          [n_env, D], shared by the candidates; never written;
 *   action_tapes  [n_cand, horizon, n_env, 2] raw actions (DAM:128-132): slice k is an eb_rollout_tape tape;
 *   ref_idx, ref_ld   training mode (DAM:340-347): candidate k follows path ref_idx[k * ref_ld + env].  ref_ld == 0: one [n_env] array
 *                 for all candidates; otherwise ref_ld >= n_env.  An id out of range keeps zero tracking (DAM:342, 352);
 *   path_ids, path_id   selecting mode (DAM:348-353): path_ids is a HOST array of n_cand path ids, or NULL: path_id for all;
 *   retrack       != 0: before step 0 every (env, candidate) replaces the tracking triple of its private copy of the row (columns
 *                 6-8) by the tracking error of the row's own pose on the candidate's path (tracking_error_vector, DAM:735-760) — the
 *                 bits eb_tracking_error(x = column 3, y = column 4, phi = column 5, v = column 0) gives for that path; a candidate
 *                 whose ref_idx is out of range gets zeros (DAM:342, 352).  This is what makes candidates on different paths
 *                 meaningful from one shared row: the reference builds one obs per path (hier_decision.py:113-117).
 *                 0: obs0's columns 6-8 as they are.  The look-ahead columns of obs0 feed no output of this entry
 *                 (DAM:189-207, 322-333);
 *   w5            HOST pointer to 5 floats, the weights of `cost`; may be NULL when cost is NULL;
 *   out5_steps    [n_cand, horizon, 5, n_env] or NULL: out5_steps[k] is, bit for bit, eb_rollout_tape's out5_steps (rewards,
 *                 punish_term_for_training, real_punish_term, veh2veh4real, veh2road4real; DAM:297-300) for (obs0, action_tapes[k],
 *                 candidate k's path) — also the bits of the value-only eb_rollout_tape_vjp;
 *   cost          [n_cand, n_env] or NULL: cost[k][e] = sum over t of s_t, accumulated in fp32 in ascending t from +0, where s_t is
 *                 the sum, in row order r = 0..4 over the rows with w5[r] != 0, of out5_t[r] * w5[r].  Every operation is one fp32
 *                 rounding (no contraction); all weights zero gives +0.  The per-step expression is that of the Python package's
 *                 mpc.cost_from_out5 (the callers' J, mpc/main.py:470-479); the order over the steps is fixed HERE, while
 *                 cost_from_out5 leaves it to torch's reduction: the two agree to rounding, not bit for bit.
 * A (row, candidate)'s bits do not depend on the row's position in the batch, on the other rows, or on the other candidates of the
 * set, and a launch repeats its bits.
 * Return codes: n_env == 0 or n_cand == 0 is a no-op.  EB_EINVAL: out5_steps == cost == NULL; cost != NULL with w5 == NULL;
 * 0 < ref_ld < n_env or ref_ld < 0; training mode without ref_idx; a path id out of range in selecting mode; horizon < 1 or > 128;
 * n_cand above eb_rollout_tape_cand_max, with the limit in eb_last_error (evaluate the set in chunks: candidates are independent). */
int eb_rollout_tape_cand(eb_handle h, int32_t n_env, int32_t n_cand, int32_t horizon, const float* obs0, const float* action_tapes,
                         const int32_t* ref_idx, int32_t ref_ld, const int32_t* path_ids, int32_t path_id, int32_t retrack,
                         const float* w5, float* out5_steps, float* cost, void* stream);

/* The most candidates one eb_rollout_tape_cand launch takes on this handle for `horizon` steps: its per-(env, candidate, slot) queue
 * (the two-circle penalty terms of the near vehicles, DAM:218-229) must fit the LDS, so the limit depends on n_veh.  At least 8 for
 * n_veh <= 32 and at least 4 for n_veh <= 64 at horizon <= 128. */
int eb_rollout_tape_cand_max(eb_handle h, int32_t horizon, int32_t* max_cand);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_CAND_H */
