/*
 * envbuild_grad.h — C-ABI of the reverse pass of the model step and of the open-loop rollout (gradients through
 * EnvironmentModel.rollout_out).
 *
 * A second header next to envbuild.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle
 * of envbuild.h has no reverse pass), EB_ABI_VERSION is untouched, and a binding looks them up on demand.  Conventions
 * (return codes, eb_last_error, device pointers, `stream`) are those of envbuild.h.
 *
 * Why the gradient exists: the reference's analytic model is differentiable on purpose — model-based RL back-propagates the sum
 * of `rewards` and `punish_term_for_training` over the rollout through rollout_out (DAM:118-126), which is why compute_rewards and
 * compute_next_obses carry tf.stop_gradient on the vehicle columns (DAM:195, 331, 402).
 *
 * The gradient contract (nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh):
 *   - inputs that receive a cotangent: obs[:, :nd] and the RAW actions [n_env, 2]; the vehicle columns receive exactly zero,
 *     and next_obs[:, nd:] contributes nothing (stop_gradient);
 *   - outputs that carry one: next_obs[:, :nd] and the five arrays of out5 (rewards, punish_term_for_training, real_punish_term,
 *     veh2veh4real, veh2road4real);
 *   - the closest path point and the +80 look-ahead points come from an integer argmin / gather (DAM:702-733): constants.  The
 *     cotangent flows through ego_xs, ego_ys, ego_phis, ego_vs of tracking_error_vector (DAM:735-770) only;
 *   - a tf.where passes the cotangent to the selected branch only; a clip passes it where lo <= x <= hi and blocks it outside:
 *     actions beyond +-1.05 (DAM:129) and a clipped v_x (DAM:390) get zero;
 *   - training mode: rows whose ref_idx is out of range keep zero tracking (DAM:342, 352) and zero tracking gradient;
 *   - ONE divergence from the reference: a circle distance (DAM:227) — or, in two2one (DAM:738, 748), the distance of the next
 *     pose to the junction corner — of exactly 0 makes the reference produce NaN (the derivative of sqrt at 0); the term
 *     contributes 0 here;
 *   - fp32 state only.  The fp16-state entry points (eb_rollout_step_f16 / eb_rollout_tape_f16), the gated kernel and second
 *     derivatives have no reverse pass; obs rows here are always fp32.  The open-loop tape has one: eb_rollout_tape_vjp.
 */
#ifndef ENVBUILD_GRAD_H
#define ENVBUILD_GRAD_H

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_GRAD_ABI_VERSION 2

int eb_grad_abi_version(void);

/* Reverse of eb_rollout_step (EnvironmentModel.rollout_out, DAM:118-126) at (obs_in, actions): the action transform
 * (DAM:128-132), compute_rewards (DAM:186-320: the six quadratic terms, the two-circle penalties DAM:218-229, the road walls
 * DAM:231-295), ego_predict (f_xu with tau = 0.1, DAM:52-83, and the v_x clip, DAM:386-392) and tracking_error_vector of the
 * next pose (DAM:735-770), transposed.  Recomputes from obs_in and actions: the forward saves nothing.  One launch.
 *   obs_in     [n_env, D] the PRE-step obs; actions [n_env, 2] raw; ref_idx / path_id as in eb_rollout_step;
 *   g_obs_out  cotangent of the next obs, row stride ld_out floats (>= nd; only the first nd columns of a row are read);
 *              NULL = zeros;
 *   g_out5     [5, n_env] cotangents of out5; NULL = zeros;
 *   g_obs_in   row stride ld_in: ld_in == nd writes compact rows [n_env, nd]; ld_in == D writes full rows whose vehicle
 *              columns are zero-filled (the first nd columns are the same bits either way);
 *   g_actions  [n_env, 2], with respect to the RAW actions.
 * n_env == 0 is a no-op; training mode without ref_idx is EB_EINVAL.  A row's result does not depend on its position in the
 * batch, and a launch repeats its bits. */
int eb_rollout_step_vjp(eb_handle h, int32_t n_env, const float* obs_in, const float* actions, const int32_t* ref_idx,
                        int32_t path_id, const float* g_obs_out, int32_t ld_out, const float* g_out5, float* g_obs_in,
                        int32_t ld_in, float* g_actions, void* stream);

/* Reverse sweep of an open-loop chain of `horizon` steps (eb_rollout_tape / `horizon` calls of eb_rollout_step; the MPC callers'
 * cost_function, mpc/main.py:470-479, and ADP's rollout loss):
 *   obs_steps     [horizon, n_env, D]: the PRE-step obs of every step (obs_steps[t] = obs_in of step t);
 *   action_tape   [horizon, n_env, 2] raw;
 *   g_obs_final   cotangent of the obs after the last step, row stride ld_final (>= nd); NULL = zeros;
 *   g_out5_steps  [horizon, 5, n_env]; NULL = zeros;
 *   g_work        scratch [n_env, nd];
 *   g_obs0        [n_env, nd]: cotangent of obs_steps[0][:, :nd];
 *   g_action_tape [horizon, n_env, 2].
 * `horizon` launches, last step first; the same bits as `horizon` calls of eb_rollout_step_vjp with compact rows. */
int eb_rollout_chain_vjp(eb_handle h, int32_t n_env, int32_t horizon, const float* obs_steps, const float* action_tape,
                         const int32_t* ref_idx, int32_t path_id, const float* g_obs_final, int32_t ld_final,
                         const float* g_out5_steps, float* g_work, float* g_obs0, float* g_action_tape, void* stream);

/* Value and gradient of an open-loop rollout of `horizon` steps in ONE launch (ABI 2): the forward sweep of eb_rollout_tape and
 * the reverse sweep of eb_rollout_chain_vjp, with the tape kept in registers and LDS (csrc/eb_rollout_tape_vjp.hip).  What an MPC
 * solver calls per evaluation of  J(u) = sum_t <w, out5_t(u)>  (the callers' cost_function, mpc/main.py:470-479).
 *   obs0          [n_env, D];  action_tape [horizon, n_env, 2] raw;  ref_idx / path_id as in eb_rollout_step;
 *   g_obs_final   cotangent of the obs after the last step, row stride ld_final (>= nd); NULL = zeros;
 *   g_out5_steps  [horizon, 5, n_env] cotangents of every step's out5, or NULL: then
 *   w5            HOST pointer to 5 floats — the cotangent of out5 row k at every step and env; NULL = zeros.  Equals a
 *                 g_out5_steps array filled with those five values;
 *   out5_steps    [horizon, 5, n_env] or NULL: the forward's outputs — the bits of eb_rollout_tape;
 *   obs_out       [n_env, D] or NULL: the obs after the last step — the bits of eb_rollout_tape;
 *   g_obs0        [n_env, nd] or NULL: cotangent of obs0[:, :nd];
 *   g_action_tape [horizon, n_env, 2] or NULL.  g_obs0 == g_action_tape == NULL is the value-only form: no reverse sweep.
 * Gradients are the bits of `horizon` calls of eb_rollout_step that keep every pre-step obs followed by eb_rollout_chain_vjp with
 * the same cotangents; the gradient contract above holds unchanged (vehicle columns are never written).  A row's bits do not depend
 * on its position in the batch or on its neighbours, and a launch repeats its bits.  No atomics to global memory.
 * horizon above eb_rollout_tape_vjp_max_horizon (>= 25 for every n_veh <= 64) is EB_EINVAL with the limit in eb_last_error: compose
 * eb_rollout_step and eb_rollout_chain_vjp instead.  n_env == 0 is a no-op; training mode without ref_idx is EB_EINVAL. */
int eb_rollout_tape_vjp(eb_handle h, int32_t n_env, int32_t horizon, const float* obs0, const float* action_tape,
                        const int32_t* ref_idx, int32_t path_id, const float* g_obs_final, int32_t ld_final,
                        const float* g_out5_steps, const float* w5, float* out5_steps, float* obs_out, float* g_obs0,
                        float* g_action_tape, void* stream);

/* The longest horizon eb_rollout_tape_vjp takes on this handle (its tile must fit the LDS; depends on n_veh). */
int eb_rollout_tape_vjp_max_horizon(eb_handle h, int32_t* max_horizon);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_GRAD_H */
