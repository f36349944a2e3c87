/*
 * envbuild_policy_rollout_grad.h — C-ABI of the closed-loop rollout WITH its gradient: `steps` model steps under an fp32 policy
 * network, the value of the rollout and its gradient with respect to the policy's parameters, in three launches whatever `steps` is
 * (csrc/eb_policy_rollout_grad.hip, then the row reduction of csrc/eb_policy_grad.hip).
 *
 * A header of its own next to envbuild_policy_rollout.h and envbuild_mlp_grad.h: these symbols are exported by
 * env_build_amd/lib/libenvbuild_hip.so ONLY, EB_ABI_VERSION and every other family's version are untouched, and a binding looks them
 * up on demand.  Conventions (return codes, eb_last_error, device pointers, `stream`) are those of envbuild.h.
 *
 * Why the entry exists: a training step of the policy on the model (ADP: J = sum over envs and steps of the weighted out5) is, through
 * the other headers, per step of the horizon eb_policy_run_batch + eb_rollout_step on the way forward and eb_rollout_step_vjp +
 * eb_mlp_backward (three launches, the policy's forward recomputed) on the way back, plus one accumulation of every parameter's
 * gradient per step.  Here a block keeps its 64 envs on the compute unit for both sweeps, and the parameter gradient is ONE row
 * reduction over steps * n_env rows.
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.  n_pad = n_env rounded up to a multiple of 64.
 */
#ifndef ENVBUILD_POLICY_ROLLOUT_GRAD_H
#define ENVBUILD_POLICY_ROLLOUT_GRAD_H

#include "envbuild.h"
#include "envbuild_mlp_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_POLICY_ROLLOUT_GRAD_ABI_VERSION 1
#define EB_POLICY_ROLLOUT_GRAD_MAX_STEPS 128

int eb_policy_rollout_grad_abi_version(void);

/* *ok = 1 when eb_policy_rollout_grad takes this pair of handles, 0 otherwise, with the first unmet condition in eb_last_error:
 *   the policy handle is one eb_mlp_grad_supported accepts: precision EB_MLP_PRECISION_F32 (the gradient is that of the fp32 forward;
 *     a binary16 handle is refused for envbuild_mlp_grad.h's reason), hidden width, padded, at most 256, every layer set;
 *   the policy's obs_dim is the model's D and its out_dim is 4 (mean and log-std of two actions);
 *   the model has n_veh <= 32 and n_future == 0 (the reference's default); the state is fp32 rows;
 *   both handles live on one device;
 *   the block's LDS (the 64 rows and the fp32 activations) fits a compute unit.
 * Returns EB_OK either way; EB_EINVAL: a NULL handle or NULL ok. */
int eb_policy_rollout_grad_supported(eb_handle h, eb_mlp policy, int32_t* ok);

/* Bytes of workspace eb_policy_rollout_grad needs for n_env envs and `steps` steps (0 for n_env == 0): eb_mlp_backward's arrays for
 * steps * n_pad rows and 16 floats of tape per row.  EB_EINVAL: NULL handles or bytes, a refused pair, n_env < 0, steps outside
 * 1 .. EB_POLICY_ROLLOUT_GRAD_MAX_STEPS, or more rows than one row reduction takes (steps * n_pad > 65535 * 2048). */
int eb_policy_rollout_grad_workspace_bytes(eb_handle h, eb_mlp policy, int32_t n_env, int32_t steps, size_t* bytes);

/* `steps` steps of [actions = eb_policy_run_batch(policy, obs, action_range); obs, out5 = eb_rollout_step(h, obs, actions)] for n_env
 * envs from obs_in, and the reverse sweep through both.  ALWAYS the same three launches: a pair eb_policy_rollout_grad_supported
 * refuses is EB_EINVAL with the same reason, never another code path.  No atomics; nothing waits on another block.
 *   obs_in           [n_env, D]; never written;
 *   ref_idx          training mode (DAM:340-347): [n_env] path of each env; an id out of range keeps zero tracking;
 *   path_id          selecting mode (DAM:348-353);
 *   action_range     eb_policy_run_batch's: > 0 scales tanh(mean), otherwise the mean itself is the action;
 *   w5               HOST pointer, 5 floats: the weights of `cost` AND the cotangent of out5 at every step and env
 *                    (eb_rollout_tape_cand_vjp's form).  ADP's loss: (-1, lambda, 0, 0, 0) / (steps * n_env);
 *   workspace        device memory of at least eb_policy_rollout_grad_workspace_bytes; its contents afterwards are unspecified;
 *   obs_out          [n_env, D] or NULL: the state after the last step; must not alias obs_in;
 *   out5_steps       [steps, 5, n_env] or NULL;  actions_steps [steps, n_env, 2] or NULL;  obs_steps [steps, n_env, D] or NULL (the
 *                    state AFTER step t): bit for bit `steps` x [eb_policy_run_batch -> eb_rollout_step] through the two handles;
 *   cost             [n_env] or NULL: eb_rollout_tape_cand's cost (the expression and order envbuild_cand.h fixes) of this rollout's out5;
 *   g_actions_steps  [steps, n_env, 2] or NULL: the cotangent of the raw action of step t;
 *   g_obs0           [n_env, 9] or NULL: the cotangent of obs_in's columns 0..8.  Both are bit for bit what this loop of single
 *                    calls gives, t = steps - 1 .. 0, lambda_steps = 0:
 *                      (s_t, g_a_t) = eb_rollout_step_vjp(obs_t, a_t, g_obs_out = lambda_{t+1}, g_out5 = w5 at every env);
 *                      p_t = eb_mlp_backward(obs_t, g_out = g_a_t, head 1, action_range)'s g_obs;
 *                      lambda_t = s_t[:, :9] + p_t[:, :9] (one fp32 add per element; the policy's cotangent of the vehicle columns
 *                      is dropped: stop_gradient, DAM:195, 331, 402);
 *   g_params         flat, unpadded, eb_mlp_param_count floats, or NULL: dJ/dtheta for J = sum of cost.  By definition
 *                    eb_mlp_backward's g_params for the steps * n_env rows (t, env), t-major, with obs = obs_t and g_out = g_a_t, up
 *                    to the order of each sum over rows; bit for bit that call's when n_env is a multiple of 64.
 * A row's out5 / action / obs / cost / g_actions / g_obs0 bits depend on that row and the two handles only, and a call repeats its
 * bits.  A non-finite row poisons its own outputs and, through the row sums, g_params (envbuild_mlp_grad.h).
 * Return codes: n_env == 0 writes zeros to g_params (if given) and nothing else.  EB_EINVAL, nothing written: a NULL handle; a refused
 * pair; n_env < 0; steps outside 1 .. EB_POLICY_ROLLOUT_GRAD_MAX_STEPS or steps * n_pad > 65535 * 2048; NULL obs_in, w5 or
 * workspace; a workspace too small; obs_out == obs_in; training mode without ref_idx; path_id out of range in selecting mode.
 * EB_ESTATE: paths or vehicle modes not set, a policy layer not set. */
int eb_policy_rollout_grad(eb_handle h, eb_mlp policy, int32_t n_env, int32_t steps, const float* obs_in, const int32_t* ref_idx,
                           int32_t path_id, float action_range, const float* w5, void* workspace, size_t workspace_bytes,
                           float* obs_out, float* out5_steps, float* actions_steps, float* obs_steps, float* cost,
                           float* g_actions_steps, float* g_obs0, float* g_params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_POLICY_ROLLOUT_GRAD_H */
