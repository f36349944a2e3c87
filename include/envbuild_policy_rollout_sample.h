/*
 * envbuild_policy_rollout_sample.h — C-ABI of the STOCHASTIC closed-loop rollout with its reparameterised gradient: `steps` steps of
 * [eb_policy_sample -> eb_rollout_step] under an fp32 policy network in ONE launch, and on request the reverse sweep through the model
 * step, the sampling head and the policy with the parameter gradient in the three launches of envbuild_policy_rollout_grad.h, whatever
 * `steps` is (csrc/eb_policy_rollout_sample.hip, then the row reduction of csrc/eb_policy_grad.hip).
 *
 * A header of its own next to envbuild_policy_rollout_grad.h and envbuild_policy_sample.h: these symbols are exported by
 * env_build_amd/lib/libenvbuild_hip.so ONLY, EB_ABI_VERSION and every other family's version are untouched, and a binding looks them
 * up on demand.  Conventions (return codes, eb_last_error, device pointers) are those of envbuild.h.
 *
 * Why the entry exists: maximum-entropy ADP / stochastic value gradients (J = sum of cost + alpha * sum of log pi, differentiated
 * through the sampled actions) and policy-gradient methods that need on-policy model trajectories with their log-probabilities are,
 * through the other headers, per step of the horizon eb_policy_sample + eb_rollout_step on the way forward and eb_rollout_step_vjp +
 * eb_policy_sample_vjp + eb_mlp_backward on the way back, plus one accumulation of every parameter's gradient per step.  Here a block
 * keeps its 64 envs on the compute unit for both sweeps with the sampling head in the loop.
 *
 * The main entry takes ONE struct: it has 27 arguments.  Its stream is therefore a field, not a parameter, and the table of
 * stream-taking prototypes (tests/test_stream_census.py) does not count it: this family's own tests hold it to that table's
 * obligations (a side stream, capture, replay).
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.  n_pad = n_env rounded up to a multiple of 64.
 */
#ifndef ENVBUILD_POLICY_ROLLOUT_SAMPLE_H
#define ENVBUILD_POLICY_ROLLOUT_SAMPLE_H

#include "envbuild.h"
#include "envbuild_mlp_grad.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_POLICY_ROLLOUT_SAMPLE_ABI_VERSION 1
#define EB_POLICY_ROLLOUT_SAMPLE_MAX_STEPS 128

/* The arguments of eb_policy_rollout_sample.  Everything that is not a pointer (w5 and w_logp, seed and counter, action_range, the
 * sizes) is read from the struct AT CALL TIME: under stream capture those values are baked into the graph, the device buffers are
 * read at every replay (envbuild.h's capture bullet).
 *   struct_size      sizeof(eb_policy_rollout_sample_args); anything else is EB_EINVAL;
 *   n_env, steps     steps in 1 .. EB_POLICY_ROLLOUT_SAMPLE_MAX_STEPS;
 *   path_id          selecting mode (DAM:348-353);
 *   action_range     eb_policy_sample's: > 0 squashes (action_range * tanh(x), the log-prob with its Jacobian), otherwise x itself;
 *   w_logp           the weight of every step's logp in the objective of the gradient, and thereby its cotangent;
 *   w5               5 floats HELD IN THE STRUCT: the weights of `cost` AND the cotangent of out5 at every step and env
 *                    (eb_policy_rollout_grad's meaning);
 *   seed, counter    step t draws its noise with (seed, counter + t);
 *   obs_in           [n_env, D]; never written;
 *   ref_idx          training mode (DAM:340-347): [n_env] path of each env; an id out of range keeps zero tracking;
 *   row_ids          [n_env] or NULL (the env index): eb_policy_sample's, so a slice of a batch repeats the batch's draws;
 *   eps_steps        [steps, n_env, 2] or NULL to draw the noise;
 *   workspace        device memory of at least eb_policy_rollout_sample_workspace_bytes; its contents afterwards are unspecified.  A
 *                    forward-only call (g_actions_steps, g_obs0 and g_params all NULL) needs NONE: 0 bytes, NULL, never touched;
 *   obs_out          [n_env, D] or NULL: the state after the last step; must not alias obs_in;
 *   out5_steps       [steps, 5, n_env] or NULL;  actions_steps [steps, n_env, 2] or NULL;  obs_steps [steps, n_env, D] or NULL (the
 *                    state AFTER step t);  cost [n_env] or NULL;
 *   logp_steps       [steps, n_env] or NULL;  eps_out_steps [steps, n_env, 2] or NULL: the noise used;
 *   g_actions_steps  [steps, n_env, 2] or NULL;  g_obs0 [n_env, 9] or NULL;  g_params flat, eb_mlp_param_count floats, or NULL;
 *   stream           the HIP stream of every launch. */
typedef struct eb_policy_rollout_sample_args {
    uint32_t struct_size;
    int32_t n_env, steps, path_id;
    float action_range;
    float w_logp;
    float w5[5];
    uint64_t seed, counter;
    const float* obs_in;
    const int32_t* ref_idx;
    const int32_t* row_ids;
    const float* eps_steps;
    void* workspace;
    size_t workspace_bytes;
    float* obs_out;
    float* out5_steps;
    float* actions_steps;
    float* obs_steps;
    float* cost;
    float* logp_steps;
    float* eps_out_steps;
    float* g_actions_steps;
    float* g_obs0;
    float* g_params;
    void* stream;
} eb_policy_rollout_sample_args;

int eb_policy_rollout_sample_abi_version(void);

/* *ok = 1 when eb_policy_rollout_sample takes this pair of handles, 0 otherwise, with the first unmet condition in eb_last_error.
 * The list is eb_policy_rollout_grad_supported's:
 *   the policy handle has precision EB_MLP_PRECISION_F32 (a binary16 handle is refused by name), hidden width, padded, at most 256,
 *     every layer set;
 *   the policy's obs_dim is the model's D and its out_dim is 4 (mean and log-std of two actions);
 *   the model has n_veh <= 32 and n_future == 0; both handles live on one device;
 *   the block's LDS (the 64 rows and the fp32 activations) fits a compute unit.
 * Returns EB_OK either way; EB_EINVAL: a NULL handle or NULL ok. */
int eb_policy_rollout_sample_supported(eb_handle h, eb_mlp policy, int32_t* ok);

/* Bytes of workspace eb_policy_rollout_sample needs for n_env envs and `steps` steps.  with_grad == 0 (a forward-only call): 0.
 * Otherwise (0 for n_env == 0) eb_mlp_backward's arrays for steps * n_pad rows and 20 floats of tape per row.  EB_EINVAL: NULL
 * handles or bytes, a refused pair, n_env < 0, steps outside 1 .. EB_POLICY_ROLLOUT_SAMPLE_MAX_STEPS, or more rows than one row
 * reduction takes (steps * n_pad > 65535 * 2048). */
int eb_policy_rollout_sample_workspace_bytes(eb_handle h, eb_mlp policy, int32_t n_env, int32_t steps, int32_t with_grad, size_t* bytes);

/* Forward: bit for bit the loop over t = 0 .. steps - 1 of
 *     eb_policy_sample(policy, n_env, obs_t, eps_steps[t] or NULL, row_ids, seed, counter + t, action_range, a_t, logp_t, NULL, eps_t);
 *     eb_rollout_step(h, obs_t, a_t) -> obs_{t+1}, out5_t
 * through the same two handles.  cost is eb_rollout_tape_cand's cost (the expression and order envbuild_cand.h fixes) of this
 * rollout's out5; logp is NOT folded into it.
 * Objective of the gradient: J = sum over envs of cost + w_logp * sum over envs and steps of logp_t, eps held fixed (the
 * reparameterised gradient).
 * g_actions_steps and g_obs0 are bit for bit this loop of single calls, t = steps - 1 .. 0, lambda_steps = 0:
 *     (s_t, g_a_t) = eb_rollout_step_vjp(obs_t, a_t, g_obs_out = lambda_{t+1}, g_out5 = w5 at every env);
 *     g_y_t = eb_policy_sample_vjp(n_env, 4, y_t, eps_t, action_range, g_a_t, g_logp = w_logp in every row), y_t = eb_mlp_forward(obs_t);
 *     p_t = eb_mlp_backward(obs_t, g_out = g_y_t, head 0)'s g_obs;
 *     lambda_t = s_t[:, :9] + p_t[:, :9] (one fp32 add per element; the policy's cotangent of the vehicle columns is dropped);
 * g_params is, by definition, eb_mlp_backward(head 0)'s g_params for the steps * n_env rows (t, env), t-major, with obs = obs_t and
 * g_out = g_y_t, up to the order of each sum over rows; bit for bit that call's when n_env is a multiple of 64.
 * Launches: g_actions_steps, g_obs0 and g_params all NULL: exactly ONE, the reverse sweep is skipped.  With g_params exactly three
 * (the kernel, mlp_wgrad_kernel, mlp_wgrad_reduce_kernel); with only g_actions_steps and / or g_obs0 one.  A pair
 * eb_policy_rollout_sample_supported refuses is EB_EINVAL with the same reason, never another code path.  No atomics; nothing waits
 * on another block.
 * A row's out5 / action / logp / eps / obs / cost / g_actions / g_obs0 bits depend on that row, its row id, (seed, counter) and the
 * two handles only, and a call repeats its bits.  A non-finite row poisons its own outputs and, through the row sums, g_params.
 * Return codes: n_env == 0 writes zeros to g_params (if given) and nothing else.  EB_EINVAL, checked before any device call, nothing
 * written: a NULL handle, policy or args; struct_size wrong; a refused pair; n_env < 0; steps outside
 * 1 .. EB_POLICY_ROLLOUT_SAMPLE_MAX_STEPS or steps * n_pad > 65535 * 2048; action_range or w_logp NaN; NULL obs_in; with a gradient
 * asked for, a NULL workspace or one too small; obs_out == obs_in; training mode without ref_idx; path_id out of range in selecting
 * mode.  EB_ESTATE: paths or vehicle modes not set, a policy layer not set. */
int eb_policy_rollout_sample(eb_handle h, eb_mlp policy, const eb_policy_rollout_sample_args* args);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_POLICY_ROLLOUT_SAMPLE_H */
