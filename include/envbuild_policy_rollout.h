/*
 * envbuild_policy_rollout.h — C-ABI of the closed-loop rollout: `steps` model steps under a policy network, policy and model step
 * fused, in one launch (csrc/eb_policy_rollout.hip).
 *
 * A header of its own next to envbuild.h and envbuild_mlp_f16.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so
 * ONLY (the CPU oracle of envbuild.h has none of them), EB_ABI_VERSION and every other family's version are untouched, and a binding
 * looks them up on demand.  Conventions (return codes, eb_last_error, device pointers, `stream`) are those of envbuild.h.
 *
 * Why the entry exists: the reference's drivers roll the model forward under the policy — the safety shield for 5 steps
 * (hier_decision.py:89-107), multi_ego's look-ahead for 20 (multi_ego.py:187-209).  Through envbuild.h that is two launches per step,
 * eb_policy_run_batch and eb_rollout_step, with the observations written to memory and read back twice in between, and
 * eb_shield_is_safe — the same two launches, enqueued by one call — returns one accumulated penalty and nothing per step.  Here a
 * block keeps its 64 envs' rows on the compute unit for the whole horizon and every step's outputs are there for the asking.
 *
 * The contract in one sentence: every output equals, bit for bit, `steps` x [eb_policy_run_batch -> eb_rollout_step] through the
 * same two handles.
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.
 */
#ifndef ENVBUILD_POLICY_ROLLOUT_H
#define ENVBUILD_POLICY_ROLLOUT_H

#include "envbuild.h"
#include "envbuild_mlp_f16.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_POLICY_ROLLOUT_ABI_VERSION 1

int eb_policy_rollout_abi_version(void);

/* *ok = 1 when eb_policy_rollout takes this pair of handles, 0 otherwise, with the first unmet condition in eb_last_error:
 *   the policy's precision is EB_MLP_PRECISION_F16 (envbuild_mlp_f16.h);
 *   the policy's obs_dim is the model's D and its out_dim is 4 (mean and log-std of two actions);
 *   its hidden width, padded, is at most 256;
 *   the model has n_veh <= 32 and n_future == 0 (the reference's default);
 *   both handles live on one device.
 * The state is fp32 rows (the binary16-state kernels have no closed-loop form).
 * Returns EB_OK either way; EB_EINVAL: a NULL handle or NULL ok. */
int eb_policy_rollout_supported(eb_handle h, eb_mlp policy, int32_t* ok);

/* `steps` >= 1 steps of [actions = eb_policy_run_batch(policy, obs, action_range); obs, out5 = eb_rollout_step(h, obs, actions)] for
 * n_env envs, starting from obs_in.  ALWAYS one launch: a pair of handles eb_policy_rollout_supported refuses is EB_EINVAL with the
 * same reason, never another code path.  No atomics to global memory; nothing waits on another block.
 *   obs_in         [n_env, D]; never written;
 *   ref_idx        training mode (DAM:340-347): [n_env] path of each env; an id out of range keeps zero tracking (DAM:342, 352);
 *   path_id        selecting mode (DAM:348-353);
 *   action_range   eb_policy_run_batch's: > 0 scales tanh(mean), otherwise the mean itself is the action;
 *   penalty        EB_PENALTY_VEH2VEH4REAL or EB_PENALTY_REAL_PUNISH_TERM: the row of out5 that `punish` accumulates;
 *   obs_out        [n_env, D], required: the state after the last step; must not alias obs_in;
 *   out5_steps     [steps, 5, n_env] or NULL: eb_rollout_step's out5 of step t (rewards, punish_term_for_training,
 *                  real_punish_term, veh2veh4real, veh2road4real; DAM:297-300);
 *   actions_steps  [steps, n_env, 2] or NULL: the raw actions the policy gave at step t;
 *   obs_steps      [steps, n_env, D] or NULL: the state AFTER step t (obs_steps[steps - 1] is obs_out);
 *   punish         [n_env] or NULL: step 0's penalty row plus the later ones in ascending t — eb_shield_is_safe's sum;
 *   safe           [n_env] bytes or NULL: !(punish > 0) after the last step — eb_shield_is_safe's flag (hier_decision.py:97).
 * A row's bits depend on that row and the two handles only — not on its position, its neighbours or n_env — and a launch repeats
 * its bits.
 * Return codes: n_env == 0 is a no-op.  EB_EINVAL: a NULL handle; a pair eb_policy_rollout_supported refuses; n_env < 0; steps < 1;
 * NULL obs_in or obs_out; obs_out == obs_in; an unknown penalty; training mode without ref_idx; path_id out of range in selecting
 * mode.  EB_ESTATE: paths or vehicle modes not set, a policy layer not set. */
int eb_policy_rollout(eb_handle h, eb_mlp policy, int32_t n_env, int32_t steps, const float* obs_in, const int32_t* ref_idx,
                      int32_t path_id, float action_range, int32_t penalty, float* obs_out, float* out5_steps,
                      float* actions_steps, float* obs_steps, float* punish, uint8_t* safe, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_POLICY_ROLLOUT_H */
