// eb_policy_rollout_sample.h — host-visible launch interface of the closed-loop rollout under the STOCHASTIC head with its
// reparameterised gradient (eb_policy_rollout_sample.hip), next to eb_policy_rollout_grad.h and eb_policy_sample.h.  The contract is
// stated in include/envbuild_policy_rollout_sample.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_policy_rollout_grad.h"

namespace eb {

// per (step, env) in the workspace: grad::TapeStep's 12, the raw action (2), then what the sampling head's reverse needs: the two
// activated means (14, 15), the two activated log-stds (16, 17), the two eps (18, 19)
constexpr int PRS_TAPE_FLOATS = 20;
constexpr int PRS_LS = 33;            // row stride of the 64 x 4 activated logits in LDS (eb_policy_sample.hip's)

// `horizon` steps of [policy_sample(obs) -> rollout_out] for n_env envs and, on request, the reverse sweep through the model step, the
// sampling head and the policy, in one launch.  The scene, the policy and the workspace are PolicyRolloutGradArgs' fields (its
// action_range is eb_policy_sample's here; its tape is [horizon][PRS_TAPE_FLOATS][n_pad]).
struct PolicyRolloutSampleArgs : PolicyRolloutGradArgs {
    const int* row_ids;        // [n_env] or NULL: the env index names the row's draw
    const float* eps_steps;    // [horizon, n_env, 2] or NULL: draw the noise
    float* logp_steps;         // [horizon, n_env] or NULL
    float* eps_out_steps;      // [horizon, n_env, 2] or NULL
    unsigned long long seed, counter;   // step t draws with (seed, counter + t)
    float log_ar;              // log(action_range) when it is > 0
    float w_logp;              // the cotangent of every step's logp
    int with_grad;             // 0: forward only, the workspace is never touched
};
size_t policy_rollout_sample_lds_bytes(int obs_dim, int n_veh, int row_stride);
size_t policy_rollout_sample_lds_limit();   // what one block may ask for on gfx950
hipError_t launch_policy_rollout_sample(int task, const PolicyRolloutSampleArgs& A, hipStream_t s);

}  // namespace eb
