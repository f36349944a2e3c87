// eb_grad.h — host-visible launch interface of the reverse pass (eb_rollout_vjp.hip), next to eb_kernels.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_kernels.h"

namespace eb {

// reverse of one eb_rollout_step launch at (obs, actions); see include/envbuild_grad.h:eb_rollout_step_vjp
struct VjpArgs {
    const float* obs;          // [n_env, obs_dim] the PRE-step obs
    const float* actions;      // [n_env, 2] raw
    const int* ref_idx;        // training mode
    const float* g_obs_out;    // cotangent of the next obs, row stride ld_out (first nd columns read), or NULL
    const float* g_out5;       // [5, n_env] or NULL
    float* g_obs_in;           // row stride ld_in: nd (compact rows) or obs_dim (vehicle columns zero-filled)
    float* g_actions;          // [n_env, 2]
    int n_env, obs_dim, nd, n_veh, n_future;
    int ld_out, ld_in;
    int path_id, training, n_paths;
    int lg;                    // log2 of the lanes per env (set by the launcher)
};
hipError_t launch_rollout_step_vjp(int task, const VjpArgs& A, hipStream_t s);

}  // namespace eb
