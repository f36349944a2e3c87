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

// value and gradient of an open-loop rollout in one launch (eb_rollout_tape_vjp.hip); see include/envbuild_grad.h:eb_rollout_tape_vjp
struct TapeVjpArgs {
    const float* obs0;         // [n_env, obs_dim]
    const float* tape;         // [horizon, n_env, 2] raw
    const int* ref_idx;        // training mode
    const float* g_obs_final;  // row stride ld_final, or NULL
    const float* g_out5_steps; // [horizon, 5, n_env], or NULL: w5 at every step and env
    float w5[5];
    float* out5_steps;         // [horizon, 5, n_env] or NULL
    float* obs_out;            // [n_env, obs_dim] or NULL
    float* g_obs0;             // [n_env, nd] or NULL
    float* g_action_tape;      // [horizon, n_env, 2] or NULL
    // the closest-point tables of the handle (as FusedArgs carries them)
    const PathTables* dt;
    const float* xy10;
    const float* phi10;
    const float* rad_all;
    const uint32_t* cells;
    float gx0, gy0;
    int gnx, gny;
    int red_off[3], red_len[3], n_paths;
    int n_env, obs_dim, nd, n_veh, n_future, horizon, ld_final;
    int path_id, training;
    int envs_per_tile;         // set by the launcher
};
// the longest horizon a launch can keep in LDS for this slot count
int rollout_tape_vjp_max_horizon(int n_veh);
// n_cu: compute units of the device (the tile is chosen so that a grid fills them)
hipError_t launch_rollout_tape_vjp(int task, const TapeVjpArgs& A, int n_cu, hipStream_t s);

}  // namespace eb
