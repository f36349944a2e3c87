// eb_ilqr.h — host-visible launch interface of the iLQR-iteration kernel (eb_rollout_tape_ilqr.hip), next to eb_sample.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_kernels.h"

namespace eb {

constexpr int IL_MAX_ALPHA = 7;      // step lengths per launch: with candidate 0, eight candidates per env
constexpr int IL_MAX_HORIZON = 32;   // 20 floats per env and step stay in the block's LDS for the backward sweep (40 KB at 16 envs)

// one iLQR iteration in one launch; see include/envbuild_ilqr.h:eb_rollout_tape_ilqr
struct TapeIlqrArgs {
    const float* obs0;         // [n_env, obs_dim], shared by the candidates
    const float* u_nom;        // [horizon, n_env, 2] raw
    const float* x_nom;        // [horizon, 6, n_env] or NULL
    const float* gains;        // [horizon, 14, n_env] or NULL
    const int* ref_idx;        // training mode: [n_env]; NULL in selecting mode
    const float* mu;           // [n_env] or NULL
    float alphas[IL_MAX_ALPHA];
    float w5[5];
    float* cost;               // [1 + n_alpha, n_env] or NULL
    int* best_index;           // [n_env] or NULL
    float* best_cost;          // [n_env] or NULL
    float* u_out;              // [horizon, n_env, 2] or NULL
    float* x_out;              // [horizon, 6, n_env] or NULL
    float* gains_out;          // [horizon, 14, n_env] or NULL
    float* dv;                 // [2, n_env] or NULL
    float* cand_out;           // [1 + n_alpha, horizon, n_env, 2] or NULL
    float* lq_out;             // [horizon, 157, n_env] or NULL
    // the closest-point tables of the handle (as TapeSampleArgs carries them)
    const PathTables* dt;
    const float* xy10;
    const float* phi10;
    const float* rad_all;
    const uint32_t* cells;
    float gx0, gy0;
    int gnx, gny;
    int red_off[3], red_len[3], n_paths;
    int n_env, n_alpha, obs_dim, nd, n_veh, horizon;
    int training, path_id;
    int envs_per_block;        // 16, 8 or 4: set by the launcher
};
hipError_t launch_rollout_tape_ilqr(int task, const TapeIlqrArgs& A, hipStream_t s);

}  // namespace eb
