// eb_cand.h — host-visible launch interface of the candidate-tape kernel (eb_rollout_tape_cand.hip), next to eb_grad.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_kernels.h"

namespace eb {

constexpr int TC_MAX_CAND = 8;     // candidates per launch at most: a block's env role is one wave of (env, candidate) lanes
constexpr int TC_MAX_HORIZON = 128;

// value-only open-loop rollout of n_cand tapes per env in one launch; see include/envbuild_cand.h:eb_rollout_tape_cand
struct TapeCandArgs {
    const float* obs0;         // [n_env, obs_dim], shared by the candidates
    const float* tapes;        // [n_cand, horizon, n_env, 2] raw
    const int* ref_idx;        // training mode: candidate k reads ref_idx[k * ref_ld + env]
    float w5[5];
    float* out5_steps;         // [n_cand, horizon, 5, n_env] or NULL
    float* cost;               // [n_cand, n_env] or NULL
    // the closest-point tables of the handle (as TapeVjpArgs carries them)
    const PathTables* dt;
    const float* xy10;
    const float* phi10;
    const float* rad_all;
    const uint32_t* cells;
    float gx0, gy0;
    int gnx, gny;
    int red_off[3], red_len[3], n_paths;
    int n_env, n_cand, obs_dim, nd, n_veh, horizon;
    int ref_ld, training, retrack;
    unsigned path_bits;        // selecting mode: candidate k's path in bits 2k, 2k + 1
    int envs_per_tile;         // set by the launcher
};
// the most candidates a launch takes for this slot count (its (env, candidate, slot) queue must fit the LDS)
int rollout_tape_cand_max(int n_veh);
// n_cu: compute units of the device (the tile is chosen so that a grid fills them)
hipError_t launch_rollout_tape_cand(int task, const TapeCandArgs& A, int n_cu, hipStream_t s);

}  // namespace eb
