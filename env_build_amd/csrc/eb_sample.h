// eb_sample.h — host-visible launch interface of the sampled-tape kernel (eb_rollout_tape_sample.hip), next to eb_cand.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_kernels.h"

namespace eb {

constexpr int TS_MAX_SAMPLES = 4096;   // samples per env and launch at most: their costs stay in the block's LDS (16 KB)
constexpr int TS_MAX_HORIZON = 128;

// draw, roll out, score and average n_samples tapes per env in one launch; see include/envbuild_sample.h:eb_rollout_tape_sample
struct TapeSampleArgs {
    const float* obs0;         // [n_env, obs_dim], shared by the samples
    const float* nominal;      // [horizon, n_env, 2] raw
    const int* ref_idx;        // training mode: [n_env]; NULL in selecting mode
    const int* env_ids;        // [n_env] or NULL
    uint64_t seed, counter;
    float sigma0, sigma1, beta, gain, inv_lambda;
    float w5[5];
    float* cost;               // [n_samples, n_env] or NULL
    float* best_tape;          // [horizon, n_env, 2] or NULL
    float* best_cost;          // [n_env] or NULL
    int* best_index;           // [n_env] or NULL
    float* mean_tape;          // [horizon, n_env, 2] or NULL
    float* samples_out;        // [n_samples, horizon, n_env, 2] or NULL
    // the closest-point tables of the handle (as TapeCandArgs carries them)
    const PathTables* dt;
    const float* xy10;
    const float* phi10;
    const float* rad_all;
    const uint32_t* cells;
    float gx0, gy0;
    int gnx, gny;
    int red_off[3], red_len[3], n_paths;
    int n_env, n_samples, obs_dim, nd, n_veh, horizon;
    int training, path_id;
    int envs_per_block;        // 4, 2 or 1: set by the launcher
};
hipError_t launch_rollout_tape_sample(int task, const TapeSampleArgs& A, hipStream_t s);

}  // namespace eb
