// eb_policy_rollout.h — host-visible launch interface of the closed-loop rollout kernel (eb_policy_rollout.hip), next to eb_cand.h and
// eb_policy_f16.h.  The contract is stated in include/envbuild_policy_rollout.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_policy_f16.h"

namespace eb {

constexpr int PR_MAX_VEH = 32;      // a tile's near-record mask is one 64-bit word per env, its fp32 rows 64 x (9 + 4 * 32) floats of LDS
constexpr int PR_MAX_UNITS = 256;   // padded hidden width: the <2, 4> tiling of 512 units leaves no room for a second block on the CU

// `horizon` steps of [policy(obs) -> rollout_out] for n_env envs in one launch; see include/envbuild_policy_rollout.h:eb_policy_rollout
struct PolicyRolloutArgs {
    const float* obs0;         // [n_env, obs_dim]
    const int* ref_idx;        // training mode: the env's path
    float* obs_out;            // [n_env, obs_dim]: the state after the last step
    float* out5_steps;         // [horizon, 5, n_env] or NULL
    float* actions_steps;      // [horizon, n_env, 2] or NULL
    float* obs_steps;          // [horizon, n_env, obs_dim] or NULL: the state AFTER step t
    float* punish;             // [n_env] or NULL
    uint8_t* safe;             // [n_env] or NULL
    // the closest-point tables of the handle (as TapeCandArgs carries them)
    const PathTables* dt;
    const float* xy10;
    const float* phi10;
    const float* rad_all;
    const uint32_t* cells;
    float gx0, gy0;
    int gnx, gny;
    int red_off[3], red_len[3], n_paths;
    int n_env, obs_dim, nd, n_veh, horizon;
    int training, path_id;
    int penalty_row;           // row of out5 that punish accumulates: 3 (veh2veh4real) or 2 (real_punish_term), DAM:126
    unsigned nv_magic;         // div_magic(n_veh)
    // the policy (as MlpF16Args carries it; the head is eb_policy_run_batch's)
    const float* scale;        // obs_scale or NULL
    int n_hidden, units, n_units, hidden_act, out_act;
    float action_range;
    int row_stride;            // LDS halves per activation row (mlp_f16_row_stride)
    MlpF16Layer hid[MLP_MAX_HIDDEN];
    MlpF16Layer outl;
};
// dynamic LDS of a block: the tile's fp32 rows, then the binary16 activations and the model step's near-record scratch in one region
size_t policy_rollout_lds_bytes(int obs_dim, int n_veh, int row_stride);
hipError_t launch_policy_rollout(int task, const PolicyRolloutArgs& A, hipStream_t s);

}  // namespace eb
