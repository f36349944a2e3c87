// eb_policy_rollout_grad.h — host-visible launch interface of the closed-loop rollout with its parameter gradient
// (eb_policy_rollout_grad.hip), next to eb_policy_rollout.h and eb_policy_grad.h.  The contract is stated in
// include/envbuild_policy_rollout_grad.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_policy_grad.h"

namespace eb {

constexpr int PRG_MAX_VEH = 32;       // a tile's near-record mask is one 64-bit word per env
constexpr int PRG_MAX_STEPS = 128;    // the cap on `steps` the entry states
constexpr int PRG_TAPE_FLOATS = 16;   // per (step, env) in the workspace: grad::TapeStep's 12, the raw action (2), the output layer's means (2)
// rows (steps * n_pad) mlp_wgrad_kernel takes in one launch: its row index is an int, its grid's y a 16-bit count of four 512-row splits
constexpr long long PRG_MAX_ROWS = 65535ll * 4 * MLP_GRAD_SPLIT_ROWS;

// `horizon` steps of [policy(obs) -> rollout_out] for n_env envs and the reverse sweep through both, in one launch
struct PolicyRolloutGradArgs {
    const float* obs0;         // [n_env, obs_dim]
    const int* ref_idx;        // training mode: the env's path
    float* obs_out;            // [n_env, obs_dim] or NULL: the state after the last step
    float* out5_steps;         // [horizon, 5, n_env] or NULL
    float* actions_steps;      // [horizon, n_env, 2] or NULL
    float* obs_steps;          // [horizon, n_env, obs_dim] or NULL: the state AFTER step t
    float* cost;               // [n_env] or NULL
    float* g_actions_steps;    // [horizon, n_env, 2] or NULL
    float* g_obs0;             // [n_env, 9] or NULL
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
    unsigned nv_magic;         // div_magic(n_veh)
    int n_pad;                 // n_env rounded up to 64: rows per step in the workspace
    float w5[5];               // the weights of cost = the cotangent of every step's out5
    // the policy (as MlpGradArgs carries it; the head is eb_policy_run_batch's)
    const float* scale;        // obs_scale or NULL
    int n_hidden, units, hidden_act, out_act;
    float action_range;
    int row_stride;            // LDS floats per activation row (max(k_pad0, units) + 4)
    int kt_out;                // padded inputs of the output layer's transposed product
    MlpLayer hid[MLP_MAX_HIDDEN];
    MlpLayer outl;
    const float* wt[MLP_GRAD_LAYERS];
    // the workspace: mlp_grad_layout's arrays for horizon * n_pad rows, row (t, env) at t * n_pad + env; then the tape
    float* ws;
    long long x_off[MLP_GRAD_LAYERS];
    long long d_off[MLP_GRAD_LAYERS];
    long long tape_off;        // [horizon][PRG_TAPE_FLOATS][n_pad]
};
// dynamic LDS of a block: the tile's fp32 rows, then the fp32 activations / cotangents and the model step's near-record scratch in one region
size_t policy_rollout_grad_lds_bytes(int obs_dim, int n_veh, int row_stride);
size_t policy_rollout_grad_lds_limit();   // what one block may ask for on gfx950
hipError_t launch_policy_rollout_grad(int task, const PolicyRolloutGradArgs& A, hipStream_t s);

}  // namespace eb
