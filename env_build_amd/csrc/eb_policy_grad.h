// eb_policy_grad.h — host-visible launch interface of the policy network's backward (eb_policy_grad.hip), next to eb_kernels.h's
// forward one.  The arithmetic contract is stated in include/envbuild_mlp_grad.h.
#pragma once
#include "eb_kernels.h"

namespace eb {

constexpr int MLP_GRAD_MAX_UNITS = 256;    // padded hidden width the backward kernels are instantiated for
constexpr int MLP_GRAD_SPLIT_ROWS = 512;   // rows of the batch one wave of mlp_wgrad_kernel reduces: one partial tile per 512 rows
constexpr int MLP_GRAD_LAYERS = MLP_MAX_HIDDEN + 1;

// the packings of one layer and where its parameters sit in the flat buffer (Model.get_weights() order: kernel [k_real, cols_real]
// row-major, then the bias)
struct MlpPackLayer {
    float* w;          // pack_weights (hidden) / pack_weights16 (output): k_pad x col_tiles * 32 floats
    float* b;          // col_tiles * 32 floats
    uint16_t* w16;     // pack_weights_f16 / pack_weights16_f16: k_pad16 x (units | 32) halves
    float* wt;         // pack_weights of the TRANSPOSED kernel: kt_pad x colt_tiles * 32 floats
    int k_real, cols_real;
    int k_pad, col_tiles;      // of w
    int k_pad16;               // of w16
    int kt_pad, colt_tiles;    // of wt: inputs = this layer's columns (padded), columns = this layer's inputs in tiles of 32
    int is_out;
    long long w_off, b_off;    // floats from the start of the flat buffer
};
struct MlpPackArgs {
    const float* params;
    int n_layers, units;
    MlpPackLayer layer[MLP_GRAD_LAYERS];
};
hipError_t launch_mlp_pack(const MlpPackArgs& A, hipStream_t s);

// one product of mlp_wgrad_kernel: dW[k, u] = sum over rows of x[r, k] * d[r, u], db[u] = sum over rows of d[r, u]
struct MlpWgradLayer {
    const float* x;    // [n_pad, x_stride]: the layer's inputs
    const float* d;    // [n_pad, d_stride]: the cotangent of its pre-activations
    int x_stride, d_stride;
    int k_real, u_real;
    int kb, ub;        // blocks of 64 inputs / 64 columns
    int task0;         // index of this layer's first (k block, u block) pair in the grid
    int pad_;
    long long part_off;      // floats from the start of one split's partials: [(kb * 64 + 1), ub * 64], the last row is the bias
    long long w_off, b_off;  // floats from the start of g_params
};
struct MlpGradArgs {
    MlpArgs fwd;               // obs, scale, out (may be NULL), n, dims, head, action_range, row_stride, packed weights and biases
    const float* g_out;        // [n, out_dim] (head 0) or [n, out_dim / 2] (head 1)
    float* g_obs;              // [n, obs_dim] or NULL
    float* g_params;           // flat, unpadded, or NULL
    const float* wt[MLP_GRAD_LAYERS];   // the transposed packings; [n_hidden] is the output layer's
    int kt_out;                // padded inputs of the output layer's transposed product: out_dim rounded up to 8
    int n_units;               // hidden width as configured
    // the workspace, in floats from its start (n_pad = n rounded up to 64 rows)
    float* ws;
    long long x_off[MLP_GRAD_LAYERS];   // x_0 [n_pad, k_pad0], x_1 .. x_H [n_pad, units]
    long long d_off[MLP_GRAD_LAYERS];   // d_0 .. d_{H-1} [n_pad, units] (cotangents of the hidden pre-activations), d_H [n_pad, 32]
    long long part_off;                 // the partial tiles: [splits][part_stride]
    long long part_stride;
    long long param_count;
    int n_tasks;
    MlpWgradLayer wl[MLP_GRAD_LAYERS];
};
// what every caller of the two entries below lays out first: fills x_off .. n_tasks, wl[] (but for the pointers) and returns the
// workspace size in bytes for A.fwd.n rows
size_t mlp_grad_layout(MlpGradArgs& A);
hipError_t launch_mlp_backward(const MlpGradArgs& A, hipStream_t s);
// mlp_wgrad_kernel + mlp_wgrad_reduce_kernel without the data pass: the workspace was filled by another kernel
hipError_t launch_mlp_wgrad(const MlpGradArgs& A, hipStream_t s);

}  // namespace eb
