// eb_policy_f16.h — host-visible launch interface of the fp16 policy kernel (eb_policy_f16.hip), next to eb_kernels.h's fp32 one.
// The arithmetic contract is stated in include/envbuild_mlp_f16.h.
#pragma once
#include "eb_kernels.h"

namespace eb {

struct MlpF16Layer {
    const uint16_t* w;   // packed binary16 weights (pack_weights_f16 / pack_weights16_f16)
    const float* b;      // fp32 bias, zero-padded to the tile width (the fp32 kernel's buffer)
    int k_pad;           // inputs, padded to a multiple of 16
    int pad_;
};
struct MlpF16Args {
    const float* obs;
    const float* scale;   // obs_scale or NULL
    float* out;           // logits [n, out_dim] or actions [n, out_dim / 2]
    int n, obs_dim, n_hidden;
    int units;            // padded hidden width: 64 / 128 / 256 / 512
    int n_units;          // hidden width as configured: units at and beyond it are held at zero
    int out_dim, hidden_act, out_act, head;
    float action_range;
    int row_stride;       // LDS halves per row: max(k_pad of layer 0, units) + 8
    MlpF16Layer hid[MLP_MAX_HIDDEN];
    MlpF16Layer outl;
};
inline int mlp_f16_k_pad0(int obs_dim) { return (obs_dim + 15) / 16 * 16; }
inline int mlp_f16_row_stride(int obs_dim, int units) { return (mlp_f16_k_pad0(obs_dim) > units ? mlp_f16_k_pad0(obs_dim) : units) + 8; }
uint16_t f16_bits(float x);   // IEEE round-to-nearest-even to binary16, overflow to +-inf
void pack_weights_f16(const float* kernel, int k_real, int cols_real, int k_pad, int col_tiles, uint16_t* out);
void pack_weights16_f16(const float* kernel, int k_real, int cols_real, int k_pad, uint16_t* out);   // the output layer's 16-column tiles
hipError_t launch_mlp_f16(const MlpF16Args& A, hipStream_t s);

}  // namespace eb
