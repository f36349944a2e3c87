// eb_policy_f16_device.h — the device code the binary16 policy kernels share: eb_policy_f16.hip (one policy evaluation per launch) and
// eb_policy_rollout.hip (the policy inside the closed-loop rollout).  The binary16 vector types, one hidden layer's k-loop
// on v_mfma_f32_32x32x16_f16 and its epilogue — one text, so one order of every sum in both kernels; the fp32 vector types and the
// deterministic activations are eb_mlp_device.h's, the ones the fp32 kernels apply
// (include/envbuild_mlp_f16.h states the arithmetic; the layout notes are at the top of eb_policy_f16.hip).
#pragma once
#include "eb_mlp_device.h"
#include "eb_policy_f16.h"

namespace eb {

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x4 __attribute__((ext_vector_type(4)));

// One layer's k-loop for the RT (observation) x CT (unit) tiles of a wave.  x_row: LDS address of X[row tile rt0][i][8 h]; wp: this
// layer's packed weights; steps = k_pad / 16.  acc enters holding the bias.  The loop moves in groups of four steps (64 inputs: 4 RT CT
// MFMAs of 32 cycles); a group's fragments are fetched into one of two register sets while the other set's MFMAs run.  Fetches past
// the last step re-read it (valid memory, never used).
template <int RT, int CT>
EB_DEV void layer_chain_f16(const _Float16* x_row, int row_tile_stride, const f16x8* __restrict__ wp, int steps, int ct0, int lane,
                            mlp::f32x16 (&acc)[RT][CT]) {
    const f16x8* wsrc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) wsrc[c] = wp + (size_t)(ct0 + c) * steps * 64 + lane;
    f16x8 wq[2][4][CT], xq[2][4][RT];
    auto fetch = [&](int set, int g) {
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int s = 4 * g + q, sc = s < steps ? s : steps - 1;
#pragma unroll
            for (int c = 0; c < CT; ++c) wq[set][q][c] = wsrc[c][(size_t)sc * 64];
#pragma unroll
            for (int r = 0; r < RT; ++r) xq[set][q][r] = *reinterpret_cast<const f16x8*>(x_row + r * row_tile_stride + sc * 16);
        }
    };
    auto run = [&](int set, int nq) {
#pragma unroll
        for (int q = 0; q < 4; ++q)                                                          // k in order
            if (q < nq) {
#pragma unroll
                for (int r = 0; r < RT; ++r)
#pragma unroll
                    for (int c = 0; c < CT; ++c)
                        acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x16_f16(wq[set][q][c], xq[set][q][r], acc[r][c], 0, 0, 0);
            }
    };
    const int full = steps >> 2, rem = steps & 3;
    fetch(0, 0);
    __builtin_amdgcn_sched_barrier(0);
    int g = 0;
    for (; g + 2 <= full; g += 2) {
        fetch(1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        run(0, 4);
        __builtin_amdgcn_sched_barrier(0);
        fetch(0, g + 2);
        __builtin_amdgcn_sched_barrier(0);
        run(1, 4);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (g < full) {                                                                          // set 0 holds group g either way
        fetch(1, g + 1);
        __builtin_amdgcn_sched_barrier(0);
        run(0, 4);
        __builtin_amdgcn_sched_barrier(0);
        if (rem) run(1, rem);
    } else if (rem) {
        run(0, rem);
    }
}

// A layer's outputs back into the LDS activation buffer as binary16, through the activation; units at and beyond n_units are zero.
template <int RT, int CT, int ACT>
EB_DEV void store_hidden_f16(_Float16* lds, int RS, int rt0, int ct0, int i, int h, int n_units, const mlp::f32x16 (&acc)[RT][CT]) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int u0 = (ct0 + c) * 32 + 4 * h;
            _Float16* dst = lds + ((rt0 + r) * 32 + i) * RS + u0;
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                f16x4 p;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float a = mlp::activate<ACT>(acc[r][c][4 * g + e]);
                    p[e] = (_Float16)(u0 + 8 * g + e < n_units ? a : 0.0f);                  // round to nearest even, overflow to inf
                }
                *reinterpret_cast<f16x4*>(dst + 8 * g) = p;
            }
        }
}

}  // namespace eb
