// eb_policy_head_device.h — what a fused epilogue kernel of the policy does before its row function, as one function: mlp_kernel
// (eb_policy.hip) up to the activated logits, then the hand-off of the block's 64 x out_dim logits through LDS to one lane per row.
// policy_logp_kernel (eb_policy_logp.hip) calls it.  policy_sample_kernel (eb_policy_sample.hip) holds the same text in its body and
// keeps it: calling this function from there changes that kernel's register allocation and instruction schedule, and its machine code
// is pinned.
//
// In the output tile a lane holds D[4 (l >> 4) + v][l & 15]: a row's mean[a] and ls[a] sit in different lanes (for act_dim = 16 in
// different column tiles), so an epilogue that works on a whole row crosses lanes.  It does so through LDS: once every wave has left the
// output chain (a __syncthreads) the activation buffer is free, the logits go there with a row stride of LS = 33 floats (lane r reads
// r * 33 + a: every bank once), and after a second __syncthreads lanes 0..15 of each wave take the wave's own 16 rows, so the four SIMDs
// share the work.  No LDS beyond mlp_kernel's (64 * 33 floats <= 64 * (64 + 4)), no atomics, plain vector stores.
#pragma once
#include "eb_mlp_device.h"

namespace eb {
namespace phead {

constexpr int LS = 33;        // row stride of the logits in LDS

// Stages the block's observations, runs the hidden chain and the 16 x 16 x 4 output chain (eb_mlp_forward's bits), writes the activated
// logits to lds[row * LS + col] and, when A.out is given, to A.out.  Ends after the __syncthreads that publishes the LDS rows.  wave / lane:
// this thread's; row0: the block's first row; rows_here: how many of its 64 rows exist.  Every thread of the block must call it.
template <int RT, int CT>
EB_DEV void logits_to_lds(const MlpArgs& A, float* lds, const int wave, const int lane, const int row0, const int rows_here) {
    const int i = lane & 31, h = lane >> 5;
    const int RS = A.row_stride, HS = (RS - 4) >> 1;
    const int D = A.obs_dim, K0 = A.hid[0].k_pad;

    // ---- stage the (preprocessed) observations: mlp_kernel's ----
    {
        constexpr int RPW = MLP_ROWS / 4, KC = 3;
        const int rbase = wave * RPW;
        for (int k0 = lane; k0 < K0; k0 += 64 * KC) {
            float v[KC][RPW], sc[KC];
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int k = k0 + 64 * c, kc = k < D ? k : D - 1;
                sc[c] = A.scale ? A.scale[kc] : 1.0f;                     // x * 1.0f is x, bit for bit
#pragma unroll
                for (int rr = 0; rr < RPW; ++rr) {
                    const int r = rbase + rr;
                    const int rc = r < rows_here ? r : rows_here - 1;
                    v[c][rr] = A.obs[(size_t)(row0 + rc) * D + kc];
                }
            }
#pragma unroll
            for (int c = 0; c < KC; ++c) {
                const int k = k0 + 64 * c;
                if (k < K0) {
                    float* dst = lds + rbase * RS + (k & 1) * HS + (k >> 1);
#pragma unroll
                    for (int rr = 0; rr < RPW; ++rr)
                        dst[rr * RS] = (rbase + rr < rows_here && k < D) ? v[c][rr] * sc[c] : 0.0f;   // preprocessor.py:121
                }
            }
        }
    }
    __syncthreads();

    // ---- hidden layers: mlp_kernel's ----
    const int rt0 = RT == 2 ? 0 : (wave & 1);
    const int ct0 = RT == 2 ? wave * CT : (wave >> 1);
    for (int L = 0; L < A.n_hidden; ++L) {
        const MlpLayer& ly = A.hid[L];
        mlp::f32x16 acc[RT][CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const float b = ly.b[(ct0 + c) * 32 + i];
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[r][c][v] = b;
        }
        mlp::layer_chain<RT, CT>(lds + (rt0 * 32 + i) * RS + h * HS, 32 * RS, reinterpret_cast<const mlp::f32x4*>(ly.w),
                                 ly.k_pad >> 3, ct0, lane, acc);
        __syncthreads();                                              // every wave has read this layer's inputs
        switch (A.hidden_act) {
            case MLP_ACT_RELU: mlp::store_hidden<RT, CT, MLP_ACT_RELU>(lds, RS, HS, rt0, ct0, i, h, acc); break;
            case MLP_ACT_ELU: mlp::store_hidden<RT, CT, MLP_ACT_ELU>(lds, RS, HS, rt0, ct0, i, h, acc); break;
            case MLP_ACT_TANH: mlp::store_hidden<RT, CT, MLP_ACT_TANH>(lds, RS, HS, rt0, ct0, i, h, acc); break;
            default: mlp::store_hidden<RT, CT, MLP_ACT_LINEAR>(lds, RS, HS, rt0, ct0, i, h, acc); break;
        }
        __syncthreads();
    }

    // ---- output layer: mlp_kernel's 16 x 16 x 4 chain (row tile = wave, ceil(out_dim / 16) <= 2 column tiles); the activated
    //      outputs of both tiles stay in registers until every wave has finished reading the activations ----
    const int i16 = lane & 15, kq = lane >> 4, hsel = kq >> 1;
    const int ct16 = (A.out_dim + 15) >> 4;
    float yv[2][4];
    {
        const int steps4 = A.outl.k_pad >> 4;                               // groups of four MFMAs (16 inputs)
        const float* a_ptr = lds + (wave * 16 + i16) * RS + (kq & 1) * HS;  // element (k >> 1) = m of this lane's parity at a_ptr[m]
        const mlp::f32x4* w16 = reinterpret_cast<const mlp::f32x4*>(A.outl.w);
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            if (ct < ct16) {
                const float b = A.outl.b[ct * 16 + i16];
                mlp::f32x4 acc = {b, b, b, b};
                const mlp::f32x4* wsrc = w16 + (size_t)ct * steps4 * 64 + lane;
                mlp::f32x4 bq = wsrc[0];
                for (int s4 = 0; s4 < steps4; ++s4) {
                    const mlp::f32x4 bn = wsrc[(size_t)(s4 + 1 < steps4 ? s4 + 1 : s4) * 64];      // the next group's weights under these MFMAs
                    const mlp::f32x4 a01 = *reinterpret_cast<const mlp::f32x4*>(a_ptr + 8 * s4);
                    const mlp::f32x4 a23 = *reinterpret_cast<const mlp::f32x4*>(a_ptr + 8 * s4 + 4);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a01[1] : a01[0], bq[0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a01[3] : a01[2], bq[1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a23[1] : a23[0], bq[2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a23[3] : a23[2], bq[3], acc, 0, 0, 0);
                    bq = bn;
                }
#pragma unroll
                for (int v = 0; v < 4; ++v) yv[ct][v] = mlp::activate_rt(A.out_act, acc[v]);
            }
        }
    }
    __syncthreads();                                                  // the activation buffer is free

    // ---- the activated logits: to LDS for the row lanes, and to A.out from the lanes that hold them ----
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int col = ct * 16 + i16;
        if (ct < ct16 && col < A.out_dim) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = wave * 16 + 4 * kq + v;
                lds[row * LS + col] = yv[ct][v];
                if (A.out && row < rows_here) A.out[(size_t)(row0 + row) * A.out_dim + col] = yv[ct][v];
            }
        }
    }
    __syncthreads();
}

}  // namespace phead
}  // namespace eb
