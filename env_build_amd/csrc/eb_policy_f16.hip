// eb_policy_f16.hip — the policy network with binary16 operands on the matrix cores (include/envbuild_mlp_f16.h), gfx950 only.
//
// The same network, block shape and launch as eb_policy.hip (one block = 64 observations x 4 waves, the whole MLP in one launch, the
// current layer's activations in LDS, the weights streaming from L2), with the operand type changed:
//
//   * hidden layers run on v_mfma_f32_32x32x16_f16 (16 inputs per instruction in half the cycles of the fp32 kernel's 2), the output
//     layer (<= 32 columns) on v_mfma_f32_16x16x32_f16, one row tile of 16 per wave.  Products of binary16 operands are exact in fp32
//     and the accumulator is fp32; the order of the sum is the instruction's and this k-loop's.
//   * the activations sit in LDS as binary16, row i at i * RS halves, RS = K + 8: a row is K / 8 + 1 sixteen-byte slots, an odd
//     number for every K that is a multiple of 16, so the 16 rows of a ds_read_b128 lane group fall on 16 different slots.
//   * a hidden layer is computed TRANSPOSED: the weights are the A operand (row = output unit), the activations the B operand
//     (column = observation).  Lane l holds A[unit l & 31][k = 8 (l >> 5) + j] and B[k = 8 (l >> 5) + j][observation l & 31], j = 0..7,
//     so the activation fragment is one ds_read_b128 of row-major LDS and the weight fragment one global_load_dwordx4 of the host's
//     packing (pack_weights_f16); the result D[unit (v & 3) + 8 (v >> 2) + 4 (l >> 5)][observation l & 31] puts FOUR consecutive units
//     of one observation in a lane's registers 4g .. 4g+3: the epilogue packs them and writes 8 bytes, where the untransposed product
//     would write 2.
//   * the bias is the accumulator's initial value; the epilogue applies the activation in fp32 (eb_mlp_device.h's, the one
//     eb_policy.hip applies), converts with round-to-nearest-even (v_cvt_f16_f32 under the default mode) and writes back once every
//     wave has read its inputs.
//   * widths are padded with zero weights / zero bias to the next supported U, k to 16.  A padded unit is WRITTEN as zero whatever
//     its accumulator holds (an inf or NaN input times a zero weight is NaN), so a row's non-finite pattern is that of the unpadded
//     network.
#include "eb_policy_f16_device.h"

#include <cstring>

namespace eb {

// LDS layout of the activations: element (row i, input k) at i * RS + k halves; RS = Kmax + 8.
template <int RT, int CT>
__global__ __launch_bounds__(MLP_THREADS, CT == 4 ? 1 : 2) void mlp_f16_kernel(const MlpF16Args A) {   // waves per SIMD
    extern __shared__ __attribute__((aligned(16))) _Float16 lds16[];
    _Float16* lds = lds16;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int RS = A.row_stride;
    const int row0 = blockIdx.x * MLP_ROWS;
    const int rows_here = A.n - row0 < MLP_ROWS ? A.n - row0 : MLP_ROWS;
    const int D = A.obs_dim, K0 = A.hid[0].k_pad;

    // ---- stage the (preprocessed) observations as binary16: a wave takes 16 rows, lanes stride over a row (coalesced); the loads
    //      of three column chunks x 16 rows are in flight together; zero beyond n and obs_dim ----
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
                    _Float16* dst = lds + rbase * RS + k;
#pragma unroll
                    for (int rr = 0; rr < RPW; ++rr) {
                        float x = v[c][rr] * sc[c];                       // one fp32 multiply (preprocessor.py:121), THEN one conversion:
                        asm("" : "+v"(x));                               // not the fused v_fma_mixlo_f16 the compiler would make of the two
                        dst[rr * RS] = (_Float16)((rbase + rr < rows_here && k < D) ? x : 0.0f);
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- hidden layers ----
    const int rt0 = RT == 2 ? 0 : (wave & 1);
    const int ct0 = RT == 2 ? wave * CT : (wave >> 1);
    for (int L = 0; L < A.n_hidden; ++L) {
        const MlpF16Layer& ly = A.hid[L];
        mlp::f32x16 acc[RT][CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const mlp::f32x4* bsrc = reinterpret_cast<const mlp::f32x4*>(ly.b + (ct0 + c) * 32 + 4 * h);   // units 8 g + 4 h + e
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const mlp::f32x4 b = bsrc[2 * g];
#pragma unroll
                for (int r = 0; r < RT; ++r)
#pragma unroll
                    for (int e = 0; e < 4; ++e) acc[r][c][4 * g + e] = b[e];
            }
        }
        layer_chain_f16<RT, CT>(lds + (rt0 * 32 + i) * RS + 8 * h, 32 * RS, reinterpret_cast<const f16x8*>(ly.w), ly.k_pad >> 4, ct0,
                                lane, acc);
        __syncthreads();                                              // every wave has read this layer's inputs
        switch (A.hidden_act) {
            case MLP_ACT_RELU: store_hidden_f16<RT, CT, MLP_ACT_RELU>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
            case MLP_ACT_ELU: store_hidden_f16<RT, CT, MLP_ACT_ELU>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
            case MLP_ACT_TANH: store_hidden_f16<RT, CT, MLP_ACT_TANH>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
            default: store_hidden_f16<RT, CT, MLP_ACT_LINEAR>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
        }
        __syncthreads();
    }

    // ---- output layer: 16 x 16 x 32 tiles, row tile = wave, ceil(out_dim / 16) column tiles.  Lane l supplies
    // A[observation l & 15][k = 32 s + 8 (l >> 4) + j] and B[k = 32 s + 8 (l >> 4) + j][column l & 15], j = 0..7; it receives
    // D[4 (l >> 4) + v][l & 15], v = 0..3.
    {
        const int i16 = lane & 15, kq = lane >> 4;
        const int steps = A.outl.k_pad >> 5;
        const _Float16* a_ptr = lds + (wave * 16 + i16) * RS + 8 * kq;
        const f16x8* w16 = reinterpret_cast<const f16x8*>(A.outl.w);
        const int ct16 = (A.out_dim + 15) >> 4;
        for (int ct = 0; ct < ct16; ++ct) {
            const float b = A.outl.b[ct * 16 + i16];
            mlp::f32x4 acc = {b, b, b, b};
            const f16x8* wsrc = w16 + (size_t)ct * steps * 64 + lane;
            f16x8 bq = wsrc[0];
            for (int s = 0; s < steps; ++s) {
                const f16x8 bn = wsrc[(size_t)(s + 1 < steps ? s + 1 : s) * 64];             // the next step's weights under this MFMA
                const f16x8 aq = *reinterpret_cast<const f16x8*>(a_ptr + 32 * s);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq, bq, acc, 0, 0, 0);
                bq = bn;
            }
            const int col = ct * 16 + i16;
            if (A.head == MLP_HEAD_LOGITS) {
                if (col < A.out_dim) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int row = wave * 16 + 4 * kq + v;
                        if (row < rows_here) A.out[(size_t)(row0 + row) * A.out_dim + col] = mlp::activate_rt(A.out_act, acc[v]);
                    }
                }
            } else {   // deterministic action: action_range * tanh(mean), utils/policy.py:89-92
                const int act_dim = A.out_dim >> 1;
                if (col < act_dim) {
#pragma unroll
                    for (int v = 0; v < 4; ++v) {
                        const int row = wave * 16 + 4 * kq + v;
                        const float mean = mlp::activate_rt(A.out_act, acc[v]);
                        if (row < rows_here)
                            A.out[(size_t)(row0 + row) * act_dim + col] = A.action_range > 0.0f ? A.action_range * mlp::tanh_det(mean) : mean;
                    }
                }
            }
        }
    }
}

hipError_t launch_mlp_f16(const MlpF16Args& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const dim3 g((A.n + MLP_ROWS - 1) / MLP_ROWS), b(MLP_THREADS);
    const size_t lds = (size_t)MLP_ROWS * A.row_stride * sizeof(uint16_t);
    const int dev = current_device_index();
    const hipError_t e = A.units == 64 ? launch_lds<&mlp_f16_kernel<1, 1>>(g, b, lds, dev, s, A)
                         : A.units == 128 ? launch_lds<&mlp_f16_kernel<2, 1>>(g, b, lds, dev, s, A)
                         : A.units == 256 ? launch_lds<&mlp_f16_kernel<2, 2>>(g, b, lds, dev, s, A)
                                          : launch_lds<&mlp_f16_kernel<2, 4>>(g, b, lds, dev, s, A);
    return e != hipSuccess ? e : hipGetLastError();
}

// IEEE binary32 -> binary16, round to nearest even, overflow to +-inf, subnormal results kept, NaN stays NaN (quiet) — numpy's
// astype(float16) and the device's v_cvt_f16_f32 under the default mode.
uint16_t f16_bits(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u > 0x7f800000u) return (uint16_t)(sign | 0x7e00u | ((u >> 13) & 0x3ffu));
    if (u >= 0x477ff000u) return (uint16_t)(sign | 0x7c00u);               // 65520 and beyond (inf included) round to inf
    if (u >= 0x38800000u) {                                                // normal result: drop 13 bits of the significand
        const uint32_t v = u - 0x38000000u;
        return (uint16_t)(sign | ((v + 0xfffu + ((v >> 13) & 1u)) >> 13));
    }
    if (u < 0x33000000u) return (uint16_t)sign;                            // below 2^-25: zero
    const int shift = 126 - (int)(u >> 23);                                // subnormal result, in units of 2^-24: 14 .. 24
    const uint32_t m = (u & 0x7fffffu) | 0x800000u;
    const uint32_t q = m >> shift, rest = m & ((1u << shift) - 1u), half = 1u << (shift - 1);
    return (uint16_t)(sign | (q + ((rest > half || (rest == half && (q & 1u))) ? 1u : 0u)));
}

// Host side of eb_mlp_set_layer, hidden layers: Keras kernel [k_real, cols_real] row-major -> per 32-unit tile, per step of 16 inputs,
// per lane, the 8 halves that lane feeds to one MFMA as its A fragment: W16[16 s + 8 (lane >> 5) + j][tile * 32 + (lane & 31)].
void pack_weights_f16(const float* kernel, int k_real, int cols_real, int k_pad, int col_tiles, uint16_t* out) {
    const int steps = k_pad / 16;
    for (int ct = 0; ct < col_tiles; ++ct)
        for (int s = 0; s < steps; ++s)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 16 * s + 8 * (l >> 5) + j, u = ct * 32 + (l & 31);
                    out[(((size_t)ct * steps + s) * 64 + l) * 8 + j] = (k < k_real && u < cols_real) ? f16_bits(kernel[(size_t)k * cols_real + u]) : 0;
                }
}

// Output layer (16 x 16 x 32 tiles): per 16-column tile, per step of 32 inputs, per lane, the 8 halves of its B fragment:
// W16[32 s + 8 (lane >> 4) + j][tile * 16 + (lane & 15)].
void pack_weights16_f16(const float* kernel, int k_real, int cols_real, int k_pad, uint16_t* out) {
    const int steps = k_pad / 32, tiles = (cols_real + 15) / 16;
    for (int ct = 0; ct < tiles; ++ct)
        for (int s = 0; s < steps; ++s)
            for (int l = 0; l < 64; ++l)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * s + 8 * (l >> 4) + j, c = ct * 16 + (l & 15);
                    out[(((size_t)ct * steps + s) * 64 + l) * 8 + j] = (k < k_real && c < cols_real) ? f16_bits(kernel[(size_t)k * cols_real + c]) : 0;
                }
}

}  // namespace eb
