// eb_policy_sample.hip — the stochastic policy head (include/envbuild_policy_sample.h), gfx950: tanh-Gaussian actions and their
// log-probabilities from the fp32 policy network in ONE launch, the same epilogue alone on given logits, and its reverse pass.
//
// policy_sample_kernel<RT, CT> is mlp_kernel (eb_policy.hip) up to the output layer's accumulators: the same staging, the hidden
// layers through mlp::layer_chain / mlp::store_hidden, the same 16 x 16 x 4 output chain — so the logits are eb_mlp_forward's bits.
// In the output tile a lane holds D[4 (l >> 4) + v][l & 15]: a row's mean[a] and ls[a] sit in different lanes (for act_dim = 16 in
// different column tiles) and logp sums over a, so the epilogue crosses lanes.  It does so through LDS: once every wave has left the
// output chain (a __syncthreads) the activation buffer is free, the block's 64 x out_dim activated logits go there with a row stride
// of 33 floats (lane r reads r * 33 + a: every bank once), and after a second __syncthreads one lane per row — lanes 0..15 of each
// wave for the wave's own 16 rows, so the four SIMDs share the work — runs psample::sample_row in ascending a.  No LDS beyond
// mlp_kernel's (64 * 33 floats <= 64 * (64 + 4)), no atomics, plain vector stores.  The noise is a function of (seed, counter, row
// id) and never exists in memory unless eps_out asks for it.
// policy_sample_logits_kernel calls the same sample_row on rows of global memory: eb_policy_sample equals eb_mlp_forward followed by
// eb_policy_sample_from_logits bit for bit because there is one definition of the row.
#include "eb_policy_sample.h"
#include "eb_policy_sample_device.h"

namespace eb {
namespace {

constexpr int PS_LS = 33;        // row stride of the logits in LDS
constexpr int PS_THREADS = 256;  // of the two elementwise kernels

}  // namespace

template <int RT, int CT>
__global__ __launch_bounds__(MLP_THREADS, CT == 4 ? 1 : 2) void policy_sample_kernel(const PolicySampleArgs P) {   // waves per SIMD
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpArgs& A = P.fwd;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int RS = A.row_stride, HS = (RS - 4) >> 1;
    const int row0 = blockIdx.x * MLP_ROWS;
    const int rows_here = A.n - row0 < MLP_ROWS ? A.n - row0 : MLP_ROWS;
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

    // ---- the activated logits: to LDS for the row lanes, and to logits_out from the lanes that hold them ----
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
        const int col = ct * 16 + i16;
        if (ct < ct16 && col < A.out_dim) {
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = wave * 16 + 4 * kq + v;
                lds[row * PS_LS + col] = yv[ct][v];
                if (A.out && row < rows_here) A.out[(size_t)(row0 + row) * A.out_dim + col] = yv[ct][v];
            }
        }
    }
    __syncthreads();

    // ---- the epilogue: one lane per row, lanes 0..15 of each wave take the wave's own rows ----
    const int row = wave * 16 + lane;
    if (lane < 16 && row < rows_here) {
        const PolicySampleHead& S = P.head;
        const size_t e = (size_t)(row0 + row);
        const int act_dim = A.out_dim >> 1;
        const uint64_t key = splitmix64(S.seed + 0x9E3779B97F4A7C15ull * S.counter);
        const uint64_t id = (uint64_t)(uint32_t)(S.row_ids ? S.row_ids[e] : (int32_t)e);
        psample::sample_row(lds + row * PS_LS, act_dim, S.eps ? S.eps + e * act_dim : nullptr, key, id, S.action_range, S.log_ar,
                            S.actions + e * act_dim, S.logp ? S.logp + e : nullptr, S.eps_out ? S.eps_out + e * act_dim : nullptr);
    }
}

hipError_t launch_policy_sample(const PolicySampleArgs& A, hipStream_t s) {
    if (A.fwd.n <= 0) return hipSuccess;
    const dim3 g((A.fwd.n + MLP_ROWS - 1) / MLP_ROWS), b(MLP_THREADS);
    const size_t lds = mlp_lds_bytes(A.fwd);
    const int dev = current_device_index();
    const hipError_t e = A.fwd.units == 64 ? launch_lds<&policy_sample_kernel<1, 1>>(g, b, lds, dev, s, A)
                         : A.fwd.units == 128 ? launch_lds<&policy_sample_kernel<2, 1>>(g, b, lds, dev, s, A)
                         : A.fwd.units == 256 ? launch_lds<&policy_sample_kernel<2, 2>>(g, b, lds, dev, s, A)
                                              : launch_lds<&policy_sample_kernel<2, 4>>(g, b, lds, dev, s, A);
    return e != hipSuccess ? e : hipGetLastError();
}

// ---- the epilogue alone: one lane per row of [n, out_dim] logits in global memory ----
__global__ __launch_bounds__(PS_THREADS) void policy_sample_logits_kernel(const PolicySampleLogitsArgs A) {
    const size_t e = (size_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (e >= (size_t)A.n) return;
    const PolicySampleHead& S = A.head;
    const int act_dim = A.out_dim >> 1;
    const uint64_t key = splitmix64(S.seed + 0x9E3779B97F4A7C15ull * S.counter);
    const uint64_t id = (uint64_t)(uint32_t)(S.row_ids ? S.row_ids[e] : (int32_t)e);
    psample::sample_row(A.logits + e * A.out_dim, act_dim, S.eps ? S.eps + e * act_dim : nullptr, key, id, S.action_range, S.log_ar,
                        S.actions + e * act_dim, S.logp ? S.logp + e : nullptr, S.eps_out ? S.eps_out + e * act_dim : nullptr);
}

hipError_t launch_policy_sample_from_logits(const PolicySampleLogitsArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(policy_sample_logits_kernel, dim3((A.n + PS_THREADS - 1) / PS_THREADS), dim3(PS_THREADS), 0, s, A);
    return hipGetLastError();
}

// ---- the reverse pass: one lane per (row, a) ----
__global__ __launch_bounds__(PS_THREADS) void policy_sample_vjp_kernel(const PolicySampleVjpArgs A) {
    const int act_dim = A.out_dim >> 1;
    const size_t item = (size_t)blockIdx.x * PS_THREADS + threadIdx.x;
    if (item >= (size_t)A.n * act_dim) return;
    const size_t e = item / (unsigned)act_dim;
    const int a = (int)(item - e * act_dim);
    const float* y = A.logits + e * A.out_dim;
    float g_mean, g_ls;
    psample::sample_vjp_elem(y[a], y[act_dim + a], A.eps[item], A.action_range, A.g_actions ? A.g_actions[item] : 0.0f,
                             A.g_logp ? A.g_logp[e] : 0.0f, g_mean, g_ls);
    float* g = A.g_logits + e * A.out_dim;
    g[a] = g_mean;
    g[act_dim + a] = g_ls;
}

hipError_t launch_policy_sample_vjp(const PolicySampleVjpArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const size_t items = (size_t)A.n * (A.out_dim >> 1);
    hipLaunchKernelGGL(policy_sample_vjp_kernel, dim3((unsigned)((items + PS_THREADS - 1) / PS_THREADS)), dim3(PS_THREADS), 0, s, A);
    return hipGetLastError();
}

}  // namespace eb
