// eb_policy_grad.hip — the policy network's backward on the f32 matrix cores (include/envbuild_mlp_grad.h), gfx950 only.
//
// Three kernels, all on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 sums), __syncthreads() the only synchronisation, no atomics:
//
//   * mlp_pack_kernel — eb_mlp_set_params_device: every packing the handle keeps (pack_weights / pack_weights16 of eb_policy.hip, the
//     binary16 packings of eb_policy_f16.hip, the padded biases and the transposed packing below) filled from ONE flat device buffer
//     in Model.get_weights() order.  One launch, no host copy.
//   * mlp_bwd_data_kernel<RT, CT> — one block = 64 rows x 4 waves with the forward's tiling (eb_policy.hip: U = 64 / 128 / 256).  The
//     forward is recomputed with mlp_kernel's own chain (layer_chain / store_hidden of eb_mlp_device.h: bias in the accumulator,
//     products added in ascending k), so `out` has eb_mlp_forward's bits; every x_l goes to the workspace.  Then the chain runs backwards: the
//     cotangent d_l sits in LDS in the activation layout as the A operand, the B operand is pack_weights applied to W_l TRANSPOSED
//     (the handle's d_wt[]), the accumulator starts at zero and the epilogue multiplies by the activation's derivative taken from the
//     activation's OUTPUT, which the same lane wrote to the workspace on the way forward (the tiling of both passes is the same, so a
//     lane reads back its own stores).  Every d_l goes to the workspace; the product with W_0 transposed has ceil(obs_dim / 32) column
//     tiles — not a hidden width — and runs in a column-tile loop of its own, straight to g_obs.
//   * mlp_wgrad_kernel + mlp_wgrad_reduce_kernel — dW_l[k, u] = sum over rows r of x_l[r, k] * d_l[r, u]: the ROWS are the reduction
//     dimension.  Lane l of a wave supplies A[k = l & 31][r = 2m + (l >> 5)] and B[r][u = l & 31] straight from the row-major
//     workspace (32 lanes read 128 contiguous bytes).  A wave owns a 64 x 64 tile of one layer for one split of 512 rows (grid:
//     (layer, k block, u block) x row splits, 4 splits per block) and writes its partial tile, with the column sums (the bias
//     gradient) as one more row; the reduce kernel adds a tile's partials in ascending split order and writes the unpadded g_params.
//     Same inputs, same bits: the order of every sum is fixed by the launch geometry, which depends on n and the handle only.
#include "eb_policy_grad.h"

#include "eb_mlp_device.h"

namespace eb {

// LDS layout of the activations and of the cotangents: element (row i, input k) at i * RS + (k & 1) * HS + (k >> 1); RS = Kmax + 4
// floats, HS = Kmax / 2 (eb_policy.hip).
template <int RT, int CT>
__global__ __launch_bounds__(MLP_THREADS, 2) void mlp_bwd_data_kernel(const MlpGradArgs G) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpArgs& A = G.fwd;
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;   // (the wave index in an SGPR)
    const int i = lane & 31, h = lane >> 5;
    const int RS = A.row_stride, HS = (RS - 4) >> 1;
    const int row0 = blockIdx.x * MLP_ROWS;
    const int rows_here = A.n - row0 < MLP_ROWS ? A.n - row0 : MLP_ROWS;
    const int D = A.obs_dim, K0 = A.hid[0].k_pad, U = A.units, H = A.n_hidden;

    // ---- stage the (preprocessed) observations as mlp_kernel does; x_0 also goes to the workspace ----
    {
        constexpr int RPW = MLP_ROWS / 4, KC = 3;
        const int rbase = wave * RPW;
        float* x0g = G.ws + G.x_off[0] + (size_t)(row0 + rbase) * K0;
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
                    for (int rr = 0; rr < RPW; ++rr) {
                        const float x = (rbase + rr < rows_here && k < D) ? v[c][rr] * sc[c] : 0.0f;
                        dst[rr * RS] = x;
                        x0g[(size_t)rr * K0 + k] = x;
                    }
                }
            }
        }
    }
    __syncthreads();

    // ---- hidden layers, forward ----
    const int rt0 = RT == 2 ? 0 : (wave & 1);
    const int ct0 = RT == 2 ? wave * CT : (wave >> 1);
    const float* a_row = lds + (rt0 * 32 + i) * RS + h * HS;
    for (int L = 0; L < H; ++L) {
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
        mlp::layer_chain<RT, CT>(a_row, 32 * RS, reinterpret_cast<const mlp::f32x4*>(ly.w), ly.k_pad >> 3, ct0, lane, acc);
        __syncthreads();                                              // every wave has read this layer's inputs
        float* xg = G.ws + G.x_off[L + 1] + (size_t)row0 * U;
        switch (A.hidden_act) {
            case MLP_ACT_RELU: mlp::store_hidden<RT, CT, MLP_ACT_RELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
            case MLP_ACT_ELU: mlp::store_hidden<RT, CT, MLP_ACT_ELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
            case MLP_ACT_TANH: mlp::store_hidden<RT, CT, MLP_ACT_TANH>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
            default: mlp::store_hidden<RT, CT, MLP_ACT_LINEAR>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
        }
        __syncthreads();
    }

    // ---- output layer as mlp_kernel runs it (16 x 16 x 4 tiles, row tile = wave), and the cotangent of its pre-activations ----
    float dl[2][4];                                                      // out_dim <= 32: at most two column tiles of 16
    {
        const int i16 = lane & 15, kq = lane >> 4, hsel = kq >> 1;
        const int steps4 = A.outl.k_pad >> 4;
        const float* a_ptr = lds + (wave * 16 + i16) * RS + (kq & 1) * HS;
        const mlp::f32x4* w16 = reinterpret_cast<const mlp::f32x4*>(A.outl.w);
        const int ct16 = (A.out_dim + 15) >> 4;
        const int act_dim = A.out_dim >> 1;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
#pragma unroll
            for (int v = 0; v < 4; ++v) dl[ct][v] = 0.0f;
            if (ct < ct16) {
                const float b = A.outl.b[ct * 16 + i16];
                mlp::f32x4 acc = {b, b, b, b};
                const mlp::f32x4* wsrc = w16 + (size_t)ct * steps4 * 64 + lane;
                mlp::f32x4 bq = wsrc[0];
                for (int s4 = 0; s4 < steps4; ++s4) {
                    const mlp::f32x4 bn = wsrc[(size_t)(s4 + 1 < steps4 ? s4 + 1 : s4) * 64];
                    const mlp::f32x4 a01 = *reinterpret_cast<const mlp::f32x4*>(a_ptr + 8 * s4);
                    const mlp::f32x4 a23 = *reinterpret_cast<const mlp::f32x4*>(a_ptr + 8 * s4 + 4);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a01[1] : a01[0], bq[0], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a01[3] : a01[2], bq[1], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a23[1] : a23[0], bq[2], acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a23[3] : a23[2], bq[3], acc, 0, 0, 0);
                    bq = bn;
                }
                const int col = ct * 16 + i16;
                const int gcols = A.head == MLP_HEAD_LOGITS ? A.out_dim : act_dim;
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int row = wave * 16 + 4 * kq + v;
                    const bool live = row < rows_here && col < gcols;
                    const float y = mlp::activate_rt(A.out_act, acc[v]);
                    const float g = live ? G.g_out[(size_t)(row0 + row) * gcols + col] : 0.0f;
                    float o = y, d = g;
                    if (A.head != MLP_HEAD_LOGITS && A.action_range > 0.0f) {   // action = action_range * tanh(mean)
                        const float t = mlp::tanh_det(y);
                        o = A.action_range * t;
                        d = (g * A.action_range) * (1.0f - t * t);
                    }
                    d = d * mlp::derivative_rt(A.out_act, y);
                    if (live && A.out) A.out[(size_t)(row0 + row) * gcols + col] = o;
                    dl[ct][v] = live ? d : 0.0f;                         // rows beyond n and the log-std columns: exact zeros
                }
            }
        }
        __syncthreads();                                                 // every wave has read x_H
        float* dg = G.ws + G.d_off[H] + (size_t)row0 * 32;
#pragma unroll
        for (int ct = 0; ct < 2; ++ct) {
            const int col = ct * 16 + i16;
#pragma unroll
            for (int v = 0; v < 4; ++v) {
                const int row = wave * 16 + 4 * kq + v;
                if (col < G.kt_out) lds[row * RS + (col & 1) * HS + (col >> 1)] = dl[ct][v];
                dg[(size_t)row * 32 + col] = dl[ct][v];
            }
        }
        __syncthreads();
    }

    // ---- backwards: d_{L-1} = (d_L * W_L^T) (.) act'(x_L), the transposed packing as the B operand, no bias ----
    for (int L = H; L >= 1; --L) {
        mlp::f32x16 acc[RT][CT];
#pragma unroll
        for (int c = 0; c < CT; ++c)
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[r][c][v] = 0.0f;
        mlp::layer_chain<RT, CT>(a_row, 32 * RS, reinterpret_cast<const mlp::f32x4*>(G.wt[L]), (L == H ? G.kt_out : U) >> 3, ct0, lane, acc);
        __syncthreads();                                              // every wave has read d_L
        const float* xg = G.ws + G.x_off[L] + (size_t)row0 * U;
        float* dg = G.ws + G.d_off[L - 1] + (size_t)row0 * U;
        switch (A.hidden_act) {
            case MLP_ACT_RELU: mlp::store_delta<RT, CT, MLP_ACT_RELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
            case MLP_ACT_ELU: mlp::store_delta<RT, CT, MLP_ACT_ELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
            case MLP_ACT_TANH: mlp::store_delta<RT, CT, MLP_ACT_TANH>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
            default: mlp::store_delta<RT, CT, MLP_ACT_LINEAR>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
        }
        __syncthreads();
    }

    // ---- g_obs = (d_0 * W_0^T) (.) scale: ceil(obs_dim / 32) column tiles, one per wave and trip, both row tiles ----
    if (G.g_obs) {
        const int tiles = (D + 31) >> 5;
        for (int ct = wave; ct < tiles; ct += 4) {
            mlp::f32x16 acc[2][1];
#pragma unroll
            for (int r = 0; r < 2; ++r)
#pragma unroll
                for (int v = 0; v < 16; ++v) acc[r][0][v] = 0.0f;
            mlp::layer_chain<2, 1>(lds + i * RS + h * HS, 32 * RS, reinterpret_cast<const mlp::f32x4*>(G.wt[0]), U >> 3, ct, lane, acc);
            const int col = ct * 32 + i;
            if (col < D) {
                const float sc = A.scale ? A.scale[col] : 1.0f;
#pragma unroll
                for (int r = 0; r < 2; ++r)
#pragma unroll
                    for (int v = 0; v < 16; ++v) {
                        const int row = r * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                        if (row < rows_here) G.g_obs[(size_t)(row0 + row) * D + col] = acc[r][0][v] * sc;
                    }
            }
        }
    }
}

// dW and db of one (layer, 64 inputs, 64 columns) tile over one split of the rows, per wave.
__global__ __launch_bounds__(MLP_THREADS) void mlp_wgrad_kernel(const MlpGradArgs G) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int i = lane & 31, h = lane >> 5;
    const int n = G.fwd.n;
    const int split = blockIdx.y * 4 + wave;
    const int r0 = split * MLP_GRAD_SPLIT_ROWS;
    if (r0 >= n) return;
    const int r1 = r0 + MLP_GRAD_SPLIT_ROWS < n ? r0 + MLP_GRAD_SPLIT_ROWS : n;
    int l = 0;
    while (l < G.fwd.n_hidden && (int)blockIdx.x >= G.wl[l + 1].task0) ++l;
    const MlpWgradLayer& W = G.wl[l];
    const int t = (int)blockIdx.x - W.task0;
    const int kblk = t / W.ub, ublk = t - kblk * W.ub;
    const int k0 = kblk * 64, u0 = ublk * 64;
    const int xs = W.x_stride, ds = W.d_stride;

    bool kin[2], uin[2], kact[2], uact[2];
    const float* xp[2];
    const float* dp[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        const int k = k0 + 32 * a + i, u = u0 + 32 * a + i;
        kin[a] = k < W.k_real;
        uin[a] = u < W.u_real;
        kact[a] = k0 + 32 * a < W.k_real;                                // wave-uniform: does this tile hold a real input / column
        uact[a] = u0 + 32 * a < W.u_real;
        xp[a] = W.x + (kin[a] ? k : 0);
        dp[a] = W.d + (uin[a] ? u : 0);
    }
    mlp::f32x16 acc[2][2];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[a][c][v] = 0.0f;
    float bs[2] = {0.0f, 0.0f};

    for (int rb = r0; rb < r1; rb += 8) {                                // four MFMA steps of two rows each
        float xa[4][2], db[4][2];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int r = rb + 2 * q + h;
            const bool live = r < r1;
            const size_t rr = live ? r : r0;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                const float x = xp[a][rr * xs], d = dp[a][rr * ds];
                xa[q][a] = (live && kin[a]) ? x : 0.0f;
                db[q][a] = (live && uin[a]) ? d : 0.0f;
            }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int a = 0; a < 2; ++a)
#pragma unroll
                for (int c = 0; c < 2; ++c)
                    if (kact[a] && uact[c]) acc[a][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[q][a], db[q][c], acc[a][c], 0, 0, 0);
            bs[0] += db[q][0];
            bs[1] += db[q][1];
        }
    }

    const int width = W.ub * 64;
    float* P = G.ws + G.part_off + (size_t)split * G.part_stride + W.part_off;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c)
            if (kact[a] && uact[c]) {
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int k = k0 + 32 * a + (v & 3) + 8 * (v >> 2) + 4 * h;
                    P[(size_t)k * width + u0 + 32 * c + i] = acc[a][c][v];
                }
            }
    if (kblk == 0) {                                                     // the bias row: even rows' sum + odd rows' sum
#pragma unroll
        for (int c = 0; c < 2; ++c) {
            const float other = __shfl_xor(bs[c], 32);
            if (h == 0 && uact[c]) P[(size_t)W.kb * 64 * width + u0 + 32 * c + i] = bs[c] + other;
        }
    }
}

// g_params[e] = the partials of element e added in ascending split order (zero splits: zero)
__global__ __launch_bounds__(256) void mlp_wgrad_reduce_kernel(const MlpGradArgs G, int splits) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= G.param_count) return;
    int l = 0;
    while (l < G.fwd.n_hidden && e >= G.wl[l + 1].w_off) ++l;
    const MlpWgradLayer& W = G.wl[l];
    const int width = W.ub * 64;
    long long at;
    if (e < W.b_off) {
        const long long j = e - W.w_off;
        const long long k = j / W.u_real;
        at = k * width + (j - k * W.u_real);
    } else {
        at = (long long)W.kb * 64 * width + (e - W.b_off);
    }
    const float* P = G.ws + G.part_off + W.part_off + at;
    float sum = 0.0f;
    for (int s = 0; s < splits; ++s) sum += P[(size_t)s * G.part_stride];
    G.g_params[e] = sum;
}

size_t mlp_grad_layout(MlpGradArgs& A) {
    const MlpArgs& F = A.fwd;
    const int H = F.n_hidden, U = F.units, K0 = F.hid[0].k_pad;
    const long long n_pad = ((long long)F.n + MLP_ROWS - 1) / MLP_ROWS * MLP_ROWS;
    const long long splits = ((long long)F.n + MLP_GRAD_SPLIT_ROWS - 1) / MLP_GRAD_SPLIT_ROWS;
    long long at = 0;
    for (int L = 0; L <= H; ++L) { A.x_off[L] = at; at += n_pad * (L == 0 ? K0 : U); }
    for (int L = 0; L <= H; ++L) { A.d_off[L] = at; at += n_pad * (L == H ? 32 : U); }
    long long part = 0, param = 0;
    int task = 0;
    for (int L = 0; L <= H; ++L) {
        MlpWgradLayer& W = A.wl[L];
        W.x_stride = L == 0 ? K0 : U;
        W.d_stride = L == H ? 32 : U;
        W.k_real = L == 0 ? F.obs_dim : A.n_units;
        W.u_real = L == H ? F.out_dim : A.n_units;
        W.kb = (W.k_real + 63) / 64;
        W.ub = (W.u_real + 63) / 64;
        W.task0 = task;
        W.pad_ = 0;
        W.part_off = part;
        W.w_off = param;
        W.b_off = param + (long long)W.k_real * W.u_real;
        task += W.kb * W.ub;
        part += ((long long)W.kb * 64 + 1) * W.ub * 64;
        param = W.b_off + W.u_real;
    }
    A.n_tasks = task;
    A.part_off = at;
    A.part_stride = part;
    A.param_count = param;
    at += splits * part;
    return (size_t)at * sizeof(float);
}

hipError_t launch_mlp_backward(const MlpGradArgs& A, hipStream_t s) {
    const MlpArgs& F = A.fwd;
    const int H = F.n_hidden;
    if (F.n > 0) {
        MlpGradArgs B = A;
        for (int L = 0; L <= H; ++L) {
            B.wl[L].x = A.ws + A.x_off[L];
            B.wl[L].d = A.ws + A.d_off[L];
        }
        const dim3 g((F.n + MLP_ROWS - 1) / MLP_ROWS), b(MLP_THREADS);
        const size_t lds = mlp_lds_bytes(F);
        const int dev = current_device_index();
        hipError_t e = F.units == 64 ? launch_lds<&mlp_bwd_data_kernel<1, 1>>(g, b, lds, dev, s, B)
                       : F.units == 128 ? launch_lds<&mlp_bwd_data_kernel<2, 1>>(g, b, lds, dev, s, B)
                                        : launch_lds<&mlp_bwd_data_kernel<2, 2>>(g, b, lds, dev, s, B);
        if (e == hipSuccess) e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (A.g_params) {
            const int splits = (F.n + MLP_GRAD_SPLIT_ROWS - 1) / MLP_GRAD_SPLIT_ROWS;
            hipLaunchKernelGGL(mlp_wgrad_kernel, dim3(A.n_tasks, (splits + 3) / 4), dim3(MLP_THREADS), 0, s, B);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
    }
    if (A.g_params) {
        const int splits = F.n > 0 ? (F.n + MLP_GRAD_SPLIT_ROWS - 1) / MLP_GRAD_SPLIT_ROWS : 0;
        hipLaunchKernelGGL(mlp_wgrad_reduce_kernel, dim3((unsigned)((A.param_count + 255) / 256)), dim3(256), 0, s, A, splits);
        return hipGetLastError();
    }
    return hipSuccess;
}

// the row reduction alone: A.ws already holds x_l and d_l for A.fwd.n rows in mlp_grad_layout's places (eb_policy_rollout_grad.hip's
// block writes them step by step); same grids, so same sums, as the tail of launch_mlp_backward
hipError_t launch_mlp_wgrad(const MlpGradArgs& A, hipStream_t s) {
    const MlpArgs& F = A.fwd;
    if (!A.g_params) return hipSuccess;
    const int splits = F.n > 0 ? (F.n + MLP_GRAD_SPLIT_ROWS - 1) / MLP_GRAD_SPLIT_ROWS : 0;
    if (F.n > 0) {
        MlpGradArgs B = A;
        for (int L = 0; L <= F.n_hidden; ++L) {
            B.wl[L].x = A.ws + A.x_off[L];
            B.wl[L].d = A.ws + A.d_off[L];
        }
        hipLaunchKernelGGL(mlp_wgrad_kernel, dim3(A.n_tasks, (splits + 3) / 4), dim3(MLP_THREADS), 0, s, B);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(mlp_wgrad_reduce_kernel, dim3((unsigned)((A.param_count + 255) / 256)), dim3(256), 0, s, A, splits);
    return hipGetLastError();
}

// ---- eb_mlp_set_params_device ----
// binary16 bits of x: the hardware conversion (round to nearest even, overflow to +-inf, subnormal results kept)
EB_DEV uint16_t f16_bits_dev(float x) { return __builtin_bit_cast(uint16_t, (_Float16)x); }

// blockIdx.y = layer; the threads of a layer stride over the elements of each of its four packings in turn.  Every destination element
// is written (padding: zeros), so the handle afterwards holds what eb_mlp_set_layer would have put there.
__global__ __launch_bounds__(256) void mlp_pack_kernel(const MlpPackArgs A) {
    const MlpPackLayer& Y = A.layer[blockIdx.y];
    const float* __restrict__ W = A.params + Y.w_off;
    const float* __restrict__ Bv = A.params + Y.b_off;
    const int kr = Y.k_real, cr = Y.cols_real;
    const int first = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    auto weight = [&](int k, int j) { return (k < kr && j < cr) ? W[(size_t)k * cr + j] : 0.0f; };

    // fp32: per column tile, per step, per lane, the 4 values that lane feeds to 4 consecutive MFMAs
    const int n_w = Y.k_pad * Y.col_tiles * 32;
    if (!Y.is_out) {
        const int steps = Y.k_pad / 8;
        for (int e = first; e < n_w; e += stride) {
            const int q = e & 3, l = (e >> 2) & 63, cs = e >> 8, s = cs % steps, ct = cs / steps;
            Y.w[e] = weight(2 * (s * 4 + q) + (l >> 5), ct * 32 + (l & 31));
        }
    } else {                                                             // pack_weights16: 16-column tiles, groups of 16 inputs
        const int groups = Y.k_pad / 16, tiles = (cr + 15) / 16;
        for (int e = first; e < n_w; e += stride) {
            const int q = e & 3, l = (e >> 2) & 63, cg = e >> 8, g = cg % groups, ct = cg / groups;
            Y.w[e] = ct < tiles ? weight(4 * (4 * g + q) + (l >> 4), ct * 16 + (l & 15)) : 0.0f;
        }
    }
    // binary16: per tile, per step, per lane, the 8 halves of one fragment
    const int n_h = Y.k_pad16 * (Y.is_out ? 32 : A.units);
    if (!Y.is_out) {
        const int steps = Y.k_pad16 / 16;
        for (int e = first; e < n_h; e += stride) {
            const int j = e & 7, l = (e >> 3) & 63, cs = e >> 9, s = cs % steps, ct = cs / steps;
            Y.w16[e] = f16_bits_dev(weight(16 * s + 8 * (l >> 5) + j, ct * 32 + (l & 31)));
        }
    } else {
        const int steps = Y.k_pad16 / 32, tiles = (cr + 15) / 16;
        for (int e = first; e < n_h; e += stride) {
            const int j = e & 7, l = (e >> 3) & 63, cs = e >> 9, s = cs % steps, ct = cs / steps;
            Y.w16[e] = ct < tiles ? f16_bits_dev(weight(32 * s + 8 * (l >> 4) + j, ct * 16 + (l & 15))) : (uint16_t)0;
        }
    }
    // transposed: pack_weights of the [cols_real, k_real] matrix W^T
    {
        const int n_t = Y.kt_pad * Y.colt_tiles * 32, steps = Y.kt_pad / 8;
        for (int e = first; e < n_t; e += stride) {
            const int q = e & 3, l = (e >> 2) & 63, cs = e >> 8, s = cs % steps, ct = cs / steps;
            Y.wt[e] = weight(ct * 32 + (l & 31), 2 * (s * 4 + q) + (l >> 5));
        }
    }
    for (int e = first; e < Y.col_tiles * 32; e += stride) Y.b[e] = e < cr ? Bv[e] : 0.0f;
}

hipError_t launch_mlp_pack(const MlpPackArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(mlp_pack_kernel, dim3(64, A.n_layers), dim3(256), 0, s, A);
    return hipGetLastError();
}

}  // namespace eb
