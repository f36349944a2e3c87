// eb_policy_logp.hip — the log-probability of GIVEN actions under the policy (include/envbuild_policy_logp.h), gfx950: network and
// epilogue in ONE launch, the same epilogue alone on given logits, and its reverse pass (the action is data: cotangents go to the mean
// and the log-std only).
//
// policy_logp_kernel<RT, CT> is policy_sample_kernel's structure with another row function: phead::logits_to_lds
// (eb_policy_head_device.h) is mlp_kernel up to the activated logits — so logits_out is eb_mlp_forward's bits — and leaves the block's
// 64 x out_dim logits in the freed activation buffer with a row stride of 33 floats.  Then one lane per row — lanes 0..15 of each wave
// for the wave's own 16 rows — reads its row's act_dim actions from global memory and runs plogp::logp_row in ascending a.
// __syncthreads only, no LDS beyond mlp_kernel's, no atomics, plain vector stores.
// policy_logp_logits_kernel calls the same logp_row on rows of global memory: eb_policy_logp equals eb_mlp_forward followed by
// eb_policy_logp_from_logits bit for bit because there is one definition of the row.
#include "eb_policy_logp.h"
#include "eb_policy_head_device.h"
#include "eb_policy_logp_device.h"

namespace eb {
namespace {

constexpr int PL_THREADS = 256;  // of the two elementwise kernels

}  // namespace

template <int RT, int CT>
__global__ __launch_bounds__(MLP_THREADS, CT == 4 ? 1 : 2) void policy_logp_kernel(const PolicyLogpArgs P) {   // waves per SIMD
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpArgs& A = P.fwd;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = blockIdx.x * MLP_ROWS;
    const int rows_here = A.n - row0 < MLP_ROWS ? A.n - row0 : MLP_ROWS;
    phead::logits_to_lds<RT, CT>(A, lds, wave, lane, row0, rows_here);

    // ---- the epilogue: one lane per row, lanes 0..15 of each wave take the wave's own rows ----
    const int row = wave * 16 + lane;
    if (lane < 16 && row < rows_here) {
        const PolicyLogpHead& S = P.head;
        const size_t e = (size_t)(row0 + row);
        const int act_dim = A.out_dim >> 1;
        plogp::logp_row(lds + row * phead::LS, act_dim, S.actions + e * act_dim, S.action_range, S.log_ar, S.logp + e,
                        S.z_out ? S.z_out + e * act_dim : nullptr);
    }
}

hipError_t launch_policy_logp(const PolicyLogpArgs& A, hipStream_t s) {
    if (A.fwd.n <= 0) return hipSuccess;
    const dim3 g((A.fwd.n + MLP_ROWS - 1) / MLP_ROWS), b(MLP_THREADS);
    const size_t lds = mlp_lds_bytes(A.fwd);
    const int dev = current_device_index();
    const hipError_t e = A.fwd.units == 64 ? launch_lds<&policy_logp_kernel<1, 1>>(g, b, lds, dev, s, A)
                         : A.fwd.units == 128 ? launch_lds<&policy_logp_kernel<2, 1>>(g, b, lds, dev, s, A)
                         : A.fwd.units == 256 ? launch_lds<&policy_logp_kernel<2, 2>>(g, b, lds, dev, s, A)
                                              : launch_lds<&policy_logp_kernel<2, 4>>(g, b, lds, dev, s, A);
    return e != hipSuccess ? e : hipGetLastError();
}

// ---- the epilogue alone: one lane per row of [n, out_dim] logits in global memory ----
__global__ __launch_bounds__(PL_THREADS) void policy_logp_logits_kernel(const PolicyLogpLogitsArgs A) {
    const size_t e = (size_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (e >= (size_t)A.n) return;
    const PolicyLogpHead& S = A.head;
    const int act_dim = A.out_dim >> 1;
    plogp::logp_row(A.logits + e * A.out_dim, act_dim, S.actions + e * act_dim, S.action_range, S.log_ar, S.logp + e,
                    S.z_out ? S.z_out + e * act_dim : nullptr);
}

hipError_t launch_policy_logp_from_logits(const PolicyLogpLogitsArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(policy_logp_logits_kernel, dim3((A.n + PL_THREADS - 1) / PL_THREADS), dim3(PL_THREADS), 0, s, A);
    return hipGetLastError();
}

// ---- the reverse pass: one lane per (row, a) ----
__global__ __launch_bounds__(PL_THREADS) void policy_logp_vjp_kernel(const PolicyLogpVjpArgs A) {
    const int act_dim = A.out_dim >> 1;
    const size_t item = (size_t)blockIdx.x * PL_THREADS + threadIdx.x;
    if (item >= (size_t)A.n * act_dim) return;
    const size_t e = item / (unsigned)act_dim;
    const int a = (int)(item - e * act_dim);
    float g_mean, g_ls;
    plogp::logp_vjp_elem(A.logits[e * A.out_dim + act_dim + a], A.z[item], A.g_logp[e], g_mean, g_ls);
    float* g = A.g_logits + e * A.out_dim;
    g[a] = g_mean;
    g[act_dim + a] = g_ls;
}

hipError_t launch_policy_logp_vjp(const PolicyLogpVjpArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const size_t items = (size_t)A.n * (A.out_dim >> 1);
    hipLaunchKernelGGL(policy_logp_vjp_kernel, dim3((unsigned)((items + PL_THREADS - 1) / PL_THREADS)), dim3(PL_THREADS), 0, s, A);
    return hipGetLastError();
}

}  // namespace eb
