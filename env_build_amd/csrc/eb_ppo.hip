// eb_ppo.hip — the PPO update's arithmetic (include/envbuild_ppo.h), gfx950: the clipped surrogate, its entropy bonus and the cotangent
// of the logits in ONE launch with the policy network, the same row alone on given logits, and generalised advantage estimation over
// [T, n] arrays in one launch.
//
// ppo_surrogate_kernel<RT, CT> is policy_logp_kernel's structure with another row function: phead::logits_to_lds
// (eb_policy_head_device.h) is mlp_kernel up to the activated logits — so logits_out is eb_mlp_forward's bits — and leaves the block's
// 64 x out_dim logits in the freed activation buffer with a row stride of 33 floats.  Then one lane per row — lanes 0..15 of each wave
// for the wave's own 16 rows — runs ppo::surrogate_row on its LDS row.  __syncthreads only, no LDS beyond mlp_kernel's, no atomics,
// plain vector stores.
// ppo_surrogate_logits_kernel copies each lane's row of global logits to an LDS row of the same stride and calls the same
// surrogate_row: eb_ppo_surrogate equals eb_mlp_forward followed by eb_ppo_surrogate_from_logits bit for bit because there is one
// definition of the row.
// gae_kernel: one lane per env, so every load and store of a step is one coalesced line per wave; the recursion is three dependent
// operations per step and no load depends on it.  A window of GAE_WIN steps is raw loads only — nothing loaded is read while the window
// is being loaded, so its 12 to 20 loads issue back to back — and the next window is issued before the current one's arithmetic and
// stores; the waits sit where the next window is moved into the current one.  One memory round trip per window of GAE_WIN steps, under
// the current window's work, not one per step: in the assembly the loop body is the loads with no s_waitcnt vmcnt between them, the four
// steps' arithmetic and stores, then the waits on the moves.
#include "eb_ppo.h"
#include "eb_policy_head_device.h"
#include "eb_ppo_device.h"

namespace eb {
namespace {

constexpr int PPO_THREADS = 128;  // of the elementwise surrogate kernel: 128 LDS rows of phead::LS floats
constexpr int GAE_THREADS = 64;   // small blocks: 4 096 envs are 64 blocks
constexpr int GAE_WIN = 4;        // steps per register window

}  // namespace

template <int RT, int CT>
__global__ __launch_bounds__(MLP_THREADS, CT == 4 ? 1 : 2) void ppo_surrogate_kernel(const PpoArgs P) {   // waves per SIMD
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const MlpArgs& A = P.fwd;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int row0 = blockIdx.x * MLP_ROWS;
    const int rows_here = A.n - row0 < MLP_ROWS ? A.n - row0 : MLP_ROWS;
    phead::logits_to_lds<RT, CT>(A, lds, wave, lane, row0, rows_here);

    // ---- the epilogue: one lane per row, lanes 0..15 of each wave take the wave's own rows ----
    const int row = wave * 16 + lane;
    if (lane < 16 && row < rows_here)
        ppo::surrogate_row(lds + row * phead::LS, A.out_dim >> 1, (size_t)(row0 + row), P.head);
}

hipError_t launch_ppo_surrogate(const PpoArgs& A, hipStream_t s) {
    if (A.fwd.n <= 0) return hipSuccess;
    const dim3 g((A.fwd.n + MLP_ROWS - 1) / MLP_ROWS), b(MLP_THREADS);
    const size_t lds = mlp_lds_bytes(A.fwd);
    const int dev = current_device_index();
    const hipError_t e = A.fwd.units == 64 ? launch_lds<&ppo_surrogate_kernel<1, 1>>(g, b, lds, dev, s, A)
                         : A.fwd.units == 128 ? launch_lds<&ppo_surrogate_kernel<2, 1>>(g, b, lds, dev, s, A)
                         : A.fwd.units == 256 ? launch_lds<&ppo_surrogate_kernel<2, 2>>(g, b, lds, dev, s, A)
                                              : launch_lds<&ppo_surrogate_kernel<2, 4>>(g, b, lds, dev, s, A);
    return e != hipSuccess ? e : hipGetLastError();
}

// ---- the row alone: one lane per row of [n, out_dim] logits in global memory, through the lane's own LDS row ----
__global__ __launch_bounds__(PPO_THREADS) void ppo_surrogate_logits_kernel(const PpoLogitsArgs A) {
    __shared__ float rows[PPO_THREADS * phead::LS];
    const size_t e = (size_t)blockIdx.x * PPO_THREADS + threadIdx.x;
    if (e >= (size_t)A.n) return;
    float* y = rows + threadIdx.x * phead::LS;
    const float* src = A.logits + e * A.out_dim;
    for (int c = 0; c < A.out_dim; ++c) y[c] = src[c];
    ppo::surrogate_row(y, A.out_dim >> 1, e, A.head);
}

hipError_t launch_ppo_surrogate_from_logits(const PpoLogitsArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppo_surrogate_logits_kernel, dim3((A.n + PPO_THREADS - 1) / PPO_THREADS), dim3(PPO_THREADS), 0, s, A);
    return hipGetLastError();
}

// ---- generalised advantage estimation: one lane per env, t = T-1 .. 0 ----
namespace {

struct GaeWindow {
    float reward[GAE_WIN], value[GAE_WIN], nonterminal[GAE_WIN], carry[GAE_WIN], next[GAE_WIN];
};

// the loads of steps t, t-1, .. t-GAE_WIN+1 of env i, and nothing else: no value loaded here is read here, so the loads issue back to
// back.  carry and next are loaded only where given (a uniform condition) and otherwise stay as they are; which one a step uses is
// decided where it is computed.  A step below 0 reads step 0 (in bounds) and is not used.
__device__ __forceinline__ void gae_load(const GaeArgs& A, int i, int t, GaeWindow& W) {
    size_t at[GAE_WIN];
#pragma unroll
    for (int k = 0; k < GAE_WIN; ++k) at[k] = (size_t)(t - k > 0 ? t - k : 0) * (size_t)A.n + (size_t)i;
#pragma unroll
    for (int k = 0; k < GAE_WIN; ++k) {
        W.reward[k] = A.rewards[at[k]];
        W.value[k] = A.values[at[k]];
        W.nonterminal[k] = A.nonterminal[at[k]];
    }
    if (A.carry) {
#pragma unroll
        for (int k = 0; k < GAE_WIN; ++k) W.carry[k] = A.carry[at[k]];
    }
    if (A.next_values) {
#pragma unroll
        for (int k = 0; k < GAE_WIN; ++k) W.next[k] = A.next_values[at[k]];
    }
}

}  // namespace

__global__ __launch_bounds__(GAE_THREADS) void gae_kernel(const GaeArgs A) {
    const int i = blockIdx.x * GAE_THREADS + threadIdx.x;
    if (i >= A.n) return;
    float run = 0.0f;
    float above = A.next_values ? 0.0f : A.v_last[i];                 // values[t + 1], v_last above the last step
    GaeWindow cur = {};
    gae_load(A, i, A.T - 1, cur);
    GaeWindow nxt = cur;
    for (int t = A.T - 1; t >= 0; t -= GAE_WIN) {
        if (t - GAE_WIN >= 0) gae_load(A, i, t - GAE_WIN, nxt);       // in flight under this window's arithmetic and stores
#pragma unroll
        for (int k = 0; k < GAE_WIN; ++k) {
            if (t - k >= 0) {
                const size_t at = (size_t)(t - k) * (size_t)A.n + (size_t)i;
                const float vn = A.next_values ? cur.next[k] : above;
                const float cy = A.carry ? cur.carry[k] : cur.nonterminal[k];
                run = ppo::gae_step(cur.reward[k], cur.value[k], vn, cur.nonterminal[k], cy, A.gamma, A.gl, run);
                A.adv[at] = run;
                if (A.ret) A.ret[at] = run + cur.value[k];
                above = cur.value[k];
            }
        }
        cur = nxt;
    }
}

hipError_t launch_gae(const GaeArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(gae_kernel, dim3((A.n + GAE_THREADS - 1) / GAE_THREADS), dim3(GAE_THREADS), 0, s, A);
    return hipGetLastError();
}

}  // namespace eb
