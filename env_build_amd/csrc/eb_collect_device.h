// eb_collect_device.h — the slot copy and the block folds of the collection kernels (include/envbuild_collect.h), each defined ONCE: the
// kernels of eb_collect.hip call these and nothing else does the arithmetic.  No other library's header is included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eb {
namespace collect {

constexpr int THREADS = 256;               // of all four kernels
constexpr int ENVS = 32;                   // envs of one block of the begin and record kernels

// dst[0 .. n) = src[0 .. n), n floats in ONE contiguous run on both sides, by the block's THREADS lanes: consecutive lanes on consecutive
// elements.  wide (uniform over the launch: both runs start 16-byte aligned) moves n / 4 float4s and the n % 4 floats behind them as
// dwords; otherwise everything goes as dwords.
__device__ __forceinline__ void copy_run(float* __restrict__ dst, const float* __restrict__ src, int n, bool wide, int t) {
    int done = 0;
    if (wide) {
        const int quads = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int q = t; q < quads; q += THREADS) d4[q] = s4[q];
        done = quads << 2;
    }
    for (int e = done + t; e < n; e += THREADS) dst[e] = src[e];
}

// the block's THREADS doubles in `red` (LDS) folded by halving in one fixed order, x[t] = op(x[t], x[t + w]) for w = 128 .. 1; every lane
// returns the result.  OP 0: the sum; 1: the larger; 2: the smaller (no NaN enters the last two: the callers select from -inf / +inf).
template <int OP>
__device__ __forceinline__ double fold(double* red, int t, double x) {
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (t < w) {
            const double a = red[t], b = red[t + w];
            red[t] = OP == 0 ? a + b : OP == 1 ? (b > a ? b : a) : (b < a ? b : a);
        }
        __syncthreads();
    }
    const double out = red[0];
    __syncthreads();                        // red is free for the next fold
    return out;
}

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }     // false for a NaN and for +-inf

}  // namespace collect
}  // namespace eb
