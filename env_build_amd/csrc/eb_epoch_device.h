// eb_epoch_device.h — the index function of the keyed shuffle and the block folds of the epoch kernels (include/envbuild_epoch.h), each
// defined ONCE: the kernels of eb_epoch.hip call these and nothing else does the arithmetic.  splitmix64 is the sampler's
// (eb_env_device.h); nothing else of that header is used, and none of its code reaches the code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eb_env_device.h"

namespace eb {
namespace epoch {

constexpr int THREADS = 256;               // of all five kernels
constexpr int CHUNK = 4 * THREADS;         // elements of one chunk of the statistics: lane t takes t, t + 256, t + 512, t + 768
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

// the key of one permutation: base + epoch is what counts
__device__ __forceinline__ uint64_t epoch_key(uint64_t seed, uint64_t epoch, uint64_t base) {
    return splitmix64(seed + GOLDEN * (base + epoch));
}

// index(key, n, i) for i < n: six Feistel rounds over [0, 2^(2h)), walked until the value is back below n.  h = half the even bit width
// of n - 1 (the host's), mask = 2^h - 1.  2h <= 32, so every value fits 32 bits.
__device__ __forceinline__ uint32_t index(uint64_t key, uint32_t n, int h, uint32_t mask, uint32_t i) {
    uint32_t x = i;
    do {
        uint32_t L = x >> h, R = x & mask;
#pragma unroll
        for (int r = 0; r < 6; ++r) {
            const uint32_t F = (uint32_t)(splitmix64(key + GOLDEN * (((uint64_t)r << 32) | (uint64_t)R)) >> 32) & mask;
            const uint32_t next = L ^ F;
            L = R;
            R = next;
        }
        x = (L << h) | R;
    } while (x >= n);
    return x;
}

// the sum of the block's THREADS doubles in `red` (LDS), folded by halving in one fixed order; every lane returns it
__device__ __forceinline__ double fold(double* red, int t, double x) {
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    const double sum = red[0];
    __syncthreads();                        // red is free for the next fold
    return sum;
}

// the same halving with the larger of two: no NaN enters (the callers select from 0)
__device__ __forceinline__ double fold_max(double* red, int t, double x) {
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t + w] > red[t] ? red[t + w] : red[t];
        __syncthreads();
    }
    const double top = red[0];
    __syncthreads();
    return top;
}

__device__ __forceinline__ bool finite(float x) { return fabsf(x) <= 3.402823466e+38f; }     // false for a NaN and for +-inf

}  // namespace epoch
}  // namespace eb
