// eb_offpolicy_device.h — the run copy, the row gather, the keyed index, the NaN-carrying minimum, the temperature and the block fold of
// the off-policy kernels (include/envbuild_offpolicy.h), each defined ONCE: the kernels of eb_offpolicy.hip call these and nothing else
// does the arithmetic.  splitmix64 is the sampler's (eb_env_device.h) and exp_det the networks' (eb_mlp_device.h); nothing else of those
// headers is used, and none of their other code reaches the code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eb_env_device.h"
#include "eb_mlp_device.h"

namespace eb {
namespace offp {

constexpr int THREADS = 256;               // of all eight kernels
constexpr int ROWS = 32;                   // rows of one block of the push, sample, pack and action-grad kernels
constexpr int ALPHA_BLOCKS = 64;           // of sac_actor_kernel with the temperature gradient
constexpr int POLYAK_CHUNK = 4 * THREADS;  // elements of one block and pass of polyak_kernel
constexpr uint64_t GOLDEN = 0x9E3779B97F4A7C15ull;

__device__ __forceinline__ bool both16(const void* a, const void* b) { return ((((uintptr_t)a) | ((uintptr_t)b)) & 15) == 0; }

// dst[0 .. n) = src[0 .. n), n floats in ONE contiguous run on both sides, by the block's THREADS lanes: consecutive lanes on consecutive
// elements.  Both runs 16-byte aligned (uniform over the block): n / 4 float4s and the n % 4 floats behind them as dwords; otherwise
// everything goes as dwords.
__device__ __forceinline__ void copy_run(float* __restrict__ dst, const float* __restrict__ src, int n, int t) {
    int done = 0;
    if (both16(dst, src)) {
        const int quads = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(dst);
        for (int q = t; q < quads; q += THREADS) d4[q] = s4[q];
        done = quads << 2;
    }
    for (int e = done + t; e < n; e += THREADS) dst[e] = src[e];
}

// the block's `rows` source rows (rows [first, first + len1) of src go to ring slot slot0 on, the rest to slot 0 on), `width` floats each
__device__ __forceinline__ void copy_rows_to_ring(float* ring, const float* src, long long slot0, int len1, int rows, int width, int t) {
    copy_run(ring + slot0 * width, src, len1 * width, t);
    if (len1 < rows) copy_run(ring, src + (long long)len1 * width, (rows - len1) * width, t);
}

// dst [rows, wa + wb] (one contiguous run) = [a[from_row[r], :wa] | b[from_row[r], :wb]]; a row with from < 0 is written as quiet NaNs.
// Consecutive lanes on consecutive destination floats, THREADS per pass; a lane's (row, column) moves from pass to pass by THREADS / width
// and THREADS % width: one division per output.  TWO false: a alone (wb is 0 and b is not read).
template <bool TWO>
__device__ __forceinline__ void gather_rows(float* __restrict__ dst, const float* __restrict__ a, int wa, const float* __restrict__ b,
                                            int wb, const int* from_row, int rows, int t) {
    const float quiet_nan = __int_as_float(0x7FC00000);
    const int width = TWO ? wa + wb : wa, total = rows * width;
    const int rows_per_pass = THREADS / width, rest_per_pass = THREADS - rows_per_pass * width;
    int r = t / width, c = t - r * width;
    for (int e = t; e < total; e += THREADS) {
        const int from = from_row[r];
        float x = quiet_nan;
        if (from >= 0) {
            if (!TWO || c < wa) x = a[(size_t)from * (size_t)wa + c];
            else x = b[(size_t)from * (size_t)wb + (c - wa)];
        }
        dst[e] = x;
        r += rows_per_pass;
        c += rest_per_pass;
        if (c >= width) {
            c -= width;
            ++r;
        }
    }
}

// the key of one draw: base + draw is what counts
__device__ __forceinline__ uint64_t draw_key(uint64_t seed, uint64_t draw, uint64_t base) { return splitmix64(seed + GOLDEN * (base + draw)); }

// the word of row r under a key: j(r) = mulhi64(word, f) in [0, f) is the high half of the 128-bit product, (uint32_t)word the row's noise id
__device__ __forceinline__ uint64_t draw_word(uint64_t key, uint64_t r) { return splitmix64(key + GOLDEN * r); }

// the smaller of two as selects; a NaN in either travels
__device__ __forceinline__ float min_nan(float a, float b) {
    float m = b < a ? b : a;
    m = b != b ? b : m;
    return m;
}

__device__ __forceinline__ float alpha_of(const float* log_alpha, float alpha) { return log_alpha ? mlp::exp_det(*log_alpha) : alpha; }

// the sum of the block's THREADS doubles in `red` (LDS), folded by halving in one fixed order; every lane returns it
__device__ __forceinline__ double fold(double* red, int t, double x) {
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t] + red[t + w];
        __syncthreads();
    }
    return red[0];
}

}  // namespace offp
}  // namespace eb
