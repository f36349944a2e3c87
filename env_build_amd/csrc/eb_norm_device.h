// eb_norm_device.h — the arithmetic of the normalisation kernels (include/envbuild_norm.h), each piece defined ONCE: the kernels of
// eb_norm.hip call these and nothing else does the arithmetic.  No other library's header is included.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace eb {
namespace norm {

constexpr int THREADS = 256;               // of all three kernels
constexpr int ROWS = 32;                   // rows of one run: what a block stages (partial) or normalises (apply) at a time
constexpr int MAX_DIM = 256;               // EB_NORM_MAX_DIM
constexpr int FOLD_DEPTH = 32;             // loads in flight per lane while the fold kernel fetches a chunk of partials
constexpr int FOLD_CHUNK = FOLD_DEPTH * THREADS;   // doubles of one chunk (64 KiB of LDS): at least 15 whole blocks' partials at D = 256

// the row groups of the partial kernel at width D: lane g * D + d, g < groups(D), owns column d
__host__ __device__ __forceinline__ int groups(int D) { return THREADS / D < ROWS ? THREADS / D : ROWS; }

// tile[0 .. n) = src[0 .. n), n floats in ONE contiguous run of global memory into LDS, by the block's THREADS lanes: consecutive lanes on
// consecutive elements.  wide (uniform over the launch: every run starts 16-byte aligned) moves n / 4 float4s and the n % 4 floats
// behind them as dwords; otherwise everything goes as dwords.  tile is 16-byte aligned.
__device__ __forceinline__ void stage_run(float* tile, const float* __restrict__ src, int n, bool wide, int t) {
    int done = 0;
    if (wide) {
        const int quads = n >> 2;
        const float4* s4 = reinterpret_cast<const float4*>(src);
        float4* d4 = reinterpret_cast<float4*>(tile);
        for (int q = t; q < quads; q += THREADS) d4[q] = s4[q];
        done = quads << 2;
    }
    for (int e = done + t; e < n; e += THREADS) tile[e] = src[e];
}

// s1[g * D + d] and s2[g * D + d], g < G, folded over g by halving in one fixed order: s[g] += s[g + w] for w = P / 2 .. 1, P the power
// of two >= G, where g + w < G.  Lane (g, d) holds the result of column d when g == 0.  Every lane of the block calls this.
__device__ __forceinline__ void fold_groups(double* s1, double* s2, int g, int d, int G, int D, bool mine) {
    int P = 1;
    while (P < G) P <<= 1;
    for (int w = P >> 1; w > 0; w >>= 1) {
        __syncthreads();
        if (mine && g < w && g + w < G) {
            s1[g * D + d] = s1[g * D + d] + s1[(g + w) * D + d];
            s2[g * D + d] = s2[g * D + d] + s2[(g + w) * D + d];
        }
    }
    __syncthreads();
}

// the merge of one column: the batch's shifted sums S1, S2 over n rows into (mean, var) with the count before; -> the new count
__device__ __forceinline__ double merge(double S1, double S2, double K, double N, double count, double& mean, double& var) {
    const double a = S1 / N;
    const double bm = K + a;
    double bv = S2 / N - a * a;
    bv = (bv < 0.0) ? 0.0 : bv;                                  // a NaN travels
    const double delta = bm - mean;
    const double tot = count + N;
    const double new_mean = mean + (delta * N) / tot;
    const double M2 = (var * count + bv * N) + (((delta * delta) * count) * N) / tot;
    mean = new_mean;
    var = M2 / tot;
    return tot;
}

__device__ __forceinline__ float den_of(double var, float eps) { return sqrtf((float)var + eps); }

__device__ __forceinline__ float clip(float v, float c) {
    v = (v < -c) ? -c : v;                                       // selects: a NaN travels
    v = (v > c) ? c : v;
    return v;
}

__device__ __forceinline__ float normalise(float x, float mean, float den, float c) { return clip((x - mean) / den, c); }

}  // namespace norm
}  // namespace eb
