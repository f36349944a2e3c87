// eb_per_device.h — the tree's geometry, a node's sum, the sequential scan of a node's children and the priority's validity and clamp of
// the prioritised-replay kernels (include/envbuild_per.h), each defined ONCE: the kernels of eb_per.hip call these and nothing else does
// the arithmetic.  The keyed word is the replay sampler's (eb_offpolicy_device.h: draw_key, draw_word), exp_det the networks'
// (eb_mlp_device.h) and log_det the stochastic head's (eb_policy_sample_device.h); nothing else of those headers is used, and none of
// their other code reaches the code object.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "eb_offpolicy_device.h"
#include "eb_policy_sample_device.h"

namespace eb {
namespace per {

constexpr int THREADS = 256;        // of all nine kernels
constexpr int RADIX = 32;           // children of a node
constexpr int MAX_LEVELS = 7;       // 32^7 >= 2^31
constexpr int SMALL_NODES = 1024;   // a level of at most this many nodes is a small one
constexpr int TOP_DOUBLES = 1 + RADIX + SMALL_NODES;   // what the small levels hold at most
constexpr int MIN_BLOCKS = 64;      // of per_sample_kernel
constexpr float PRIO_MIN = 9.094947017729282e-13f;     // 2^-40
constexpr float PRIO_MAX = 1099511627776.0f;           // 2^40

// n[0] = C (the leaves); level k = 1 .. levels has n[k] nodes at tree + off[k]; the levels first_small .. levels are the small ones
struct Geometry {
    int levels, first_small;
    int n[MAX_LEVELS + 1];
    int off[MAX_LEVELS + 1];
    int doubles;
};

__host__ __device__ inline Geometry geometry(int capacity) {
    Geometry G{};
    G.n[0] = capacity;
    int k = 0, at = 0;
    do {
        ++k;
        G.n[k] = (int)(((long long)G.n[k - 1] + RADIX - 1) / RADIX);
        G.off[k] = at;
        at += G.n[k];
    } while (G.n[k] > 1);
    G.levels = k;
    G.doubles = at;
    G.first_small = k;
    while (G.first_small > 1 && G.n[G.first_small - 1] <= SMALL_NODES) --G.first_small;
    return G;
}

// node i of level k recomputed from its existing children, ascending from 0.0, one double addition per child
__device__ __forceinline__ double node_sum(const Geometry& G, const float* prio, const double* tree, int k, long long i) {
    const long long first = i * RADIX;
    const long long rest = (long long)G.n[k - 1] - first;
    const int cnt = rest < RADIX ? (int)rest : RADIX;
    double s = 0.0;
    if (k == 1) {
        const float* ch = prio + first;
#pragma unroll
        for (int c = 0; c < RADIX; ++c) {
            const double x = c < cnt ? (double)ch[c] : 0.0;
            if (c < cnt) s = s + x;
        }
    } else {
        const double* ch = tree + G.off[k - 1] + first;
#pragma unroll
        for (int c = 0; c < RADIX; ++c) {
            const double x = c < cnt ? ch[c] : 0.0;
            if (c < cnt) s = s + x;
        }
    }
    return s;
}

// the descent's step at one node: the sequential ascending prefix over the cnt existing children ch[0 .. cnt) -> the chosen child (-1:
// no child is positive) and the residual u.  The children are loaded together, guarded, before the scan.
template <typename T>
__device__ __forceinline__ int scan_children(const T* ch, int cnt, double& u) {
    double s[RADIX];
#pragma unroll
    for (int c = 0; c < RADIX; ++c) s[c] = c < cnt ? (double)ch[c] : 0.0;
    double acc = 0.0, base = 0.0;
    int chosen = -1, last = -1;
#pragma unroll
    for (int c = 0; c < RADIX; ++c) {
        const double nxt = acc + s[c];
        const bool hit = chosen < 0 && c < cnt && u < nxt;
        chosen = hit ? c : chosen;
        base = hit ? acc : base;
        last = s[c] > 0.0 ? c : last;
        acc = nxt;
    }
    if (chosen >= 0) {
        u = u - base;
    } else {
        chosen = last;
        u = 0.0;
    }
    return chosen;
}

__device__ __forceinline__ bool valid_value(float v) { return v > 0.0f && v < __builtin_inff(); }   // a NaN fails both
__device__ __forceinline__ bool valid_row(int j, float v, int capacity) { return j >= 0 && j < capacity && valid_value(v); }
__device__ __forceinline__ float clamp_prio(float v) {
    const float lo = v < PRIO_MIN ? PRIO_MIN : v;
    return lo > PRIO_MAX ? PRIO_MAX : lo;
}

// the minimum of the block's THREADS floats, folded by halving; every lane returns it (a minimum does not depend on the order)
__device__ __forceinline__ float fold_min(float* red, int t, float x) {
    red[t] = x;
    __syncthreads();
#pragma unroll
    for (int w = THREADS / 2; w > 0; w >>= 1) {
        if (t < w) red[t] = red[t + w] < red[t] ? red[t + w] : red[t];
        __syncthreads();
    }
    return red[0];
}

}  // namespace per
}  // namespace eb
