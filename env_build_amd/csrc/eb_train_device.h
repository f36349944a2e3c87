// eb_train_device.h — the row of the value loss and the element of the Adam update (include/envbuild_train.h), each defined ONCE: the
// kernels of eb_train.hip call these and nothing else does the arithmetic.  Every operation below is one fp32 rounding
// (-ffp-contract=off); every choice is a select on a comparison, so a NaN makes them false and travels.
#pragma once
#include <hip/hip_runtime.h>

namespace eb {
namespace train {

constexpr int THREADS = 256;               // of all three kernels
constexpr int CHUNK = 4 * THREADS;         // elements of one chunk of a segment: lane t takes t, t + 256, t + 512, t + 768

// the value loss of one row: v, ret and v_old (read only with `clipped`) -> loss (unscaled) and g (scaled)
__device__ __forceinline__ void value_loss_row(float v, float ret, float v_old, bool clipped, float c, float scale, float& loss, float& g) {
    const float e = v - ret;
    const float l1 = e * e;
    if (!clipped) {                         // uniform over the launch
        loss = 0.5f * l1;
        g = scale * e;
        return;
    }
    const float dv = v - v_old;
    const float cl = dv < -c ? -c : (dv > c ? c : dv);
    const float vc = v_old + cl;
    const float e2 = vc - ret;
    const float l2 = e2 * e2;
    const bool inside = dv >= -c && dv <= c;
    const bool second = l2 > l1;
    loss = 0.5f * (second ? l2 : l1);
    g = scale * (second ? (inside ? e2 : 0.0f) : e);
}

// what every element of one Adam step shares
struct AdamUniform {
    float coef;                             // the clipping coefficient, 1.0f when clipping is off
    float ss, sb;                           // (float)(lr / (1 - b1t)), (float)sqrt(1 - b2t)
    float b1, b2, o1, o2;                   // (float)beta1, (float)beta2, (float)(1 - beta1), (float)(1 - beta2)
    float eps, lwd;                         // (float)eps, (float)(lr * weight_decay)
    int decay;                              // weight_decay != 0
};

// one element: p, m and v updated in place from the gradient g
__device__ __forceinline__ void adam_element(const AdamUniform& U, float g, float& p, float& m, float& v) {
    g = g * U.coef;
    if (U.decay) p = p - U.lwd * p;
    m = U.b1 * m + U.o1 * g;
    v = U.b2 * v + (U.o2 * g) * g;
    const float den = sqrtf(v) / U.sb + U.eps;
    p = p - U.ss * (m / den);
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

}  // namespace train
}  // namespace eb
