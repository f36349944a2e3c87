// eb_policy_rollout_grad_device.h — what policy_rollout_grad_kernel (eb_policy_rollout_grad.hip) restates of eb_policy_grad.hip's
// device code: the deterministic activations with their derivatives, mlp_kernel's layer chain on v_mfma_f32_32x32x2_f32, and the two
// epilogues that leave x_l / d_l in LDS and in the workspace.  The text is that file's, under other names: eb_policy_grad.hip's
// machine code does not move when this kernel changes, and the two files' bits agree because their text does
// (tests/test_gpu_policy_rollout_grad.py holds them to each other).
#pragma once
#include "eb_policy_grad.h"

namespace eb {
namespace prg {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

namespace act {

EB_DEV float exp_det(float x0) {
    const float x = x0 > 88.0f ? 88.0f : (x0 < -87.0f ? -87.0f : x0);   // NaN falls through both compares
    const float fx = __builtin_rintf(x * 1.44269504088896341f);
    float r = __builtin_fmaf(-fx, 0.693359375f, x);
    r = __builtin_fmaf(-fx, -2.12194440e-4f, r);
    const float z = r * r;
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, z, r) + 1.0f;
    const int n = (x0 == x0) ? (int)fx : 0;                              // -126 .. 127
    const float v = y * __builtin_bit_cast(float, (unsigned)(n + 127) << 23);
    return (x0 == x0) ? v : x0;
}

EB_DEV float tanh_det(float x) {
    const float ax = __builtin_fabsf(x);
    const float s = exp_det(ax + ax);
    const float t = 1.0f - 2.0f / (s + 1.0f);
    const float big = x < 0.0f ? -t : t;
    const float z = x * x;
    float p = -5.70498872745e-3f;
    p = __builtin_fmaf(p, z, 2.06390887954e-2f);
    p = __builtin_fmaf(p, z, -5.37397155531e-2f);
    p = __builtin_fmaf(p, z, 1.33314422036e-1f);
    p = __builtin_fmaf(p, z, -3.33332819422e-1f);
    const float small = __builtin_fmaf(p * z, x, x);
    const float sat = x > 0.0f ? 1.0f : -1.0f;
    return ax > 44.0f ? sat : (ax >= 0.625f ? big : small);              // NaN: both compares false -> small = NaN
}

EB_DEV float elu_det(float x0) {
    const float x = x0 < -87.0f ? -87.0f : x0;
    const float fx = __builtin_rintf(x * 1.44269504088896341f);
    float r = __builtin_fmaf(-fx, 0.693359375f, x);
    r = __builtin_fmaf(-fx, -2.12194440e-4f, r);
    const float z = r * r;
    float p = 1.9875691500e-4f;
    p = __builtin_fmaf(p, r, 1.3981999507e-3f);
    p = __builtin_fmaf(p, r, 8.3334519073e-3f);
    p = __builtin_fmaf(p, r, 4.1665795894e-2f);
    p = __builtin_fmaf(p, r, 1.6666665459e-1f);
    p = __builtin_fmaf(p, r, 5.0000001201e-1f);
    const float y = __builtin_fmaf(p, z, r) + 1.0f;
    const float v = __builtin_amdgcn_ldexpf(y, (int)fx);
    return x0 > 0.0f ? x0 : v - 1.0f;
}

template <int ACT>
EB_DEV float activate(float x) {
    if (ACT == MLP_ACT_RELU) return x > 0.0f ? x : 0.0f;
    if (ACT == MLP_ACT_ELU) return elu_det(x);
    if (ACT == MLP_ACT_TANH) return tanh_det(x);
    return x;
}
EB_DEV float activate_rt(int act, float x) {
    switch (act) {
        case MLP_ACT_RELU: return activate<MLP_ACT_RELU>(x);
        case MLP_ACT_ELU: return activate<MLP_ACT_ELU>(x);
        case MLP_ACT_TANH: return activate<MLP_ACT_TANH>(x);
        default: return x;
    }
}

// the derivative of an activation from its OUTPUT y, one fp32 operation each (include/envbuild_mlp_grad.h)
template <int ACT>
EB_DEV float derivative(float y) {
    if (ACT == MLP_ACT_RELU) return y > 0.0f ? 1.0f : 0.0f;
    if (ACT == MLP_ACT_ELU) return y > 0.0f ? 1.0f : y + 1.0f;
    if (ACT == MLP_ACT_TANH) return 1.0f - y * y;
    return 1.0f;
}
EB_DEV float derivative_rt(int act, float y) {
    switch (act) {
        case MLP_ACT_RELU: return derivative<MLP_ACT_RELU>(y);
        case MLP_ACT_ELU: return derivative<MLP_ACT_ELU>(y);
        case MLP_ACT_TANH: return derivative<MLP_ACT_TANH>(y);
        default: return 1.0f;
    }
}

}  // namespace act

// eb_policy_grad.hip's grad_layer_chain, restated: one layer's k-loop for the RT x CT tiles of a wave.  a_row: LDS address of
// A[row tile rt0][i][h][0]; wp: packed weights (pack_weights); steps = k_pad / 8.  Fragments are fetched two steps ahead into one of
// three register sets; the loop is unrolled by three so that the sets rotate by name.
template <int RT, int CT>
EB_DEV void layer_chain(const float* a_row, int row_tile_stride, const f32x4* __restrict__ wp, int steps, int ct0, int lane,
                             f32x16 (&acc)[RT][CT]) {
    const f32x4* bsrc[CT];
#pragma unroll
    for (int c = 0; c < CT; ++c) bsrc[c] = wp + (size_t)(ct0 + c) * steps * 64 + lane;
    f32x4 bq[3][CT], aq[3][RT];
    auto fetch = [&](int set, int s) {
        const int sc = s < steps ? s : steps - 1;
#pragma unroll
        for (int c = 0; c < CT; ++c) bq[set][c] = bsrc[c][(size_t)sc * 64];
#pragma unroll
        for (int r = 0; r < RT; ++r) aq[set][r] = *reinterpret_cast<const f32x4*>(a_row + r * row_tile_stride + sc * 4);
    };
    auto run = [&](int set) {
#pragma unroll
        for (int q = 0; q < 4; ++q)                                                          // k pairs in order
#pragma unroll
            for (int r = 0; r < RT; ++r)
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[r][c] = __builtin_amdgcn_mfma_f32_32x32x2f32(aq[set][r][q], bq[set][c][q], acc[r][c], 0, 0, 0);
    };
#define EB_STEP(FSET, FS, RSET)                   \
    fetch(FSET, FS);                              \
    __builtin_amdgcn_sched_barrier(0);            \
    run(RSET);                                    \
    __builtin_amdgcn_sched_barrier(0)
    fetch(0, 0);
    fetch(1, 1);
    __builtin_amdgcn_sched_barrier(0);
    int s = 0;
    for (; s + 3 <= steps; s += 3) {
        EB_STEP(2, s + 2, 0);
        EB_STEP(0, s + 3, 1);
        EB_STEP(1, s + 4, 2);
    }
    if (s < steps) { EB_STEP(2, s + 2, 0); }
    if (s + 1 < steps) run(1);
#undef EB_STEP
}

// eb_policy.hip's store_hidden, restated, with the copy the backward needs: a layer's outputs through the activation into the LDS
// activation buffer AND into the workspace (xg: row 0 of this block, `units` floats per row).
template <int RT, int CT, int ACT>
EB_DEV void store_hidden(float* lds, int RS, int HS, int rt0, int ct0, int i, int h, const f32x16 (&acc)[RT][CT], float* xg, int units) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = (ct0 + c) * 32 + i;
            float* dst = lds + (col & 1) * HS + (col >> 1);
            const int lane_off = 4 * h * units + col;                   // the lane's part of the address; the rest is wave-uniform
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int urow = (rt0 + r) * 32 + (v & 3) + 8 * (v >> 2);
                const float y = act::activate<ACT>(acc[r][c][v]);
                dst[(urow + 4 * h) * RS] = y;
                (xg + (size_t)urow * units)[lane_off] = y;
            }
        }
}

// The backward epilogue of a hidden layer: cotangent of the layer's outputs (the accumulators) times the derivative from the outputs
// the same lane stored on the way forward -> the cotangent of its pre-activations, into LDS (the next product's A operand) and the
// workspace (mlp_wgrad_kernel's B operand).
template <int RT, int CT, int ACT>
EB_DEV void store_delta(float* lds, int RS, int HS, int rt0, int ct0, int i, int h, const f32x16 (&acc)[RT][CT], const float* xg,
                             float* dg, int units) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = (ct0 + c) * 32 + i;
            float* dst = lds + (col & 1) * HS + (col >> 1);
            const int lane_off = 4 * h * units + col;                   // the lane's part of the address; the rest is wave-uniform
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int urow = (rt0 + r) * 32 + (v & 3) + 8 * (v >> 2);
                const float d = acc[r][c][v] * act::derivative<ACT>((xg + (size_t)urow * units)[lane_off]);
                dst[(urow + 4 * h) * RS] = d;
                (dg + (size_t)urow * units)[lane_off] = d;
            }
            __builtin_amdgcn_sched_barrier(0);                           // one tile's sixteen loads in flight, not every tile's
        }
}

}  // namespace prg
}  // namespace eb
