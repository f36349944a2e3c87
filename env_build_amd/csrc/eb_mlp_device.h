// eb_mlp_device.h — the device code every policy-network kernel shares, written once: eb_policy.hip (fp32 forward), eb_policy_grad.hip
// (backward), eb_policy_rollout_grad.hip (closed-loop rollout with its parameter gradient) and, through eb_policy_f16_device.h,
// eb_policy_f16.hip and eb_policy_rollout.hip (binary16); eb_rollout_tape_sample.hip takes exp_det.  The deterministic activations
// and their derivatives, one hidden layer's k-loop on v_mfma_f32_32x32x2_f32 and the epilogues that leave a layer's outputs /
// cotangents in LDS and in the backward's workspace.  The policy family's numerical contract is this text: fp16 and fp32 agree on
// activation bits, the fused rollouts equal the loop of single calls bit for bit and the oracle's eb_expf / eb_tanhf match because
// there is one definition of each function.  Everything is EB_DEV (forced inline): a translation unit's machine code depends on what
// it calls, not on what else this header holds.
#pragma once
#include "eb_kernels.h"

namespace eb {
namespace mlp {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// ---- deterministic exp / tanh (Cephes scheme, explicit fma; oracle: eb_expf / eb_tanhf) ----
// Written without branches (selects): the epilogue applies them to 64 accumulator values per lane and layer.
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

// ELU = x > 0 ? x : exp_det(x) - 1, written for the epilogue (64 values per lane and layer): only x <= 0 reaches the
// exponential's result, so the upper clamp goes, the scaling by 2^n is one v_ldexp_f32 (exactly the multiplication by the
// bit-built power of two, denormal results included) and a NaN needs no select — it travels through the fma chain by
// itself (v_cvt_i32_f32 of NaN is 0).  Same bits as exp_det(x) - 1 for every x <= 0, so the oracle's eb_expf stays as it is.
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

// One layer's k-loop for the RT x CT tiles of a wave.  a_row: LDS address of A[row tile rt0][i][h][0];
// wp: this layer's packed weights; steps = k_pad / 8.  acc enters holding the bias.  Fragments are fetched two
// steps ahead into one of three register sets; the loop is unrolled by three so that the sets rotate by name
// (a register copy would make every step wait for the load it has just issued).
template <int RT, int CT>
EB_DEV void layer_chain(const float* a_row, int row_tile_stride, const f32x4* __restrict__ wp, int steps, int ct0,
                        int lane, f32x16 (&acc)[RT][CT]) {
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
    // the scheduling fences keep every fetch where it is written: two steps (32 MFMAs) ahead of its use
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

// A layer's outputs back into the LDS activation buffer (its layout: eb_policy.hip, at mlp_kernel), through the activation.
template <int RT, int CT, int ACT>
EB_DEV void store_hidden(float* lds, int RS, int HS, int rt0, int ct0, int i, int h, const f32x16 (&acc)[RT][CT]) {
#pragma unroll
    for (int r = 0; r < RT; ++r)
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            const int col = (ct0 + c) * 32 + i;
            float* dst = lds + (col & 1) * HS + (col >> 1);
#pragma unroll
            for (int v = 0; v < 16; ++v) {
                const int row = (rt0 + r) * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                dst[row * RS] = activate<ACT>(acc[r][c][v]);
            }
        }
}

// store_hidden with the copy the backward needs: a layer's outputs through the activation into the LDS activation buffer AND into
// the workspace (xg: row 0 of this block, `units` floats per row).
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
                const float y = activate<ACT>(acc[r][c][v]);
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
                const float d = acc[r][c][v] * derivative<ACT>((xg + (size_t)urow * units)[lane_off]);
                dst[(urow + 4 * h) * RS] = d;
                (dg + (size_t)urow * units)[lane_off] = d;
            }
            __builtin_amdgcn_sched_barrier(0);                           // one tile's sixteen loads in flight, not every tile's
        }
}

}  // namespace mlp
}  // namespace eb
