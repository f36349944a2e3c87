/*
 * envbuild_mlp_f16.h — C-ABI of the policy network's inference precision: an opt-in evaluation with IEEE binary16 operands on the
 * matrix cores (csrc/eb_policy_f16.hip, v_mfma_f32_32x32x16_f16 / v_mfma_f32_16x16x32_f16).
 *
 * A header of its own next to envbuild.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle of
 * envbuild.h has none of them), EB_ABI_VERSION is untouched, and a binding looks them up on demand.  Conventions (return codes,
 * eb_last_error, device pointers, `stream`) are those of envbuild.h.
 *
 * The default precision of every handle is EB_MLP_PRECISION_F32: the bit-exact fp32 chain envbuild.h states, reproduced by the CPU
 * oracle.  Nothing about it changes.  EB_MLP_PRECISION_F16 trades that reproducibility for matrix-core time: eb_mlp_forward,
 * eb_policy_run_batch and eb_shield_is_safe keep their signatures and evaluate the handle's network as stated below.  The result
 * cannot be reproduced bit for bit on the CPU (the order of a sum is the kernel's own), and shield flags are thresholds: switch
 * where the throughput matters and the policy's actions are not compared bit for bit with another implementation's.
 *
 * The arithmetic of a handle whose precision is EB_MLP_PRECISION_F16 (f16(.) is IEEE round-to-nearest-even to binary16, overflow to
 * +-inf, subnormal results kept):
 *   input        x0[k] = f16(obs[k] * scale[k]); the multiply is one fp32 multiply and happens only when a scale is set;
 *   weights      W16 = f16(W), converted on the host when eb_mlp_set_layer is called.  A layer's fp32 packing and its binary16 packing
 *                are both kept from then on: switching precision flips a flag and never needs the weights again.  Biases stay fp32;
 *   every layer  pre[j] = b[j] + sum over k of x[k] * W16[k][j].  The products are exact in fp32 (11 + 11 significand bits); the sum is
 *                in fp32, in the order the matrix instruction and the kernel's k-loop give it.  That order is the kernel's own and is
 *                NOT part of the contract: a restatement agrees to the rounding of an fp32 sum, not bit for bit — except where every
 *                partial sum is exact, where every order gives the same bits;
 *   hidden layer x_next[j] = f16(act(pre[j])), act being envbuild.h's deterministic fp32 elu / tanh / relu / identity, applied in fp32;
 *   output layer out[j] = act_out(pre[j]), stored as fp32; eb_policy_run_batch's head (action_range * tanh(mean)) is unchanged;
 *   padding      of k (to 16) and of the width (to 64 / 128 / 256 / 512) is zeros meeting zeros: exact no-ops.  A padded unit is held
 *                at zero whatever its sum gives, so a row with inf / NaN inputs has the non-finite pattern of the unpadded network;
 *   subnormals   binary16 subnormal operands (|x| < 2^-14) take part in the products with their value: neither the conversions nor
 *                the matrix instruction flush them (measured on gfx950: 2^-24 * 2^10 accumulates as 2^-14);
 *   rows         a row's bits depend on that row and the handle only — not on the row's position, its neighbours or n — and a launch
 *                repeats its bits.  No atomics.
 * The Python package restates this contract in NumPy: env_build_amd.policy.mlp_f16_reference.
 */
#ifndef ENVBUILD_MLP_F16_H
#define ENVBUILD_MLP_F16_H

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_MLP_F16_ABI_VERSION 1

#define EB_MLP_PRECISION_F32 0
#define EB_MLP_PRECISION_F16 1

int eb_mlp_f16_abi_version(void);

/* The precision eb_mlp_forward, eb_policy_run_batch and eb_shield_is_safe evaluate this handle with from the next call on.  Any time
 * after eb_mlp_create, before or after eb_mlp_set_layer / eb_mlp_set_obs_scale; work already enqueued is not affected.
 * EB_EINVAL: NULL handle, or a value that is neither EB_MLP_PRECISION_F32 nor EB_MLP_PRECISION_F16 (the handle keeps its precision). */
int eb_mlp_set_precision(eb_mlp m, int32_t precision);

/* The handle's precision.  EB_EINVAL: NULL handle or NULL precision. */
int eb_mlp_get_precision(eb_mlp m, int32_t* precision);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_MLP_F16_H */
