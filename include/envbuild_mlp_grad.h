/*
 * envbuild_mlp_grad.h — C-ABI of the policy network's backward: the gradient of eb_mlp_forward / eb_policy_run_batch with respect to
 * the observations and to every weight and bias, on the f32 matrix cores (csrc/eb_policy_grad.hip, v_mfma_f32_32x32x2_f32), and the
 * device-side weight update that lets a trainer keep the handle current without a host round trip.
 *
 * A header of its own next to envbuild.h: these symbols are exported by env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle of
 * envbuild.h has none of them), EB_ABI_VERSION is untouched, and a binding looks them up on demand.  Conventions (return codes,
 * eb_last_error, device pointers, `stream`) are those of envbuild.h.  Nothing here synchronises, allocates per call or uses atomics.
 *
 * Parameter layout.  `params` and `g_params` are flat DEVICE fp32 buffers of eb_mlp_param_count floats in Model.get_weights() order
 * and shape: kernel 0 [in, out] row-major, bias 0, kernel 1, bias 1, ...  They are unpadded.
 *
 * Supported handles.  The handle's precision is EB_MLP_PRECISION_F32, its padded hidden width is at most 256, and every layer has
 * been set (eb_mlp_set_layer for each, or one eb_mlp_set_params_device).  Anything else is refused and nothing is written: a handle
 * whose precision is EB_MLP_PRECISION_F16, or whose width pads to 512, with EB_EINVAL and the first unmet condition in eb_last_error
 * (what eb_mlp_grad_supported reports); a layer never set with EB_ESTATE.  The fp16 handle is refused on purpose: nobody should
 * receive the gradient of a function other than the one eb_mlp_forward evaluates on that handle.  (Switch to fp32, differentiate,
 * switch back: the switch is a flag.)
 *
 * The contract of eb_mlp_backward (act' is the derivative of the activation taken from the activation's OUTPUT y, one fp32 operation
 * each: relu y > 0 ? 1 : 0; elu y > 0 ? 1 : y + 1; tanh 1 - y * y; linear 1):
 *   forward      recomputed inside the call with the forward kernel's own chain: x_0 = obs * scale, pre_l = b_l + sum over k of
 *                x_{l-1}[k] * W_l[k][.] as fused multiply-adds in ascending k, x_l = act(pre_l).  `out` therefore equals
 *                eb_mlp_forward (head 0) / eb_policy_run_batch (head 1) bit for bit;
 *   head 0       g_out is [n, out_dim], the cotangent of eb_mlp_forward's output y: d_out = g_out * act_out'(y); `out` receives y;
 *   head 1       g_out is [n, out_dim / 2], the cotangent of eb_policy_run_batch's actions; `out` receives the actions.  On the mean
 *                columns d_out = (g_out * action_range) * (1 - t * t) * act_out'(mean) with t = tanh_det(mean); action_range <= 0
 *                means the mean itself, d_out = g_out * act_out'(mean).  The log-std columns get 0;
 *   backwards    d_{l-1} = (d_l * W_l^T) (.) act'(x_{l-1}),  g_obs = (d_1 * W_1^T) (.) scale,  dW_l = x_{l-1}^T * d_l,
 *                db_l = sum over the rows of d_l.  Products are fp32 and sums are fp32; the ORDER of each backward sum is the
 *                kernel's own and is NOT part of the contract: a restatement agrees to the rounding of an fp32 sum, and bit for bit
 *                where every partial sum is exact;
 *   repeats      the same call on the same handle and inputs repeats its bits;
 *   rows         a row's `out` and g_obs depend on that row and the handle only — not on its position, its neighbours or n;
 *   padding      padded units and padded inputs contribute exact zeros;
 *   n = 0        g_params (if given) is written as zeros and nothing else is touched;
 *   non-finite   inf and NaN travel through both chains as IEEE arithmetic carries them: a non-finite row poisons its own g_obs row
 *                and, through the sums over the rows, g_params (unless the activation absorbs it: relu maps NaN to 0, a saturated
 *                tanh has derivative 0).  Other rows' `out` and g_obs are unaffected.
 * The Python package restates this contract in NumPy: env_build_amd.policy_grad.mlp_backward_reference.
 */
#ifndef ENVBUILD_MLP_GRAD_H
#define ENVBUILD_MLP_GRAD_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_MLP_GRAD_ABI_VERSION 1

int eb_mlp_grad_abi_version(void);

/* ok = 1 when eb_mlp_backward accepts this handle as it stands, else 0 with the first unmet condition in eb_last_error.
 * EB_EINVAL: NULL handle or NULL ok. */
int eb_mlp_grad_supported(eb_mlp m, int32_t* ok);

/* Floats in `params` / `g_params`: the sum over the layers of k_real * cols_real + cols_real.  EB_EINVAL: NULL handle or NULL count. */
int eb_mlp_param_count(eb_mlp m, int64_t* count);

/* Fills every packing the handle keeps (fp32, binary16 — hardware round-to-nearest-even, subnormals kept —, the transposed one the
 * backward reads, the padded biases) from the flat device buffer, on `stream`, in one launch, with no host copy and no
 * synchronisation.  Afterwards the handle is indistinguishable from one filled by eb_mlp_set_layer with the same values, at either
 * precision, and every layer counts as set.  `params` must stay valid until the launch has run.  The update is ordered on `stream`
 * only: work that reads the handle on another stream is the caller's to order.  Any handle (any width, either precision).
 * EB_EINVAL: NULL handle or NULL params. */
int eb_mlp_set_params_device(eb_mlp m, const float* params, void* stream);

/* Bytes of workspace eb_mlp_backward needs for n rows on this handle (the recomputed activations, the cotangents and the partial
 * tiles of the parameter gradients).  0 for n = 0.  EB_EINVAL: NULL handle, NULL bytes, n < 0, or an unsupported handle. */
int eb_mlp_backward_workspace_bytes(eb_mlp m, int32_t n, size_t* bytes);

/* The contract above.  obs [n, obs_dim]; g_out by `head` (0: logits, 1: actions); workspace: DEVICE memory of at least
 * eb_mlp_backward_workspace_bytes(m, n) bytes, 16-byte aligned, contents undefined before and after; out, g_obs [n, obs_dim] and
 * g_params may each be NULL (that output is not computed).  A fixed number of launches on `stream`, independent of n.
 * EB_EINVAL (nothing written): NULL handle, unsupported handle, n < 0, head neither 0 nor 1, head 1 with an odd out_dim, NULL obs /
 * g_out / workspace with n > 0, workspace_bytes too small.  EB_ESTATE: a layer was never set. */
int eb_mlp_backward(eb_mlp m, int32_t n, const float* obs, const float* g_out, int32_t head, float action_range,
                    void* workspace, size_t workspace_bytes, float* out, float* g_obs, float* g_params, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_MLP_GRAD_H */
