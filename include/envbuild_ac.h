/*
 * envbuild_ac.h — C-ABI of the two row kernels a SHARED-TRUNK actor-critic needs: one network with W = 2 * act_dim + 1 outputs — the
 * policy's mean and log-std in columns 0 .. 2A-1, exactly as every other entry reads them, and the value in column 2A — instead of a
 * policy network and a value network over the same observations: csrc/eb_ac.hip.
 *
 *   eb_ac_loss     ONE launch   the PPO surrogate row on columns 0 .. 2A-1 and the value-loss row on column 2A of y [n, W], with
 *                               the WHOLE cotangent g_y [n, W]: what eb_mlp_backward(head = 0) takes for one backward of one network
 *   eb_ac_sample   ONE launch   the sampling row on columns 0 .. 2A-1, the dense logits [n, 2A] and the value column split off
 *
 * The network side needs nothing new: eb_mlp_forward and eb_mlp_backward(head = 0) take any out_dim <= 32.  What was missing is
 * everything that reads the policy's logits: eb_ppo_surrogate[_from_logits], eb_policy_sample[_from_logits],
 * eb_policy_logp_from_logits and g_logits assume a dense [n, 2 * act_dim] array.
 *
 * A LIBRARY OF ITS OWN.  These symbols are exported by env_build_amd/lib/libenvbuild_ac.so ONLY.  libenvbuild_hip.so,
 * libenvbuild_train.so, libenvbuild_epoch.so, libenvbuild_collect.so, libenvbuild_ctl.so, EB_ABI_VERSION and every other family's
 * version are untouched.  This header restates NO arithmetic: the surrogate row is envbuild_ppo.h's, the log-probability and its
 * reverse pass envbuild_policy_logp.h's, the sampling row envbuild_policy_sample.h's and the value-loss row envbuild_train.h's, line
 * by line, and the unit calls the same device functions (plogp::logp_row, plogp::logp_vjp_elem, mlp::exp_det, psample::sample_row,
 * train::value_loss_row).  Return codes are envbuild.h's (EB_OK, EB_EINVAL, EB_EDEVICE); the reason of a failure is in
 * eb_ac_last_error() — this library's own string.  Nothing here synchronises, allocates, copies or uses atomics.  Both entries run on
 * the current device.
 *
 * Both entries take ONE struct.  Their stream is therefore a field, not a parameter, and the table of stream-taking prototypes
 * (tests/test_stream_census.py) does not count them: tests/test_gpu_ac.py holds each of them to that table's obligations (a side
 * stream, capture, replay).  The census of struct-taking entries in the same file holds a fixed table of the twenty entries of the
 * other families; the two prototypes below are declared WITHOUT a parameter name, which its parser passes over, so that table stands as
 * it is, and tests/test_ac_host.py applies the census's own check (the capture test names the entry, a side stream, capture, replay)
 * to these two.  When the table takes them in, the parameter gets its name `a`; the ABI does not change.
 * Every scalar and every pointer of a struct is read AT CALL TIME: under stream capture those values are baked into the graph, and
 * the device buffers they point to — adv_norm's two floats included — are read at every replay.
 *
 * The layout.  y is [n, W] with W = 2 * act_dim + 1: what eb_mlp_forward wrote for the shared network, after the output activation.
 * act_dim lies in 1 .. 15, so W <= 31 (eb_mlp_backward's cotangent row is 32 floats wide).  W is odd: a row of y or g_y is aligned to
 * 4 bytes only, and every load and store here is a dword.
 *
 * eb_ac_loss (ac_loss_kernel, one lane per row).  With logits = y[:, :2A] and values = y[:, 2A]:
 *   logp, ratio, surr, ent, z_out and g_y[:, :2A]  are eb_ppo_surrogate_from_logits' logp, ratio, surr, ent, z_out and g_logits on a
 *                                                  dense copy of the logits with the same actions, logp_old, adv, adv_norm,
 *                                                  action_range, clip, ent_coef and scale, bit for bit
 *   vloss and g_y[:, 2A]                           are eb_value_loss' loss and g_values on (values = y + 2A, stride = W) with the same
 *                                                  ret, v_old, clip_v and scale = v_scale, bit for bit
 * g_y is the cotangent of y for  -scale * sum(surr) - scale * ent_coef * sum(ent) + v_scale * sum(vloss).  scale = 1 / n and v_scale =
 * vf_coef / n make it the PPO loss of a minibatch.  Every column of g_y is written.  v_old NULL: the unclipped value loss, clip_v is
 * not read.  A NaN in a row's inputs poisons that row only: the policy columns as envbuild_ppo.h says, the value column as
 * envbuild_train.h says.
 *
 * eb_ac_sample (ac_sample_kernel, one lane per row).  actions, logp and eps_out are eb_policy_sample_from_logits' on the dense copy of
 * the logits with the same eps, row_ids, seed, counter and action_range, bit for bit: the same (seed, counter, row id) noise.
 * logits_out [n, 2A] is that dense copy — dense, so that eb_policy_logp_from_logits and a rollout buffer take it as it is — and
 * values [n] is column 2A.  actions NULL means SPLIT ONLY: nothing is drawn, logp and eps_out are not written, and only logits_out and
 * values are.
 *
 * Rows are independent; n = 0 is a no-op that needs no pointer; a refusal names its entry in eb_ac_last_error, launches nothing and
 * writes nothing; repeated calls on equal inputs repeat their bits.
 * The Python package restates this contract in NumPy by composition: env_build_amd.ac.ac_loss_reference and ac_sample_reference.
 */
#ifndef ENVBUILD_AC_H
#define ENVBUILD_AC_H

#include <stddef.h>
#include <stdint.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_AC_ABI_VERSION 1
#define EB_AC_MAX_ACT_DIM 15

typedef struct eb_ac_loss_args {
    int32_t n;                 /* rows, >= 0 */
    int32_t act_dim;           /* 1 .. EB_AC_MAX_ACT_DIM; W = 2 * act_dim + 1 */
    const float* y;            /* [n, W] */
    const float* actions;      /* [n, act_dim] */
    const float* logp_old;     /* [n] */
    const float* adv;          /* [n] */
    const float* adv_norm;     /* [2] on the DEVICE: (mean, 1 / std), or NULL: adv is used as it is */
    const float* ret;          /* [n] */
    const float* v_old;        /* [n], or NULL: the unclipped value loss */
    float action_range;        /* > 0: squashed; <= 0: not; NaN refused */
    float clip;                /* >= 0; NaN refused */
    float ent_coef;            /* NaN refused */
    float scale;               /* the weight of a row's surrogate and entropy, 1 / n for a mean; NaN refused */
    float clip_v;              /* >= 0 and not NaN with v_old; not read without */
    float v_scale;             /* the weight of a row's value loss, vf_coef / n; NaN refused */
    float* logp;               /* [n]            required */
    float* ratio;              /* [n] or NULL */
    float* surr;               /* [n] or NULL    unscaled */
    float* ent;                /* [n] or NULL    unscaled */
    float* vloss;              /* [n] or NULL    unscaled */
    float* g_y;                /* [n, W] or NULL NULL: evaluation only */
    float* z_out;              /* [n, act_dim] or NULL */
    void* stream;
} eb_ac_loss_args;

typedef struct eb_ac_sample_args {
    int32_t n;                 /* rows, >= 0 */
    int32_t act_dim;           /* 1 .. EB_AC_MAX_ACT_DIM */
    const float* y;            /* [n, W] */
    const float* eps;          /* [n, act_dim], or NULL: drawn from (seed, counter, row id) */
    const int32_t* row_ids;    /* [n], or NULL: the row index */
    uint64_t seed;
    uint64_t counter;
    float action_range;        /* NaN refused */
    float* actions;            /* [n, act_dim], or NULL: split only */
    float* logits_out;         /* [n, 2 * act_dim] dense, or NULL */
    float* values;             /* [n] or NULL */
    float* logp;               /* [n] or NULL */
    float* eps_out;            /* [n, act_dim] or NULL */
    void* stream;
} eb_ac_sample_args;

int eb_ac_abi_version(void);
const char* eb_ac_last_error(void);

/* The loss rows as stated above: ALWAYS exactly ONE launch (none with n == 0).
 * EB_EINVAL (nothing launched): NULL args, n < 0, act_dim outside 1 .. 15, action_range, clip, ent_coef, scale or v_scale NaN,
 * clip < 0, clip_v < 0 or NaN with v_old, a pointer that is not 4-byte aligned, and with n > 0: NULL y, actions, logp_old, adv, ret
 * or logp. */
int eb_ac_loss(const eb_ac_loss_args*);

/* The sampling row and the split as stated above: ALWAYS exactly ONE launch (none with n == 0).
 * EB_EINVAL (nothing launched): NULL args, n < 0, act_dim outside 1 .. 15, action_range NaN, a pointer that is not 4-byte aligned,
 * and with n > 0: NULL y, or actions, logits_out and values all NULL (nothing to write). */
int eb_ac_sample(const eb_ac_sample_args*);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_AC_H */
