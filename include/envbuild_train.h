/*
 * envbuild_train.h — C-ABI of the arithmetic a PPO minibatch needs between the entries of envbuild_ppo.h and envbuild_mlp_grad.h: the
 * (clipped) value loss with its gradient in ONE launch (eb_value_loss), and Adam / AdamW with global-norm gradient clipping whose step
 * count and bias-correction powers live on the DEVICE (eb_adam_step, always exactly TWO launches): csrc/eb_train.hip.  With them one
 * minibatch is a fixed chain of library launches that can be captured once and replayed: a replayed graph takes the NEXT optimiser step.
 *
 * A LIBRARY OF ITS OWN.  These symbols are exported by env_build_amd/lib/libenvbuild_train.so ONLY: training-only code that an inference
 * deployment never loads.  libenvbuild_hip.so, EB_ABI_VERSION and every other family's version are untouched.  Return codes are
 * envbuild.h's (EB_OK, EB_EINVAL, EB_EDEVICE); the reason of a failure is in eb_train_last_error() — this library's own string, NOT
 * eb_last_error().  Nothing here synchronises, allocates or uses atomics.  Both working entries run on the current device.
 *
 * Both working entries take ONE struct.  Their stream is therefore a field, not a parameter, and the table of stream-taking prototypes
 * (tests/test_stream_census.py) does not count them: tests/test_gpu_train.py holds each of them to that table's obligations (a side
 * stream, capture, replay).  Every scalar and every pointer of a struct is read AT CALL TIME: under stream capture those values are baked
 * into the graph, and the device buffers they point to — the optimiser state included — are read at every replay.
 *
 * The value loss.  One lane per row; values is read, and g_values written, at element i * stride (the value network's [n, 1] output has
 * stride 1, a column of a wider head its width).  c = clip_v.  Every line below is one fp32 rounding (-ffp-contract=off) and every choice
 * a select, so that a NaN poisons its own row only:
 *
 *   e  = v - ret                      l1 = e * e
 *   with v_old:
 *     dv = v - v_old                  cl = dv < -c ? -c : (dv > c ? c : dv)
 *     vc = v_old + cl                 e2 = vc - ret                 l2 = e2 * e2
 *     inside = dv >= -c && dv <= c
 *     loss = 0.5f * (l2 > l1 ? l2 : l1)
 *     g    = scale * (l2 > l1 ? (inside ? e2 : 0.0f) : e)
 *   without v_old (NULL):
 *     loss = 0.5f * l1                g = scale * e
 *
 * loss is written unscaled.  g is autograd's gradient of  scale * sum(0.5 * torch.max((v - ret)^2, (v_old + (v - v_old).clamp(-c, c) -
 * ret)^2))  with respect to v: what eb_mlp_backward(head = 0) takes as g_out for the value network.  scale = vf_coef / n makes it the
 * value term of the PPO loss.  INSIDE the interval (dv == -c, dv == c and dv == 0 included) the clamp passes and vc = v_old + (v - v_old).
 * Where that difference is exact — |v| and |v_old| within a factor of two of each other, or v formed as v_old + step — vc == v and
 * l2 == l1: torch.max gives each argument half of the cotangent, both halves pass, and the full gradient scale * e is what the
 * unclipped branch returns.  Where v - v_old is a ROUNDED difference (v from the network, v_old stored, magnitudes further apart) vc
 * misses v by a unit in the last place, the squares differ, and either may be the larger: with l2 > l1 the row takes the clipped
 * branch with `inside` true and returns scale * e2, torch's gradient through the passing clamp.  Every arm of the two selects is
 * reached by ordinary data; none is dead code.
 * OUTSIDE the interval a tie l2 == l1 (e2 == -e: ret exactly halfway between v and the clamped value, or both squares rounded to the
 * same number) takes the unclipped branch, scale * e, where torch gives HALF of it: the one tie split otherwise than torch.  The tests
 * stay off it.  A NaN makes every comparison false, so the row takes the unclipped branch: with a NaN in v or ret its loss and g are NaN
 * and no other row's are; with a NaN in v_old alone they are the unclipped loss and gradient of that row (torch.max would give NaN).
 *
 * Adam.  The parameters are up to EB_TRAIN_MAX_SEGMENTS segments {params, grads, m, v, count}, held in the struct BY VALUE; segments are
 * views into larger tensors, so a pointer needs 4-byte alignment only.  state points to an eb_adam_state on the device (8-byte aligned);
 * a zero-filled state is a valid start.  partials points to EB_TRAIN_ADAM_PARTIALS doubles of device scratch (8-byte aligned), contents
 * undefined before and after.  Two calls that share a state or partials must be ordered by their streams.
 *
 * The order of the sum of squares is a pure function of the counts — the same on every stream, eagerly and under capture:
 *   segment s is cut into ceil(count_s / 1024) chunks of 1024 consecutive elements (the last one ragged); the chunks of all segments are
 *   numbered in segment order, C in all; P = min(C, EB_TRAIN_ADAM_PARTIALS).
 *   Block b < P of 256 lanes takes the chunks b, b + P, b + 2P, ... in ascending order; lane t adds, to a double that starts at +0.0,
 *   (double)g * (double)g of the elements t, t + 256, t + 512, t + 768 of each chunk in that order; the block's 256 doubles are folded
 *   by halving (x[t] += x[t + w] for w = 128, 64, ... 1) and x[0] is partial b.
 *   The partials 0 .. P-1 (the rest taken as +0.0) are folded by the same halving over 256 slots: `sum`.
 *
 * Launch 1 (adam_norm_kernel) writes the partials, and ONE lane of block 0 advances the state — nothing else in this launch reads it:
 *   was0 = step == 0;   step += 1;   b1t = (was0 ? 1.0 : b1t) * beta1;   b2t = (was0 ? 1.0 : b2t) * beta2        # doubles
 * Launch 2 (adam_update_kernel): every block folds the partials itself, then
 *   gnorm = (float)sqrt(sum)                                          # double square root, rounded once
 *   clipping on (max_grad_norm > 0 and not +inf):
 *     q = (float)max_grad_norm / (gnorm + 1e-6f)       coef = q > 1.0f ? 1.0f : q        # a NaN travels, as clip_grad_norm_'s does
 *   clipping off:  coef = 1.0f
 *   uniforms, formed in double and rounded once:
 *     ss = (float)(lr / (1.0 - b1t))   sb = (float)sqrt(1.0 - b2t)   o1 = (float)(1.0 - beta1)   o2 = (float)(1.0 - beta2)
 *     b1 = (float)beta1   b2 = (float)beta2   ep = (float)eps   lwd = (float)(lr * weight_decay)
 *   per element, one fp32 rounding per operation, `/` and sqrt IEEE-correct:
 *     g = g * coef
 *     weight_decay != 0:  p = p - lwd * p                             # decoupled (AdamW); 0 gives Adam
 *     m = b1 * m + o1 * g
 *     v = b2 * v + (o2 * g) * g
 *     den = sqrt(v) / sb + ep
 *     p = p - ss * (m / den)
 *   and block 0 stores gnorm and coef into the state, for logging.  grads is not written.
 * Launch 1 only writes step, b1t and b2t after reading them in one lane; launch 2 only reads them: no race inside a launch.  Because the
 * step and the powers live on the device, the host holds no counter and a replayed graph takes the next step.
 * With coef == 1.0f (the norm below max_grad_norm) the result is bit for bit that of clipping off.  A NaN gradient element makes gnorm,
 * coef and — with clipping on — every parameter NaN; an inf element makes gnorm inf, coef 0 and its own g NaN (inf * 0).
 *
 * n = 0 (a total count of 0) is a no-op that needs no pointer, launches nothing and leaves the state alone; a refusal names its entry in
 * eb_train_last_error and writes nothing; a NaN scalar is refused; repeated calls on equal inputs repeat their bits.
 * The Python package restates this contract in NumPy: env_build_amd.train.value_loss_reference and adam_reference.
 */
#ifndef ENVBUILD_TRAIN_H
#define ENVBUILD_TRAIN_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_TRAIN_ABI_VERSION 1
#define EB_TRAIN_MAX_SEGMENTS 32
#define EB_TRAIN_ADAM_PARTIALS 256

typedef struct eb_value_loss_args {
    int32_t n, stride;         /* n >= 0; stride >= 1: the element step of values and g_values */
    const float* values;       /* [n] at stride */
    const float* ret;          /* [n] */
    const float* v_old;        /* [n] or NULL: no clipping */
    float clip_v;              /* >= 0; NaN refused; not read when v_old is NULL */
    float scale;               /* the weight of a row's loss in the objective, vf_coef / n for PPO; NaN refused */
    float* loss;               /* [n] or NULL           unscaled */
    float* g_values;           /* [n] at stride, or NULL */
    void* stream;
} eb_value_loss_args;

typedef struct eb_adam_segment {
    float* params;             /* [count]  updated in place */
    const float* grads;        /* [count] */
    float* m;                  /* [count]  first moment, updated in place */
    float* v;                  /* [count]  second moment, updated in place */
    int64_t count;             /* 0 .. 2^31 - 1; with 0 the pointers are not read */
} eb_adam_segment;

typedef struct eb_adam_state {   /* 32 bytes on the DEVICE; all zero is a valid start */
    int64_t step;
    double b1t, b2t;           /* beta1^step, beta2^step by repeated multiplication */
    float gnorm, coef;         /* of the last step: the global gradient norm and the clipping coefficient */
} eb_adam_state;

typedef struct eb_adam_args {
    int32_t n_segments;        /* 0 .. EB_TRAIN_MAX_SEGMENTS */
    eb_adam_segment segments[EB_TRAIN_MAX_SEGMENTS];
    double lr;                 /* >= 0.  DOUBLES, what a Python trainer holds; NaN refused */
    double beta1, beta2;       /* in [0, 1) */
    double eps;                /* >= 0 */
    double weight_decay;       /* >= 0; decoupled; 0: Adam */
    double max_grad_norm;      /* <= 0 or +inf: no clipping */
    eb_adam_state* state;
    double* partials;          /* EB_TRAIN_ADAM_PARTIALS doubles of device scratch */
    void* stream;
} eb_adam_args;

int eb_train_abi_version(void);
const char* eb_train_last_error(void);

/* The value loss as stated above: one launch, one lane per row.
 * EB_EINVAL (nothing written): NULL args, n < 0, stride < 1, NULL values or ret with n > 0, scale NaN, and with v_old: clip_v NaN or
 * < 0. */
int eb_value_loss(const eb_value_loss_args* a);

/* One optimiser step as stated above: ALWAYS exactly TWO launches on a->stream (none with a total count of 0).
 * EB_EINVAL (nothing written): NULL args, n_segments outside 0 .. EB_TRAIN_MAX_SEGMENTS, a count < 0 or > 2^31 - 1, a NULL or not 4-byte
 * aligned params, grads, m or v of a segment with count > 0, NULL or not 8-byte aligned state or partials with a total count > 0, a NaN
 * scalar, lr, eps or weight_decay < 0, beta1 or beta2 outside [0, 1). */
int eb_adam_step(const eb_adam_args* a);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_TRAIN_H */
