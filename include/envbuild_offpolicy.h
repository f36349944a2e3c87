/*
 * envbuild_offpolicy.h — C-ABI of OFF-POLICY TRAINING on the device: a replay ring and the memory-bound and elementwise work of a SAC
 * (or TD3 / DDPG) update between the network launches the other libraries already have — eb_replay_push, eb_replay_sample, eb_q_pack,
 * eb_sac_critic, eb_sac_actor, eb_q_action_grad, eb_polyak: csrc/eb_offpolicy.hip.
 *
 * A LIBRARY OF ITS OWN.  These symbols are exported by env_build_amd/lib/libenvbuild_offpolicy.so ONLY; the other seven libraries,
 * EB_ABI_VERSION and every other family's version are untouched.  Return codes are envbuild.h's (EB_OK, EB_EINVAL, EB_EDEVICE); the
 * reason of a failure is in eb_offpolicy_last_error() — this library's own string, NOT eb_last_error().  Nothing here synchronises,
 * allocates, copies or uses atomics.  The working entries run on the current device.
 *
 * Every working entry takes ONE struct.  Its stream is therefore a field, not a parameter, and the table of stream-taking prototypes
 * (tests/test_stream_census.py) does not count it; the prototypes are declared without a parameter name, as envbuild_norm.h's are, so
 * that the fixed table of the other families' struct-taking entries stays as it is: tests/test_offpolicy_host.py and
 * tests/test_gpu_offpolicy.py hold each entry to that table's obligations (a side stream, capture, replay).  Every scalar and every
 * pointer of a struct is read AT CALL TIME; the device words named below (*fill, *counter, *log_alpha) are read by the kernel, so at
 * every replay of a captured call.
 *
 * Common rules.  256-thread blocks, rows indexed in 64 bits, plain vector stores.  Every line of arithmetic below is ONE fp32 rounding
 * (the library is compiled with -ffp-contract=off); fmaf is the single-rounding fused multiply-add and is used only where written.  A
 * refusal (EB_EINVAL) names its entry in eb_offpolicy_last_error and launches and writes nothing: NULL args, a needed pointer that is
 * NULL or misaligned for its element (4 bytes for float and int32, 8 for the 8-byte words and doubles, none for uint8), a count outside
 * 0 .. 2^31 - 1, a rows x width product above 2^31 - 1, a NaN scalar.  A count of 0 (n, m, no segment with elements) returns EB_OK,
 * launches nothing and needs no pointer.  Repeated calls on equal inputs repeat their bits.  A row's outputs depend on that row only.
 *
 * THE RING.  Capacity C rows of caller-owned device arrays
 *   obs [C, D]   act [C, A]   rew [C]   next_obs [C, D]   nonterminal [C] (float)   fill: ONE 8-byte word, the number of valid rows, 0 .. C
 * with D = obs_dim in 1 .. EB_OFFPOLICY_MAX_OBS (4096) and A = act_dim in 1 .. EB_OFFPOLICY_MAX_ACT (16), C * (D + A) <= 2^31 - 1.
 *
 * eb_replay_push, ONE launch of ceil(n / 32) blocks (replay_push_kernel): n <= C transitions go to the slots (start + i) mod C, i = 0 ..
 * n - 1; start is a host scalar in 0 .. C - 1 (the cursor lives on the host: collection is issued eagerly).  Two optional parts over the
 * same n rows, at least one present:
 *   before   obs[slot] = prev_obs[i]      act[slot] = action[i]                           (prev_obs [n, D] and action [n, A]: both or none)
 *   after    what eb_env_step left behind: reward [n], obs_after [n, D] (under auto-reset the reset rows of finished envs), done_code [n]
 *            uint8, final_obs [n, D] or NULL.  With c = done_code[i]:
 *              next_obs[slot]    = (c != 0 && final_obs) ? final_obs[i] : obs_after[i]     a finished env's transition ends in its terminal
 *                                                                                          observation, never in the reset row
 *              rew[slot]         = reward[i]
 *              nonterminal[slot] = (c == 0 || (c == EB_DONE_TIME_LIMIT && final_obs)) ? 1.0f : 0.0f
 *            — eb_collect_record's rule: a time-limit truncation still bootstraps.  reward, obs_after and done_code: all or none;
 *            final_obs only with them.  With the after part ONE lane stores fill_after (a host scalar, 0 .. C) to *fill; the kernel does
 *            not read *fill, and a call without the after part does not write it.  Ordering is the stream's.
 * Block k takes the rows 32 k .. 32 k + 31.  Their slots are one contiguous piece of the ring, or two when the piece crosses slot C - 1
 * (n <= C: at most once per block): each piece is copied as ONE run, consecutive lanes on consecutive floats, as 16-byte accesses when
 * the piece's source and destination both start 16-byte aligned (the floats behind the last whole quad as dwords) and as dwords
 * otherwise.  next_obs takes obs_after's runs that way; then, behind a barrier, each of the block's four waves walks the rows wave, wave
 * + 4, ... and overwrites a finished row with final_obs[i], dwords.  The per-row scalars are the first 32 lanes', one row each.
 *
 * eb_replay_sample, ONE launch of ceil(m / 32) blocks (replay_sample_kernel): a minibatch of m rows drawn WITH replacement from the
 * f = *fill valid rows (f is read by the kernel and clamped to 0 .. C).  Outputs, each optional, at least one present:
 *   obs_out [m, D]   qin_out [m, D + A] = [obs | act]   next_obs_out [m, D]   rew_out [m]   nonterminal_out [m]   index_out [m] int32
 *   noise_id_out [m] uint32
 * Keyed route (indices NULL), all in unsigned 64-bit arithmetic, GOLDEN = 0x9E3779B97F4A7C15 and splitmix64 csrc/eb_env_device.h's:
 *   key  = splitmix64(seed + GOLDEN * (base + draw))        base = *counter when a device counter is given, else 0
 *   w(r) = splitmix64(key + GOLDEN * r)
 *   j(r) = mulhi64(w(r), f)                                 the high half of the 128-bit product: in [0, f), never in memory
 * so a replay sees the ring's growth and, after eb_epoch_advance on the counter, draws anew.  Explicit route: indices [m], int32
 * (index_bytes 4) or int64 (8), as eb_minibatch_gather's perm.  An explicit index outside [0, f) is never dereferenced, and no index is
 * when f == 0: that destination row is written as quiet NaNs (0x7FC00000) in every output and index_out gets -1.
 * noise_id_out[r] = (uint32_t)w(r), the LOW half of the row's word, on either route and whatever f is: a per-row number that changes
 * with every draw and is independent of the index (the high bits).  Passed as row_ids to eb_policy_sample it gives a replayed update
 * fresh action noise from device state alone — that entry's seed and counter are host scalars a captured graph cannot move.
 * Block k takes 32 destination rows; its first 32 lanes form the indices once and share them through LDS; then, output by output,
 * consecutive lanes write consecutive floats of the block's contiguous 32 x width destination (dwords: rows are views aligned to 4 bytes
 * only); rew_out and nonterminal_out (width 1) take one lane per row, each on another group of 32 lanes.
 *
 * eb_q_pack, ONE launch (q_pack_kernel): qin [m, D + A];  qin[i, :D] = obs[i, :] when obs is given, qin[i, D:] = act[i, :] when act is
 * given; at least one.  Columns of the part not given are not written.  It builds [next_obs | a'], and over a sampled qin_out it
 * overwrites the action columns alone with a fresh action.
 *
 * eb_sac_critic, ONE launch, one lane per row (sac_critic_kernel): the TD target and both critics' loss rows and cotangents.
 *   alpha = log_alpha ? exp_det(*log_alpha) : alpha         (exp_det: csrc/eb_mlp_device.h; the device word is read by the kernel)
 *   qm  = (q2t[i] < q1t[i]) ? q2t[i] : q1t[i];   qm = (q2t[i] != q2t[i]) ? q2t[i] : qm        a select; a NaN in either travels
 *   e   = alpha * logp_next[i]
 *   v   = qm - e
 *   y   = fmaf(gamma * nonterminal[i], v, reward_scale * rew[i])
 *   d_k = q_k[i] - y          loss_k[i] = (0.5f * d_k) * d_k          g_q_k[i] = d_k * inv_m          k = 1, 2
 * inv_m is a host float.  y, loss1, loss2, g_q1, g_q2 are each optional (at least one); q1 / q2 are needed only by their own outputs.
 * g_q_k is what eb_mlp_backward(head = 0) takes as g_out.
 *
 * eb_sac_actor, ONE launch without the temperature gradient, exactly TWO with it (sac_actor_kernel, sac_alpha_fold_kernel).  q1, q2:
 * the online critics at [obs | a_new].  alpha as above.  Per row:
 *   qm = the minimum as above          e = alpha * logp[i]          loss[i] = e - qm
 *   g_q1[i] = (q1[i] <= q2[i]) ? -inv_m : 0.0f        g_q2[i] = (q1[i] <= q2[i]) ? 0.0f : -inv_m      (a NaN in either: all to g_q2)
 *   g_logp[i] = alpha * inv_m
 * loss, g_q1, g_q2, g_logp are each optional.  With g_log_alpha the call forms S = sum over i of ((double)logp[i] + target_entropy)
 * ((double)target_entropy; one double addition per row) in eb_ppo_log's order: ALWAYS 64 blocks of 256 lanes; lane t of block b adds the
 * rows b * 256 + t + k * 16384, k ascending, in double from 0; the block folds by halving (x[t] += x[t + w], w = 128 .. 1) and writes
 * ONE double to partials[b] (caller-owned, 64 doubles, no initialisation needed).  The second launch, one block, adds the 64 partials in
 * ascending order from 0 and writes g_log_alpha[0] = (float)(-(S / (double)m)): the gradient of -log_alpha * mean(logp +
 * target_entropy).  No atomics, no last-block ticket.  The row work and the partials share the first launch: without g_log_alpha its grid
 * is ceil(m / 256) blocks, with it 64 blocks striding over the rows.
 *
 * eb_q_action_grad, ONE launch (q_action_grad_kernel): g_a[i, a] = g_in1[i, D + a] + g_in2[i, D + a], one fp32 addition; g_in1, g_in2
 * [m, D + A] are the two critics' g_obs, g_a the dense [m, A] eb_policy_sample_vjp takes.  g_in2 NULL (one critic, DDPG): g_a = g_in1's
 * columns as they are.
 *
 * eb_polyak, ONE launch (polyak_kernel): up to EB_OFFPOLICY_MAX_SEGMENTS (32) segments {target, online, count}, by value in the struct;
 *   t = fmaf(tau, o - t, t)             (o - t is one rounding, the fmaf the second)
 * per element.  target must not overlap online or another segment (not checked beyond equality of the two pointers).  The grid is
 * (min(ceil(largest count / 1024), 1024), n_segments): a block row per segment, each block walking chunks of 1024 elements of its
 * segment; an element's result does not depend on the grid.
 *
 * The Python package restates this contract in NumPy, in the kernels' own order: env_build_amd.offpolicy.push_reference,
 * sample_index_reference, sample_reference, q_pack_reference, critic_reference, actor_reference, action_grad_reference, polyak_reference.
 */
#ifndef ENVBUILD_OFFPOLICY_H
#define ENVBUILD_OFFPOLICY_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_OFFPOLICY_ABI_VERSION 1
#define EB_OFFPOLICY_MAX_OBS 4096
#define EB_OFFPOLICY_MAX_ACT 16
#define EB_OFFPOLICY_ROWS 32
#define EB_OFFPOLICY_ALPHA_BLOCKS 64
#define EB_OFFPOLICY_MAX_SEGMENTS 32

typedef struct eb_replay_push_args {
    int32_t capacity;          /* C, 1 .. 2^31 - 1, C * (D + A) <= 2^31 - 1 */
    int32_t n;                 /* rows, 0 .. C */
    int32_t start;             /* 0 .. C - 1 */
    int32_t obs_dim;           /* D, 1 .. 4096 */
    int32_t act_dim;           /* A, 1 .. 16 */
    int32_t fill_after;        /* 0 .. C; stored to *fill with the after part */
    float* obs;                /* [C, D], with the before part */
    float* act;                /* [C, A], with the before part */
    float* rew;                /* [C], with the after part */
    float* next_obs;           /* [C, D], with the after part */
    float* nonterminal;        /* [C], with the after part */
    uint64_t* fill;            /* DEVICE, one word, with the after part */
    const float* prev_obs;     /* [n, D] or NULL: no before part */
    const float* action;       /* [n, A], with prev_obs */
    const float* reward;       /* [n] or NULL: no after part */
    const float* obs_after;    /* [n, D], with reward */
    const uint8_t* done_code;  /* [n], with reward */
    const float* final_obs;    /* [n, D] or NULL; only with reward */
    void* stream;
} eb_replay_push_args;

typedef struct eb_replay_sample_args {
    int32_t capacity;          /* C, as above */
    int32_t m;                 /* rows drawn, 0 .. 2^31 - 1, m * (D + A) <= 2^31 - 1 */
    int32_t obs_dim, act_dim;  /* D, A */
    const float* obs;          /* the ring: each needed by the outputs that read it */
    const float* act;
    const float* rew;
    const float* next_obs;
    const float* nonterminal;
    const uint64_t* fill;      /* DEVICE, read at every replay */
    uint64_t seed, draw;       /* the keyed route */
    const uint64_t* counter;   /* DEVICE, or NULL: base = 0 */
    const void* indices;       /* [m] or NULL: the keyed route */
    int32_t index_bytes;       /* 4 or 8; read only with indices */
    float* obs_out;            /* [m, D] or NULL */
    float* qin_out;            /* [m, D + A] or NULL */
    float* next_obs_out;       /* [m, D] or NULL */
    float* rew_out;            /* [m] or NULL */
    float* nonterminal_out;    /* [m] or NULL */
    int32_t* index_out;        /* [m] or NULL */
    uint32_t* noise_id_out;    /* [m] or NULL */
    void* stream;
} eb_replay_sample_args;

typedef struct eb_q_pack_args {
    int32_t m;                 /* rows, 0 .. 2^31 - 1, m * (D + A) <= 2^31 - 1 */
    int32_t obs_dim, act_dim;  /* D, A */
    const float* obs;          /* [m, D] or NULL */
    const float* act;          /* [m, A] or NULL */
    float* qin;                /* [m, D + A] */
    void* stream;
} eb_q_pack_args;

typedef struct eb_sac_critic_args {
    int32_t m;                 /* rows, 0 .. 2^31 - 1 */
    const float* q1t;          /* [m] each: the target critics at [next_obs | a'] */
    const float* q2t;
    const float* logp_next;    /* [m] */
    const float* rew;          /* [m] */
    const float* nonterminal;  /* [m] */
    const float* q1;           /* [m]; with loss1 or g_q1 */
    const float* q2;           /* [m]; with loss2 or g_q2 */
    const float* log_alpha;    /* DEVICE, one float, or NULL: alpha by value */
    float alpha;               /* NaN refused when log_alpha is NULL */
    float gamma, reward_scale, inv_m;   /* NaN refused */
    float* y;                  /* [m] each, or NULL */
    float* loss1;
    float* loss2;
    float* g_q1;
    float* g_q2;
    void* stream;
} eb_sac_critic_args;

typedef struct eb_sac_actor_args {
    int32_t m;                 /* rows, 0 .. 2^31 - 1 */
    const float* q1;           /* [m] each */
    const float* q2;
    const float* logp;         /* [m] */
    const float* log_alpha;    /* DEVICE, one float, or NULL: alpha by value */
    float alpha;               /* NaN refused when log_alpha is NULL */
    float inv_m;               /* NaN refused */
    float target_entropy;      /* NaN refused; read with g_log_alpha */
    float* loss;               /* [m] each, or NULL */
    float* g_q1;
    float* g_q2;
    float* g_logp;
    float* g_log_alpha;        /* [1] or NULL: no temperature gradient, one launch */
    double* partials;          /* EB_OFFPOLICY_ALPHA_BLOCKS doubles of device scratch, with g_log_alpha */
    void* stream;
} eb_sac_actor_args;

typedef struct eb_q_action_grad_args {
    int32_t m;                 /* rows, 0 .. 2^31 - 1, m * (D + A) <= 2^31 - 1 */
    int32_t obs_dim, act_dim;  /* D, A */
    const float* g_in1;        /* [m, D + A] */
    const float* g_in2;        /* [m, D + A] or NULL */
    float* g_a;                /* [m, A] */
    void* stream;
} eb_q_action_grad_args;

typedef struct eb_polyak_segment {
    float* target;             /* [count]  updated in place */
    const float* online;       /* [count] */
    int64_t count;             /* 0 .. 2^31 - 1; with 0 the pointers are not read */
} eb_polyak_segment;

typedef struct eb_polyak_args {
    int32_t n_segments;        /* 0 .. EB_OFFPOLICY_MAX_SEGMENTS */
    eb_polyak_segment segments[EB_OFFPOLICY_MAX_SEGMENTS];
    float tau;                 /* NaN refused */
    void* stream;
} eb_polyak_args;

int eb_offpolicy_abi_version(void);
const char* eb_offpolicy_last_error(void);

/* ONE launch (none with n 0).  EB_EINVAL: NULL args; capacity < 1; n outside 0 .. capacity; start outside 0 .. capacity - 1; obs_dim
 * outside 1 .. 4096; act_dim outside 1 .. 16; capacity * (obs_dim + act_dim) above 2^31 - 1; and with n > 0: neither prev_obs nor
 * reward; one of prev_obs / action without the other, or with them a NULL or not 4-byte aligned obs, act, prev_obs or action; one of
 * reward / obs_after / done_code without the others, final_obs without them, or with them fill_after outside 0 .. capacity, a NULL or not
 * 4-byte aligned rew, next_obs, nonterminal, reward or obs_after, a not 4-byte aligned final_obs, a NULL or not 8-byte aligned fill. */
int eb_replay_push(const eb_replay_push_args*);

/* ONE launch (none with m 0).  EB_EINVAL: NULL args; capacity, obs_dim, act_dim as above; m outside 0 .. 2^31 - 1; m * (obs_dim +
 * act_dim) above 2^31 - 1; and with m > 0: no output; a NULL or not 8-byte aligned fill; a not 8-byte aligned counter; with indices an
 * index_bytes that is neither 4 nor 8 or indices not aligned to it; a not 4-byte aligned output; a NULL or not 4-byte aligned ring array
 * that an output present reads (obs: obs_out, qin_out; act: qin_out; next_obs, rew, nonterminal: their outputs). */
int eb_replay_sample(const eb_replay_sample_args*);

/* ONE launch (none with m 0).  EB_EINVAL: NULL args; m, obs_dim, act_dim, m * (obs_dim + act_dim) as above; and with m > 0: neither
 * obs nor act; a NULL or not 4-byte aligned qin; a not 4-byte aligned obs or act. */
int eb_q_pack(const eb_q_pack_args*);

/* ONE launch (none with m 0).  EB_EINVAL: NULL args; m outside 0 .. 2^31 - 1; a NaN gamma, reward_scale or inv_m; a NaN alpha without
 * log_alpha; and with m > 0: no output; a NULL or not 4-byte aligned q1t, q2t, logp_next, rew or nonterminal; a not 4-byte aligned
 * log_alpha or output; loss1 or g_q1 with a NULL or not 4-byte aligned q1, loss2 or g_q2 likewise with q2. */
int eb_sac_critic(const eb_sac_critic_args*);

/* ONE launch, or exactly TWO with g_log_alpha (none with m 0).  EB_EINVAL: NULL args; m outside 0 .. 2^31 - 1; a NaN inv_m; a NaN alpha
 * without log_alpha; with g_log_alpha a NaN target_entropy; and with m > 0: no output; a NULL or not 4-byte aligned q1, q2 or logp; a
 * not 4-byte aligned log_alpha or output; with g_log_alpha a NULL or not 8-byte aligned partials. */
int eb_sac_actor(const eb_sac_actor_args*);

/* ONE launch (none with m 0).  EB_EINVAL: NULL args; m, obs_dim, act_dim, m * (obs_dim + act_dim) as above; and with m > 0: a NULL or
 * not 4-byte aligned g_in1 or g_a; a not 4-byte aligned g_in2. */
int eb_q_action_grad(const eb_q_action_grad_args*);

/* ONE launch (none when no segment has elements).  EB_EINVAL: NULL args; n_segments outside 0 .. 32; a NaN tau; a count outside 0 ..
 * 2^31 - 1 or a total above it; for a segment with elements a NULL or not 4-byte aligned target or online, or target == online. */
int eb_polyak(const eb_polyak_args*);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_OFFPOLICY_H */
