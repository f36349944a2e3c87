/*
 * envbuild_collect.h — C-ABI of the COLLECTION phase of a PPO iteration: the rollout buffer the env step's outputs are recorded into
 * (eb_collect_begin, eb_collect_record: ONE launch each), the bootstrap values of time-limit truncations (eb_collect_next_values, ONE
 * launch) and the episode statistics (eb_collect_episode_log, ONE launch): csrc/eb_collect.hip.  With them one PPO iteration is library
 * launches from the first sample to the last Adam step: per collected step eb_policy_sample, eb_env_step and eb_collect_record, and at
 * the head of the update two eb_mlp_forward of the value network, eb_collect_next_values, eb_policy_logp_from_logits and eb_gae.
 *
 * A LIBRARY OF ITS OWN.  These symbols are exported by env_build_amd/lib/libenvbuild_collect.so ONLY.  libenvbuild_hip.so,
 * libenvbuild_train.so, libenvbuild_epoch.so, EB_ABI_VERSION and every other family's version are untouched.  Return codes are
 * envbuild.h's (EB_OK, EB_EINVAL, EB_EDEVICE); the reason of a failure is in eb_collect_last_error() — this library's own string, NOT
 * eb_last_error().  Nothing here synchronises, allocates, copies or uses atomics.  The library sees no eb_mlp handle and runs no
 * network: the networks are run by the entries of envbuild.h / envbuild_policy_sample.h, which write straight into the buffers below
 * through pointers.  The working entries run on the current device.
 *
 * Every working entry takes ONE struct.  Its stream is therefore a field, not a parameter, and the table of stream-taking prototypes
 * (tests/test_stream_census.py) does not count it: tests/test_gpu_collect.py holds each entry to that table's obligations (a side
 * stream, capture, replay).  Every scalar and every pointer of a struct is read AT CALL TIME.
 *
 * The rollout buffer.  B = n_env envs, D = obs_dim floats per observation, T steps.  Arrays named [T, B] are t-major — element (t, i)
 * at t * B + i — the layout eb_gae reads (envbuild_ppo.h).  obs_buf is [T + 1, B, D]: slot t holds the observation step t acted on, slot
 * T the observation that bootstraps the last step.  A slot's B * D floats are ONE contiguous run in the source and in the destination.
 *
 * eb_collect_begin, ONE launch:
 *   obs_buf[0, :, :] = obs[:, :]        trunc_t[i] = -1 for every env i                                  and it writes nothing else.
 *
 * eb_collect_record, ONE launch per env step: slot t from what eb_env_step left behind — obs [B, D] (the observation AFTER the step; the
 * reset rows of the finished envs under auto-reset), reward [B], done_code [B] (uint8, envbuild.h's EB_DONE_*), final_obs [B, D] or NULL
 * (eb_auto_reset's: the terminal observation in the rows of the finished envs, the other rows unspecified and never read) — and the
 * running state ep_ret [B] (float), ep_len [B] (int32).  Per env i, with
 *   c = done_code[i]        live = (c == 0)        trunc = (c == EB_DONE_TIME_LIMIT && final_obs != NULL)
 * it writes
 *   obs_buf[t + 1, i, :] = obs[i, :]                rew_buf[t, i] = reward[i]
 *   nonterminal[t, i] = (live || trunc) ? 1.0f : 0.0f
 *   carry[t, i]       = live ? 1.0f : 0.0f
 *   if trunc:  trunc_obs[i, :] = final_obs[i, :]    trunc_t[i] = t             # the row of an env that is not truncated is NOT touched
 *   R = ep_ret[i] + reward[i]  (one fp32 addition)  L = ep_len[i] + 1
 *   ret_buf[t, i] = R          len_buf[t, i] = L    code_buf[t, i] = c
 *   (ep_ret[i], ep_len[i]) = (c != 0) ? (0.0f, 0) : (R, L)
 * nonterminal, carry and next_values (below) are eb_gae's truncation arrays: a time-limit truncation is nonterminal = 1 (its delta
 * bootstraps), carry = 0 (the running advantage stops at the episode's end) and next_values = V(final_obs).  With final_obs NULL a
 * time-limit code is an ordinary termination (nonterminal = carry = 0).  ret_buf / len_buf hold the RUNNING return and length of the
 * episode at every slot; where code_buf != 0 they are the finished episode's.  The inputs are not written; the state carries from one
 * collection to the next (the caller zeroes it once).
 *
 * ONE trunc_obs ROW PER ENV SUFFICES when T <= max_episode_steps, the env's time limit: the limit counts the steps since the env's last
 * reset, so two truncations of one env lie at least max_episode_steps steps apart — the first at some t0 >= 0 of the collection, a
 * second not before t0 + max_episode_steps >= T, outside it.  (An env may TERMINATE any number of times within a collection; only the
 * truncation needs a stored observation.)  The library cannot see the env's limit: the caller holds T to it (env_build_amd.collect.
 * Collector refuses steps > env.max_episode_steps).  Were the bound broken, the later truncation would overwrite the row and trunc_t,
 * and eb_collect_next_values would bootstrap the earlier one from values[t + 1]: wrong numbers, no fault.
 *
 * eb_collect_next_values, ONE launch: with values [T + 1, B] (the value network over obs_buf) and v_trunc [B] (over trunc_obs),
 *   next_values[t, i] = (trunc_t[i] == t) ? v_trunc[i] : values[t + 1, i]                     0 <= t < T
 * A select: the value of a trunc_obs row nobody wrote (whatever the buffer held, a NaN included) does not travel.
 *
 * eb_collect_episode_log, ONE launch of EB_COLLECT_LOG_BLOCKS = 64 blocks of 256 lanes, always, over the n = T * B slots of ret_buf,
 * len_buf and code_buf: block b takes the slots b * 256 + lane, stepping by 64 * 256, in ascending order, folds by halving (x[t] op=
 * x[t + w], w = 128 .. 1) and writes out[b][0 .. 15], doubles.  A slot is FINISHED when its code != 0; R, L are its ret_buf, len_buf:
 *    0  the number of finished slots
 *    1  sum R            2  sum R * R  (the product in double)            over the finished slots whose R is not a NaN
 *    3  sum L                                                             over the finished slots
 *    4  max R            5  min R      (selects from -inf / +inf)         over the finished slots whose R is not a NaN
 *    6  the number of finished slots whose R is not finite (a NaN or an infinity)
 *    7 .. 14  the number of slots with code 0 .. 7 (code 0, not finished, included; a code above 7 is counted in field 0 only)
 *   15  the block's slot count
 * Blocks without slots write zeros, with fields 4 and 5 at -inf and +inf.  An infinite R is in the sums and in the maximum or minimum, as
 * IEEE has it; field 6 says that the figures are not to be trusted.  The fold over the 64 blocks is the reader's, on the host, in
 * ascending order, whenever the caller chooses to read (env_build_amd.collect.fold_episode_log).
 *
 * A count of 0 (n_env, obs_dim of a copy, n_slots) is a no-op that launches nothing; a refusal names its entry in eb_collect_last_error
 * and launches and writes nothing; repeated calls on equal inputs repeat their bits.  The Python package restates this contract in
 * NumPy: env_build_amd.collect.record_reference, next_values_reference and episode_log_reference.
 */
#ifndef ENVBUILD_COLLECT_H
#define ENVBUILD_COLLECT_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_COLLECT_ABI_VERSION 1
#define EB_COLLECT_LOG_BLOCKS 64
#define EB_COLLECT_LOG_FIELDS 16

typedef struct eb_collect_begin_args {
    int32_t n_env;             /* B, 0 .. 2^31 - 1 */
    int32_t obs_dim;           /* D, 1 .. 2^31 - 1, B * D <= 2^31 - 1 */
    const float* obs;          /* [B, D] */
    float* obs_buf;            /* [T + 1, B, D]: slot 0 is written */
    int32_t* trunc_t;          /* [B] */
    void* stream;
} eb_collect_begin_args;

typedef struct eb_collect_record_args {
    int32_t n_env;             /* B, 0 .. 2^31 - 1 */
    int32_t obs_dim;           /* D, 1 .. 2^31 - 1, B * D <= 2^31 - 1 */
    int32_t steps;             /* T, 1 .. 2^31 - 1 */
    int32_t t;                 /* the step recorded, 0 .. T - 1 */
    const float* obs;          /* [B, D] */
    const float* reward;       /* [B] */
    const uint8_t* done_code;  /* [B] */
    const float* final_obs;    /* [B, D] or NULL: a time-limit code is then a termination */
    float* ep_ret;             /* [B], read and written */
    int32_t* ep_len;           /* [B], read and written */
    float* obs_buf;            /* [T + 1, B, D]: slot t + 1 is written */
    float* rew_buf;            /* [T, B] each: element (t, i) is written */
    float* nonterminal;
    float* carry;
    float* ret_buf;
    int32_t* len_buf;
    uint8_t* code_buf;
    float* trunc_obs;          /* [B, D]; needed only with final_obs */
    int32_t* trunc_t;          /* [B];    needed only with final_obs */
    void* stream;
} eb_collect_record_args;

typedef struct eb_collect_next_values_args {
    int32_t n_env;             /* B, 0 .. 2^31 - 1 */
    int32_t steps;             /* T, 0 .. 2^31 - 1, (T + 1) * B <= 2^31 - 1 */
    const float* values;       /* [T + 1, B] */
    const float* v_trunc;      /* [B] */
    const int32_t* trunc_t;    /* [B] */
    float* next_values;        /* [T, B] */
    void* stream;
} eb_collect_next_values_args;

typedef struct eb_collect_episode_log_args {
    int64_t n_slots;           /* T * B, 0 .. 2^31 - 1 */
    const float* ret_buf;      /* [n_slots] each */
    const int32_t* len_buf;
    const uint8_t* code_buf;
    double* out;               /* [EB_COLLECT_LOG_BLOCKS][EB_COLLECT_LOG_FIELDS] */
    void* stream;
} eb_collect_episode_log_args;

int eb_collect_abi_version(void);
const char* eb_collect_last_error(void);

/* The first slot as stated above: ONE launch (none with n_env 0).
 * EB_EINVAL (nothing launched or written): NULL args, n_env outside 0 .. 2^31 - 1, obs_dim outside 1 .. 2^31 - 1, n_env * obs_dim above
 * 2^31 - 1, and with n_env > 0: a NULL or not 4-byte aligned obs, obs_buf or trunc_t. */
int eb_collect_begin(const eb_collect_begin_args* a);

/* One step as stated above: ONE launch (none with n_env 0).
 * EB_EINVAL: NULL args, n_env outside 0 .. 2^31 - 1, obs_dim or steps outside 1 .. 2^31 - 1, n_env * obs_dim above 2^31 - 1, t outside
 * [0, steps), and with n_env > 0: a NULL done_code, code_buf, or a NULL or not 4-byte aligned obs, reward, ep_ret, ep_len, obs_buf,
 * rew_buf, nonterminal, carry, ret_buf or len_buf; final_obs not 4-byte aligned; with final_obs, a NULL or not 4-byte aligned trunc_obs
 * or trunc_t. */
int eb_collect_record(const eb_collect_record_args* a);

/* The bootstrap values as stated above: ONE launch (none with n_env or steps 0).
 * EB_EINVAL: NULL args, n_env or steps outside 0 .. 2^31 - 1, (steps + 1) * n_env above 2^31 - 1, and with work to do: a NULL or not
 * 4-byte aligned values, v_trunc, trunc_t or next_values. */
int eb_collect_next_values(const eb_collect_next_values_args* a);

/* The episode statistics as stated above: ONE launch of EB_COLLECT_LOG_BLOCKS blocks (none with n_slots 0).
 * EB_EINVAL: NULL args, n_slots outside 0 .. 2^31 - 1, and with n_slots > 0: a NULL code_buf, a NULL or not 4-byte aligned ret_buf or
 * len_buf, a NULL or not 8-byte aligned out. */
int eb_collect_episode_log(const eb_collect_episode_log_args* a);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_COLLECT_H */
