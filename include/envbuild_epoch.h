/*
 * envbuild_epoch.h — C-ABI of what the update phase of a PPO iteration needs AROUND the minibatch chain of envbuild_train.h: the
 * minibatch gather under a keyed shuffle whose permutation never exists in memory (eb_minibatch_gather, ONE launch), the two floats of
 * the advantage normalisation (eb_adv_stats, always exactly TWO launches), the per-minibatch logging sums (eb_ppo_log, ONE launch) and
 * the iteration counter of the shuffle on the DEVICE (eb_epoch_advance, ONE launch): csrc/eb_epoch.hip.  With them epochs x minibatches
 * minibatches — shuffles, gathers, normalisation and logging included — are one linear chain of library kernels that can be captured
 * once and replayed once per iteration: a replayed graph takes the NEXT iteration's permutations.
 *
 * A LIBRARY OF ITS OWN.  These symbols are exported by env_build_amd/lib/libenvbuild_epoch.so ONLY.  libenvbuild_hip.so,
 * libenvbuild_train.so, EB_ABI_VERSION and every other family's version are untouched.  Return codes are envbuild.h's (EB_OK, EB_EINVAL,
 * EB_EDEVICE); the reason of a failure is in eb_epoch_last_error() — this library's own string, NOT eb_last_error().  Nothing here
 * synchronises, allocates, copies or uses atomics.  The working entries run on the current device.
 *
 * Every working entry takes ONE struct.  Its stream is therefore a field, not a parameter, and the table of stream-taking prototypes
 * (tests/test_stream_census.py) does not count it: tests/test_gpu_epoch.py holds each entry to that table's obligations (a side stream,
 * capture, replay).  Every scalar and every pointer of a struct is read AT CALL TIME: under stream capture those values are baked into the
 * graph, and the device buffers they point to — the counter included — are read at every replay.
 *
 * The index function.  index(key, n, i) for 0 <= i < n <= 2^31 - 1 is a KEYED BIJECTION of [0, n): a 6-round balanced Feistel network
 * over the next even power of two, with cycle walking.  All arithmetic is unsigned 64-bit with wrap-around; GOLDEN = 0x9E3779B97F4A7C15
 * and splitmix64 is the sampler's (csrc/eb_env_device.h):
 *
 *   b = max(2, bit_length(n - 1)) rounded up to even        h = b / 2        mask = 2^h - 1
 *   key = splitmix64(seed + GOLDEN * (base + epoch))        base = *counter when a device counter is given, else 0
 *   x = i
 *   repeat
 *     L = x >> h        R = x & mask
 *     for r = 0 .. 5:   F = (splitmix64(key + GOLDEN * ((r << 32) | R)) >> 32) & mask        (L, R) = (R, L ^ F)
 *     x = (L << h) | R
 *   until x < n
 *
 * One pass of the rounds is a permutation of [0, 2^b), whatever F is; the domain is below 4 n, so a walk takes fewer than 4 passes on
 * average, and it terminates because a cycle of a permutation returns to its start, which is below n.  base + epoch is what keys a
 * permutation: (base = 1, epoch = 0) is (base = 0, epoch = 1).  The contract is "a keyed bijection with the coarse uniformity the tests
 * hold" (tests/test_epoch_host.py: the quarter a slot's source row falls into, fixed points, agreement between keys).
 * It is NOT a certified uniform shuffle, and no cryptographic claim is made.
 *
 * The gather.  n_sources in 1 .. EB_EPOCH_MAX_SOURCES sources {src, dst, width} of n_total rows each; a row is `width` contiguous floats,
 * and src and dst need 4-byte alignment only (widths 41 and 137 are odd; a destination may be a view at an odd float offset).
 * Destination row r < count of every source takes source row
 *   perm[offset + r]                       the explicit route: perm not NULL, elements of perm_bytes 4 (int32) or 8 (int64)
 *   index(key, n_total, offset + r)        the keyed route: perm NULL
 * An explicit index outside [0, n_total) is NEVER dereferenced: its destination row is written as quiet NaNs (0x7FC00000) in every
 * source and index_out gets -1.  index_out ([count] int32, optional) receives the source row each destination row took.  The sources
 * are not written.  ONE launch, always: block k of 256 lanes takes the EB_EPOCH_GATHER_ROWS = 32 destination rows from 32 k; the
 * first 32 lanes compute (or read) the rows' indices ONCE and share them through LDS; then, source by source, consecutive lanes move
 * consecutive floats of the block's 32 x width destination floats as dwords (width >= 3), or one lane moves one row (width 1 or 2).
 *
 * The statistics.  n >= 2.  With d = (double)x - (double)x[0], the deviation from the FIRST element, S = sum d and Q = sum d * d in an
 * order that is a pure function of n — Adam's (envbuild_train.h): x is cut into ceil(n / 1024) chunks of 1024 consecutive elements, C in
 * all, P = min(C, EB_EPOCH_PARTIALS); block b < P of 256 lanes takes the chunks b, b + P, ... in ascending order, lane t adds to two
 * doubles that start at +0.0 the elements t, t + 256, t + 512, t + 768 of each chunk in that order, the block's doubles are folded by
 * halving (x[t] += x[t + w], w = 128 .. 1) and written to partials[b] (S) and partials[EB_EPOCH_PARTIALS + b] (Q): launch 1
 * (adv_stats_partial_kernel).  Launch 2 (adv_stats_fold_kernel, one block) folds the partials 0 .. P-1 (the rest +0.0) by the same
 * halving and one lane writes
 *   mean = (float)((double)x[0] + S / n)
 *   v = (Q - S * S / n) / (n - 1)        var = v < 0 ? 0 : v            # doubles; unbiased, as torch.std; a select: a NaN travels
 *   std = (float)sqrt(var)
 *   inv = 1.0f / (std + (float)eps)                                     # fp32, IEEE division
 * to out[0] = mean, out[1] = inv — the layout eb_ppo_args.adv_norm reads — and std to std_out when given.  No atomics and no last-block
 * ticket.  A NaN element makes all three NaN.  Q - S^2 / n in double LOSES DIGITS to cancellation: about m^2 / var * 2^-53 of the
 * variance, where m is the mean OF THE DEVIATIONS, mean - x[0].  Without the shift m would be the mean itself, and data at mean / std =
 * 10^3 would keep 10 digits of the standard deviation (measured: 4e-11 relative at n = 100 003); with it m is of the order of the
 * standard deviation whatever the mean, unless x[0] itself lies many standard deviations out: the result is meaningless once
 * (mean - x[0])^2 / var approaches 10^9 or more.  Advantages are nowhere near that.
 *
 * The log.  EB_EPOCH_LOG_BLOCKS = 64 blocks of 256 lanes, always; block b takes the rows b * 256 + t, stepping by 64 * 256, in ascending
 * order, folds by halving and writes out[b][0 .. 7], doubles:
 *   0  sum surr            1  sum vloss            2  sum ent
 *   3  the number of rows with fabsf(ratio - 1.0f) > clip                # fp32, the trainer's torch expression
 *   4  sum (double)(logp_old - logp)                                     # the subtraction in fp32; needs both, else 0
 *   5  max fabsf(ratio - 1.0f)                                           # a select from 0: a NaN is passed over (it is counted in 6)
 *   6  the number of rows where any GIVEN input is not finite
 *   7  the block's row count
 * A NULL input contributes 0.  Blocks without rows write zeros.  The fold over the 64 blocks is the reader's, on the host, in a fixed
 * order, whenever the caller chooses to read (env_build_amd.epoch.fold_log).
 *
 * The counter.  eb_epoch_advance: one lane does *counter += by.  The keyed gathers of an iteration read the counter, the advance at the
 * iteration's end moves it past the iteration's epochs; ordering is the stream's.
 *
 * A count of 0 is a no-op that launches nothing; a refusal names its entry in eb_epoch_last_error and launches and writes nothing; a NaN
 * scalar is refused; repeated calls on equal inputs repeat their bits.  The Python package restates this contract in NumPy:
 * env_build_amd.epoch.index_reference, adv_stats_reference and ppo_log_reference.
 */
#ifndef ENVBUILD_EPOCH_H
#define ENVBUILD_EPOCH_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_EPOCH_ABI_VERSION 1
#define EB_EPOCH_MAX_SOURCES 8
#define EB_EPOCH_MAX_WIDTH 4096
#define EB_EPOCH_GATHER_ROWS 32
#define EB_EPOCH_PARTIALS 256
#define EB_EPOCH_LOG_BLOCKS 64
#define EB_EPOCH_LOG_FIELDS 8

typedef struct eb_gather_source {
    const float* src;          /* [n_total, width] */
    float* dst;                /* [count, width] */
    int32_t width;             /* floats per row, 1 .. EB_EPOCH_MAX_WIDTH */
} eb_gather_source;

typedef struct eb_gather_args {
    int64_t n_total;           /* rows of every source, 0 .. 2^31 - 1 */
    int64_t offset, count;     /* 0 .. 2^31 - 1 each, offset + count <= n_total */
    int32_t n_sources;         /* 1 .. EB_EPOCH_MAX_SOURCES */
    eb_gather_source sources[EB_EPOCH_MAX_SOURCES];
    const void* perm;          /* [n_total] or NULL: the keyed route */
    int32_t perm_bytes;        /* 4 or 8; read only with perm */
    uint64_t seed, epoch;      /* the keyed route */
    const uint64_t* counter;   /* DEVICE, or NULL: base = 0 */
    int32_t* index_out;        /* [count] or NULL */
    void* stream;
} eb_gather_args;

typedef struct eb_adv_stats_args {
    int64_t n;                 /* 0, or 2 .. 2^31 - 1 */
    const float* x;            /* [n] */
    double eps;                /* NaN refused */
    float* out;                /* [2]: mean, 1 / (std + eps) */
    float* std_out;            /* [1] or NULL */
    double* partials;          /* 2 * EB_EPOCH_PARTIALS doubles of device scratch */
    void* stream;
} eb_adv_stats_args;

typedef struct eb_ppo_log_args {
    int64_t n;                 /* 0 .. 2^31 - 1 */
    const float* logp;         /* [n] each, or NULL */
    const float* logp_old;
    const float* ratio;
    const float* surr;
    const float* ent;
    const float* vloss;
    float clip;                /* NaN refused */
    double* out;               /* [EB_EPOCH_LOG_BLOCKS][EB_EPOCH_LOG_FIELDS] */
    void* stream;
} eb_ppo_log_args;

typedef struct eb_epoch_advance_args {
    uint64_t* counter;         /* DEVICE */
    uint64_t by;
    void* stream;
} eb_epoch_advance_args;

int eb_epoch_abi_version(void);
const char* eb_epoch_last_error(void);

/* The gather as stated above: ONE launch (none with count 0).
 * EB_EINVAL (nothing launched or written): NULL args, n_total, offset or count outside 0 .. 2^31 - 1, offset + count > n_total,
 * n_sources outside 1 .. EB_EPOCH_MAX_SOURCES, a width outside 1 .. EB_EPOCH_MAX_WIDTH, and with count > 0: a NULL or not 4-byte aligned
 * src or dst, perm_bytes other than 4 or 8 with perm, perm not aligned to perm_bytes, counter not 8-byte aligned, index_out not 4-byte
 * aligned. */
int eb_minibatch_gather(const eb_gather_args* a);

/* The statistics as stated above: ALWAYS exactly TWO launches (none with n 0).
 * EB_EINVAL: NULL args, n 1, n outside 0 .. 2^31 - 1, eps NaN, and with n > 0: NULL or not 4-byte aligned x or out, std_out not 4-byte
 * aligned, NULL or not 8-byte aligned partials. */
int eb_adv_stats(const eb_adv_stats_args* a);

/* The log as stated above: ONE launch of EB_EPOCH_LOG_BLOCKS blocks (none with n 0).
 * EB_EINVAL: NULL args, n outside 0 .. 2^31 - 1, clip NaN, and with n > 0: an input not 4-byte aligned, NULL or not 8-byte aligned out. */
int eb_ppo_log(const eb_ppo_log_args* a);

/* *counter += by: ONE launch.  EB_EINVAL: NULL args, NULL or not 8-byte aligned counter. */
int eb_epoch_advance(const eb_epoch_advance_args* a);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_EPOCH_H */
