/*
 * envbuild_norm.h — C-ABI of the RUNNING NORMALISATION of observations and rewards on the device: the reference's 'normalize'
 * preprocessor (utils/preprocessor.py: RunningMeanStd, process_obs, process_rew, np_process_obses, np_process_rewards) as library
 * launches — eb_norm_update (exactly TWO launches) merges a batch into the running statistics, eb_norm_apply (ONE launch) normalises with
 * them: csrc/eb_norm.hip.
 *
 * A LIBRARY OF ITS OWN.  These symbols are exported by env_build_amd/lib/libenvbuild_norm.so ONLY; the other six libraries, EB_ABI_VERSION
 * and every other family's version are untouched.  Return codes are envbuild.h's (EB_OK, EB_EINVAL, EB_EDEVICE); the reason of a failure
 * is in eb_norm_last_error() — this library's own string, NOT eb_last_error().  Nothing here synchronises, allocates, copies or uses
 * atomics.  The working entries run on the current device.
 *
 * Every working entry takes ONE struct.  Its stream is therefore a field, not a parameter, and the table of stream-taking prototypes
 * (tests/test_stream_census.py) does not count it; the two prototypes are declared without a parameter name, as envbuild_ac.h's are, so
 * that the fixed table of the other families' struct-taking entries stays as it is: tests/test_norm_host.py and tests/test_gpu_norm.py
 * hold each entry to that table's obligations (a side stream, capture, replay).  Every scalar and every pointer of a struct is read AT CALL TIME.
 *
 * THE STATE of width D is caller-owned device memory, two arrays:
 *   stat   double[2 D + 1]:  mean[D], var[D], count            the reference's RunningMeanStd, in double
 *   scale  float[2 D]:       mean_f[D], den_f[D]               what eb_norm_apply reads:
 *                            mean_f = (float)mean      den_f = sqrtf((float)var + eps_f)
 * eps_f is the fp32 rounding of the reference's epsilon and the sqrt the correctly rounded fp32 one.  The initial state is the
 * reference's: mean 0, var 1, count 1e-4 (and scale derived from it by the two formulas above).  Two states exist in a PPO collection:
 * one of width D for the observations and one of width 1 for the discounted return; ret_run [n] (fp32) is the per-env running
 * discounted return the second one is fed from.
 *
 * eb_norm_update, exactly TWO launches, no atomics.  Two optional parts, at least one present, both over the same n rows:
 *   observation part  x [n, D] -> the state (obs_stat, obs_scale) of width D;
 *   return part       per env i:  R = ret_run[i] * gamma + reward[i]   (one fp32 multiply, one fp32 add: the reference's
 *                     `self.ret * self.gamma + rew`);  ret_run[i] = R;  the n values of R are the batch of the width-1 state
 *                     (ret_stat, ret_scale).
 * First launch (norm_partial_kernel): min(ceil(n / 32), EB_NORM_MAX_BLOCKS) blocks of 256 lanes.  Block b takes the 32 rows from
 * 32 (b + k * blocks), k = 0, 1, ...: each run of 32 x D floats is staged in LDS (16-byte loads when x is 16-byte aligned, dwords
 * otherwise and for the tail).  With G = min(256 / D, 32) row groups, lane g * D + d (g < G) owns column d and walks the rows g, g + G,
 * ... of every run, ascending, summing in double
 *   S1 += (x - K)        S2 += (x - K) * (x - K)        K = (double)mean_f[d] as it stood BEFORE the launch
 * — the multiply and the add are separate roundings, and the shift keeps the one-pass sums from cancelling when |mean| >> std.  The G
 * lanes of a column are folded in LDS by halving, s[g] += s[g + w] for w = P / 2 .. 1 with P the power of two >= G (g + w < G), and ONE
 * partial per block and column is written to the workspace.  The return column is summed the same way by the block's first 32 lanes,
 * one row of every run each (G = 32), with K = (double)ret_scale[0].  The order is a pure function of (n, D).
 * Second launch (norm_fold_kernel, one block, one lane per column): the partials are added in ascending block order, then, all in
 * double and in the reference's operation order (update_mean_var_count_from_moments, preprocessor.py:14-25), with N = (double)n:
 *   a = S1 / N        bm = K + a        bv = S2 / N - a * a        bv = (bv < 0) ? 0 : bv            (a NaN travels)
 *   delta = bm - mean         tot = count + N
 *   mean' = mean + (delta * N) / tot
 *   M2 = (var * count + bv * N) + (((delta * delta) * count) * N) / tot
 *   var' = M2 / tot           count' = tot
 * and mean_f and den_f of the column are rewritten from mean', var' and eps.  The workspace — eb_norm_workspace_bytes(D) bytes, 8-byte
 * aligned, caller-owned — needs no initialisation and holds nothing between calls.
 *
 * eb_norm_apply, ONE launch of ceil(n / 32) blocks.  It reads the states and NEVER writes them.  Three optional parts, at least one
 * present, over the same n rows; mean_f and den_f are staged in LDS once per block:
 *   dense observations   y[i, d] = clip((x[i, d] - mean_f[d]) / den_f[d])        one fp32 subtraction, one IEEE fp32 division
 *                        clip(v) = min(max(v, -clip_obs), clip_obs) as two selects (v < -c ? -c : v, then v > c ? c : v): a NaN travels.
 *                        y may be x itself (in place); any other overlap is undefined.  16-byte accesses when x and y are both 16-byte
 *                        aligned, dwords otherwise and for the tail.
 *   selected rows        the same in place on sel_x [n, D], ONLY for the rows i with sel[i] == sel_value (int32).  The rows not
 *                        selected are neither read nor written.
 *   reward               reward_out[i] = clip(reward[i] / den_ret_f) with clip_rew and den_ret_f = ret_scale[1]: NO mean subtraction
 *                        (preprocessor.py:87).  reward_out may be reward itself.  With done_code (uint8 [n]) and ret_run:
 *                        ret_run[i] = (done_code[i] != 0) ? 0 : ret_run[i]
 *                        — the reference's evident intent.  Its batched branch, `np.where(done == 1, np.zeros(self.ret), self.ret)`
 *                        (preprocessor.py:88), RAISES as written, because np.zeros receives the array as a shape; its single-env branch
 *                        (`0 if done else self.ret`) is what this restates per env.  done_code and ret_run are given together or not
 *                        at all (frozen statistics: ret_run is then left alone).
 * The update comes BEFORE the apply of the same batch, as in process_obs / process_rew.
 *
 * A count of 0 (n) is a no-op that launches nothing and needs no pointer; a refusal names its entry in eb_norm_last_error and launches
 * and writes nothing; repeated calls on equal inputs repeat their bits.  The Python package restates this contract in NumPy, in the
 * kernels' own order: env_build_amd.norm.update_reference and apply_reference.
 */
#ifndef ENVBUILD_NORM_H
#define ENVBUILD_NORM_H

#include <stddef.h>

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_NORM_ABI_VERSION 1
#define EB_NORM_MAX_DIM 256
#define EB_NORM_MAX_BLOCKS 512

typedef struct eb_norm_update_args {
    int32_t n;                 /* rows (envs), 0 .. 2^31 - 1 */
    int32_t dim;               /* D, 1 .. 256, n * D <= 2^31 - 1 (1 for a call with the return part alone) */
    const float* x;            /* [n, D] or NULL: no observation part */
    double* obs_stat;          /* [2 D + 1], with x */
    float* obs_scale;          /* [2 D], with x */
    const float* reward;       /* [n] or NULL: no return part */
    float* ret_run;            /* [n], with reward: read and written */
    double* ret_stat;          /* [3], with reward */
    float* ret_scale;          /* [2], with reward */
    double* workspace;         /* eb_norm_workspace_bytes(dim) bytes */
    float gamma;               /* finite; read with reward */
    float eps;                 /* finite: eps_f */
    void* stream;
} eb_norm_update_args;

typedef struct eb_norm_apply_args {
    int32_t n;                 /* rows (envs), 0 .. 2^31 - 1 */
    int32_t dim;               /* D, 1 .. 256, n * D <= 2^31 - 1 (1 for a call with the reward part alone) */
    const float* obs_scale;    /* [2 D], with x or sel_x */
    const float* x;            /* [n, D] or NULL: no dense part */
    float* y;                  /* [n, D], with x; may be x */
    float* sel_x;              /* [n, D] or NULL: no selected rows */
    const int32_t* sel;        /* [n], with sel_x */
    int32_t sel_value;
    float clip_obs;            /* finite */
    const float* ret_scale;    /* [2], with reward */
    const float* reward;       /* [n] or NULL: no reward part */
    float* reward_out;         /* [n], with reward; may be reward */
    const uint8_t* done_code;  /* [n] or NULL; with ret_run or not at all */
    float* ret_run;            /* [n] or NULL */
    float clip_rew;            /* finite */
    void* stream;
} eb_norm_apply_args;

int eb_norm_abi_version(void);
const char* eb_norm_last_error(void);

/* The size of eb_norm_update's workspace for width D: EB_NORM_MAX_BLOCKS * 2 * (D + 1) doubles; 0 for a D outside 1 .. 256. */
size_t eb_norm_workspace_bytes(int32_t dim);

/* The statistics as stated above: exactly TWO launches (none with n 0).
 * EB_EINVAL (nothing launched or written): NULL args, n outside 0 .. 2^31 - 1, dim outside 1 .. 256, n * dim above 2^31 - 1, a gamma or
 * eps that is not finite, and with n > 0: neither x nor reward; with x a NULL or misaligned obs_stat (8 bytes), obs_scale or x (4);
 * with reward a NULL or misaligned ret_stat (8), ret_scale, ret_run or reward (4); a NULL or not 8-byte aligned workspace. */
int eb_norm_update(const eb_norm_update_args*);

/* The normalisation as stated above: ONE launch (none with n 0).
 * EB_EINVAL: NULL args, n outside 0 .. 2^31 - 1, dim outside 1 .. 256, n * dim above 2^31 - 1, a clip_obs or clip_rew that is not
 * finite, and with n > 0: none of x, sel_x and reward; with x or sel_x a NULL or not 4-byte aligned obs_scale; with x a NULL or not
 * 4-byte aligned y, a not 4-byte aligned x; with sel_x a NULL or not 4-byte aligned sel, a not 4-byte aligned sel_x; with reward a NULL
 * or not 4-byte aligned ret_scale or reward_out, a not 4-byte aligned reward; one of done_code and ret_run without the other, or a
 * not 4-byte aligned ret_run, or either without reward. */
int eb_norm_apply(const eb_norm_apply_args*);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_NORM_H */
