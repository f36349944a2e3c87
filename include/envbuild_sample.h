/*
 * envbuild_sample.h — C-ABI of the sampled-tape rollout: S perturbed open-loop action tapes per env are drawn, rolled out from ONE
 * shared scene, scored and averaged in one launch (the inner step of a sampling MPC: MPPI / CEM).
 *
 * A header of its own next to envbuild.h, envbuild_grad.h, envbuild_cand.h and envbuild_cand_grad.h: these symbols are exported by
 * env_build_amd/lib/libenvbuild_hip.so ONLY (the CPU oracle of envbuild.h has none of them), the four older ABI numbers are
 * untouched, and a binding looks the symbols up on demand.  Conventions (return codes, eb_last_error, device pointers, `stream`) are
 * those of envbuild.h.
 *
 * Why the entry exists: the cost of an open-loop tape (EnvironmentModel.rollout_out, DAM:118-126, chained as mpc/main.py:470-479
 * chains it) is non-convex — the collision discs of DAM:218-229 — so a descent ends in the basin it starts in.  A sampling planner
 * takes hundreds of perturbed tapes per scene and a soft-min average of them, and needs no gradient.  The vehicles of a scene do not
 * depend on the ego (tf.stop_gradient on the vehicle columns, DAM:195, 331, 402; predict_for_a_mode, DAM:405-427, reads the
 * vehicle's own record only), so the S rollouts share one vehicle trajectory; the perturbations are a pure function of a counter
 * (the generator of eb_traffic_respawn), so they never exist in memory.
 *
 * nd = 6 + 3 * (n_future + 1), D = nd + 4 * n_veh.  fp32 obs rows only.
 */
#ifndef ENVBUILD_SAMPLE_H
#define ENVBUILD_SAMPLE_H

#include "envbuild.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EB_SAMPLE_ABI_VERSION 1

int eb_sample_abi_version(void);

/* Draws n_samples action tapes per env around `nominal`, rolls each out over `horizon` model steps from the env's row of obs0
 * (csrc/eb_rollout_tape_sample.hip), and returns their costs, the best one and their soft-min average.  One launch; no atomics to
 * global memory.
 *
 * Noise.   key = splitmix64(seed + GOLDEN * counter).  For env id i (env_ids[e], taken as an unsigned 32-bit number; NULL: the row
 *   index), sample s >= 1, step t, component a:   idx = 4 * (a + 2 * (t + H * (i * S + s)))  in uint64 (H = horizon, S = n_samples),
 *   u_j = u01(key, idx + j), j = 0..3, with splitmix64 / u01 / GOLDEN those of eb_traffic_respawn (csrc/eb_env_device.h:253-262);
 *       xi = (((u_0 + u_1) + (u_2 + u_3)) - 2.0f) * 1.7320508f        a zero-mean, unit-variance sum of four uniforms;
 *       eps_0 = xi_0,   eps_t = beta * eps_{t-1} + gain * xi_t,        gain = (float)sqrt(1 - (double)beta * beta), formed on the host.
 *   Every operation is one fp32 rounding (no contraction), so NumPy float32 reproduces every bit.
 * Samples. Sample 0 is the nominal tape clamped to [-1, 1] (DAM:128-132 takes raw actions in the box, mpc/main.py:549);
 *   sample s >= 1 is clamp(nominal[t][e][a] + sigma2[a] * eps_t, -1, 1).  The clamp is x < -1 ? -1 : x > 1 ? 1 : x: a NaN stays a NaN.
 * Cost.    cost[s][e] is, bit for bit, what eb_rollout_tape_cand (include/envbuild_cand.h:50-54) returns as `cost` for that tape on
 *   the env's path without retrack: the same rollout, the same per-step order over the non-zero weights, the same ascending-t sum
 *   from +0.
 * Best.    The first minimum over s wins; a NaN never wins; all NaN gives sample 0.  best_cost / best_tape are that sample's bits.
 * Mean.    w_s = exp(-(cost_s - best_cost) * inv_lambda) by a deterministic branch-free exp (csrc/eb_mlp_device.h:exp_det); a NaN
 *   cost, and a weight that is not a number (inf - inf), has weight 0 and its tape is left out.
 *   mean_tape[t][e][a] = clamp(sum_s w_s u_s / sum_s w_s, -1, 1).  The order of the sums is the kernel's own and fixed (two launches
 *   repeat their bits); it is not part of the ABI.  When sum_s w_s is not positive (all costs NaN or infinite) the mean is sample 0.
 * Independence.  An env's outputs depend only on its row, its nominal tape, its path, its id, (seed, counter) and the scalars — not on
 *   the row's position in the batch or on the other rows.
 *
 *   obs0          [n_env, D], shared by the samples; never written;
 *   nominal       [horizon, n_env, 2] raw actions;
 *   ref_idx, path_id   as eb_rollout_tape: one path per env (training: ref_idx[e], an id out of range keeps zero tracking, DAM:342,
 *                 352; selecting: path_id);
 *   sigma2, w5    HOST pointers.
 * Return codes: n_env == 0 or n_samples == 0 is a no-op.  EB_EINVAL, with the reason in eb_last_error: every output NULL;
 * w5 == NULL; sigma2 == NULL or a negative (or NaN) entry; beta outside [0, 1); inv_lambda < 0 or not finite; horizon < 1 or > 128;
 * n_samples above eb_rollout_tape_sample_max, with the limit in eb_last_error; training mode without ref_idx; a path_id out of range
 * in selecting mode. */
int eb_rollout_tape_sample(eb_handle h, int32_t n_env, int32_t n_samples, int32_t horizon,
        const float* obs0,            /* [n_env, D], shared by the samples; never written */
        const float* nominal,         /* [horizon, n_env, 2] raw actions */
        const int32_t* ref_idx, int32_t path_id,      /* as eb_rollout_tape: one path per env */
        const int32_t* env_ids,       /* [n_env] or NULL (= row index): the id that keys an env's noise */
        uint64_t seed, uint64_t counter,
        const float* sigma2,          /* HOST, 2 floats >= 0: per action component */
        float beta,                   /* in [0, 1): AR(1) smoothing of the noise over t; 0 = white */
        float inv_lambda,             /* >= 0: soft-min sharpness; 0 = plain average */
        const float* w5,              /* HOST, 5 floats: cost weights, as eb_rollout_tape_cand */
        float* cost,                  /* [n_samples, n_env] or NULL */
        float* best_tape, float* best_cost, int32_t* best_index,   /* [horizon, n_env, 2], [n_env], [n_env]; each may be NULL */
        float* mean_tape,             /* [horizon, n_env, 2] or NULL */
        float* samples_out,           /* [n_samples, horizon, n_env, 2] or NULL: the tapes as scored (debug / tests) */
        void* stream);

/* The most samples one eb_rollout_tape_sample launch takes on this handle for `horizon` steps (the costs of an env's samples stay in
 * its block's LDS).  At least 1024 for n_veh <= 64 and horizon <= 128. */
int eb_rollout_tape_sample_max(eb_handle h, int32_t horizon, int32_t* max_samples);

#ifdef __cplusplus
}
#endif
#endif /* ENVBUILD_SAMPLE_H */
