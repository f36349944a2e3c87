// eb_rollout_tape_sample.hip — S perturbed open-loop action tapes per env drawn, rolled out, scored and averaged in ONE launch
// (eb_rollout_tape_sample, include/envbuild_sample.h), gfx950.  The inner step of a sampling MPC (MPPI / CEM).
//
// Two facts make it cheap:
//   - the vehicles do not depend on the ego (stop_gradient, DAM:195, 331, 402): a scene's records (predict_for_a_mode, DAM:405-427)
//     advance the same way under every sample and are advanced ONCE per env and step, whatever S is;
//   - the perturbations are a pure function of a counter (splitmix64 / u01, eb_env_device.h:253-262), so a tape never exists in
//     memory: it is drawn when it is rolled out and drawn again when it is averaged.
// A wave is (one env, 64 consecutive samples); a block of 256 threads carries four such waves: four envs for S <= 64, two for
// S <= 128, one for S <= 256, and for S > 256 one env whose samples are taken in ceil(S / 256) rounds, each restarting the records
// from obs0.  All samples of an env stay in one block, so the reduction never leaves it.
//
//   records      the first E * n_veh threads keep one 16-byte (env, vehicle) record each; per step they publish the PRE-step record
//                as (x, y, sin, cos) to LDS — the heading's sin / cos is formed once per record and step, not once per near pair —
//                and advance it.  Two LDS buffers, so one barrier per step suffices.
//   sample lane  per step: its noise from the counter (eps carried in registers), the env's own chain (action transform, rewards,
//                bicycle step, closest point, tracking, walls: eb_rollout_tape_cand.hip's), then the env's slots in slot order —
//                every lane of a wave reads the same LDS address, a broadcast — with grad::record_near and veh2veh_terms for the
//                near ones, each record's four-term partial added in slot order.  That is the summation order of the tape kernels,
//                so cost is eb_rollout_tape_cand's bit for bit without a queue, a ballot or a per-(env, candidate, slot) table.
//   afterwards   the costs go to LDS; a fixed-order reduction per env gives the first minimum; then the samples are drawn again and
//                sum_s w_s u_s is formed per tape entry: a butterfly over the wave, one LDS slot per wave and entry, the waves of
//                an env added in wave order.
// The closest-point lookup is tape_closest of eb_tape_device.h, shared with the other tape kernels.
// No atomics, no scratch; fp32 state only.
#include <hip/hip_runtime.h>

#include "eb_sample.h"
#include "eb_env_device.h"
#include "eb_mlp_device.h"
#include "eb_tape_device.h"
#include "eb_tape_grad_device.h"

namespace eb {
namespace {

constexpr int TS_THREADS = 256;

// the soft-min weight of a sample (include/envbuild_sample.h): a NaN cost and a weight that is not a number count 0
__device__ __forceinline__ float ts_weight(float c, float best, float inv_lambda) {
    const float w = mlp::exp_det((-(c - best)) * inv_lambda);
    return (c == c && w == w) ? w : 0.0f;
}

// one unit-variance draw: four uniforms of the counter (include/envbuild_sample.h)
__device__ __forceinline__ float ts_xi(uint64_t key, uint64_t idx) {
    const float u0 = u01(key, idx), u1 = u01(key, idx + 1), u2 = u01(key, idx + 2), u3 = u01(key, idx + 3);
    return (((u0 + u1) + (u2 + u3)) - 2.0f) * 1.7320508f;
}

__device__ __forceinline__ float ts_clamp(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }   // a NaN stays a NaN

// the action of sample s at step t: the AR(1) state (e0, e1) advances by one step
struct TsNoise { uint64_t key, row; float sigma0, sigma1, beta, gain; int H; };
__device__ __forceinline__ void ts_action(const TsNoise& N, int s, int t, float n0, float n1, float& e0, float& e1, float& u0, float& u1) {
    if (s > 0) {
        const uint64_t idx = 8ull * ((uint64_t)t + (uint64_t)N.H * N.row);
        const float x0 = ts_xi(N.key, idx), x1 = ts_xi(N.key, idx + 4);
        e0 = t == 0 ? x0 : N.beta * e0 + N.gain * x0;
        e1 = t == 0 ? x1 : N.beta * e1 + N.gain * x1;
        n0 = n0 + N.sigma0 * e0;
        n1 = n1 + N.sigma1 * e1;
    }
    u0 = ts_clamp(n0); u1 = ts_clamp(n1);
}

__device__ __forceinline__ float ts_wave_sum(float v) {                  // a butterfly: the same order on every launch
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <int TASK>
__global__ __launch_bounds__(TS_THREADS) void rollout_tape_sample_kernel(const TapeSampleArgs A) {
    __shared__ float4 s_rec[2][TS_THREADS];            // x, y, sin, cos of the pre-step record of (env, slot)
    __shared__ float s_acc[4][2 * TS_MAX_HORIZON];     // per wave: sum_s w_s u_s of every tape entry
    __shared__ float s_wsum[4];
    __shared__ float s_redv[TS_THREADS];
    __shared__ int s_redi[TS_THREADS];
    __shared__ float s_bcost[4];
    __shared__ int s_bidx[4];
    __shared__ unsigned char s_turn[64];
    extern __shared__ __align__(16) float ts_cost[];   // max(256, S) costs: (env, sample) at env * G + sample
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int E = A.envs_per_block, NV = A.n_veh, D = A.obs_dim, nd = A.nd, H = A.horizon, S = A.n_samples;
    const int G = TS_THREADS / E, WPE = 4 / E;         // threads and waves per env; E is 4, 2 or 1
    const int el = tid / G, j = tid - el * G;
    const int e0 = blockIdx.x * E, nE = min(E, A.n_env - e0);
    const bool env_ok = el < nE;
    const int ge = e0 + (env_ok ? el : 0);             // idle env slots shadow the block's first env (in bounds), store nothing
    const size_t n = (size_t)A.n_env;
    const int rounds = E == 1 ? (S + TS_THREADS - 1) / TS_THREADS : 1;
    // (read once, up front: a select between a global load and a member of the argument block would put the block in scratch)
    const float w5_0 = A.w5[0], w5_1 = A.w5[1], w5_2 = A.w5[2], w5_3 = A.w5[3], w5_4 = A.w5[4];

    const bool rec_lane = tid < nE * NV;               // E * n_veh <= 256
    const int renv = rec_lane ? tid / NV : 0, rslot = rec_lane ? tid - renv * NV : 0;
    if (tid < 64) s_turn[tid] = A.dt->turn[tid];
    const SinCosK SK = sincos_consts();

    TsNoise N;
    N.key = splitmix64(A.seed + 0x9E3779B97F4A7C15ull * A.counter);
    N.sigma0 = A.sigma0; N.sigma1 = A.sigma1; N.beta = A.beta; N.gain = A.gain; N.H = H;
    const uint64_t id = (uint64_t)(uint32_t)(A.env_ids ? A.env_ids[ge] : ge);

    int p = A.path_id;
    if (A.training) {
        const int pr = A.ref_idx[ge];
        p = (pr >= 0 && pr < A.n_paths) ? pr : -1;                              // DAM:342, 352
    }
    const int roff = p == 1 ? A.red_off[1] : p == 2 ? A.red_off[2] : A.red_off[0];
    const float* const orow = A.obs0 + (size_t)ge * D;
    __syncthreads();

    for (int r = 0; r < rounds; ++r) {
        const int s = r * G + j;
        const bool act = env_ok && s < S;
        N.row = id * (uint64_t)S + (uint64_t)s;
        f4u rec = f4u{1e30f, 0.0f, 0.0f, 0.0f};
        if (rec_lane) rec = *reinterpret_cast<const f4u*>(A.obs0 + (size_t)(e0 + renv) * D + nd + 4 * rslot);
        float st[6], trk[3];
        {
            const f4u h0 = *reinterpret_cast<const f4u*>(orow), h1 = *reinterpret_cast<const f4u*>(orow + 4);
            st[0] = h0.x; st[1] = h0.y; st[2] = h0.z; st[3] = h0.w; st[4] = h1.x; st[5] = h1.y;
            trk[0] = h1.z; trk[1] = h1.w; trk[2] = orow[8];
        }
        float eps0 = 0.0f, eps1 = 0.0f, J = 0.0f;

        for (int t = 0; t < H; ++t) {
            float4* const buf = s_rec[t & 1];
            if (rec_lane) {
                // predict_record_tc returns sin / cos of the PRE-step heading — the operations of sincos_det(deg2rad(rec.w)), the pair
                // the penalty terms need (DAM:221): one evaluation per record and step serves both
                const float px = rec.x, py = rec.y;
                float vs, vc;
                rec = predict_record_tc<float>(rec, turn_consts(s_turn[rslot]), SK, vs, vc);
                buf[tid] = make_float4(px, py, vs, vc);
            }
            __syncthreads();
            if (act) {
                const f2u nom = *reinterpret_cast<const f2u*>(A.nominal + 2 * ((size_t)t * n + ge));
                float a0, a1;
                ts_action(N, s, t, nom.x, nom.y, eps0, eps1, a0, a1);
                if (A.samples_out) {
                    float* o = A.samples_out + 2 * (((size_t)s * H + t) * n + ge);
                    o[0] = a0; o[1] = a1;
                }
                // ---- the env's own chain: eb_rollout_tape_cand.hip's ----
                const float phi_rad = deg2rad(st[5]);
                float es, ec;
                sincos_det(phi_rad, es, ec);                                    // DAM:211 and DAM:79-80
                float steer, a_x;
                action_transform(a0, a1, steer, a_x);                           // DAM:120
                const float punish_steer = -sq(steer), punish_a_x = -sq(a_x);   // DAM:198-199
                const float punish_yaw_rate = -sq(st[2]);                       // DAM:202
                const float devi_y = -sq(trk[0]);                               // DAM:205
                const float devi_phi = -sq(deg2rad(trk[1]));                    // DAM:206
                const float devi_v = -sq(trk[2]);                               // DAM:207
                const float rew = 0.05f * devi_v + 0.8f * devi_y + 30.0f * devi_phi + 0.02f * punish_yaw_rate + 5.0f * punish_steer +
                                  0.05f * punish_a_x;                           // DAM:297-298
                float nx[6];
                f_xu_core(st, steer, a_x, TAU10, phi_rad, es, ec, nx);          // DAM:387
                nx[0] = __builtin_fminf(__builtin_fmaxf(nx[0], 0.0f), 35.0f);   // DAM:390
                float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
                if (p >= 0) {                                                   // DAM:334-353
                    float rx = 0.0f, ry = 0.0f, rphi = 0.0f;
                    tape_closest(A, p, roff, nx[3], nx[4], rx, ry, rphi);
                    t0 = two2one<TASK>(nx[3], nx[4], rx, ry);                   // DAM:758
                    t1 = deal_with_phi_diff(nx[5] - rphi);                      // DAM:759
                    t2 = nx[0] - EXP_V;                                         // DAM:760
                }
                float road_t = 0.0f, road_r = 0.0f;
                road_terms<TASK>(st[3] + LWS * ec, st[4] + LWS * es, road_t, road_r);   // DAM:231-295
                road_terms<TASK>(st[3] - LWS * ec, st[4] - LWS * es, road_t, road_r);
                // ---- the env's slots in slot order: near records only (DAM:218-229; far records add exact zeros) ----
                const float4 pts = make_float4(st[3] + LWS * ec, st[4] + LWS * es, st[3] - LWS * ec, st[4] - LWS * es);
                const float4* const rb = buf + el * NV;
                float a35 = 0.0f, a25 = 0.0f;
                for (int k = 0; k < NV; ++k) {
                    const float4 v = rb[k];                                     // one address per wave: a broadcast
                    if (grad::record_near(st[3], st[4], v.x, v.y)) {
                        float t35[4], t25[4];
                        veh2veh_terms(pts, v.x, v.y, v.z, v.w, t35, t25);
                        a35 += ((t35[0] + t35[1]) + t35[2]) + t35[3];
                        a25 += ((t25[0] + t25[1]) + t25[2]) + t25[3];
                    }
                }
                const float o1 = a35 + road_t, o2 = a25 + road_r;               // DAM:299-300
                // s_t: the rows with a non-zero weight, in row order; J: ascending t from +0 (include/envbuild_cand.h)
                float sum = 0.0f;
                bool any = false;
                if (w5_0 != 0.0f) { sum = rew * w5_0; any = true; }
                if (w5_1 != 0.0f) { const float v = o1 * w5_1; sum = any ? sum + v : v; any = true; }
                if (w5_2 != 0.0f) { const float v = o2 * w5_2; sum = any ? sum + v : v; any = true; }
                if (w5_3 != 0.0f) { const float v = a25 * w5_3; sum = any ? sum + v : v; any = true; }
                if (w5_4 != 0.0f) { const float v = road_r * w5_4; sum = any ? sum + v : v; any = true; }
                if (any) J += sum;
#pragma unroll
                for (int c = 0; c < 6; ++c) st[c] = nx[c];
                trk[0] = t0; trk[1] = t1; trk[2] = t2;
            }
            // (step t + 1 writes the other buffer; step t + 2 writes this one after the barrier of step t + 1, which a lane passes
            //  only when it is through with this step's reads)
        }
        if (s < S) ts_cost[el * G + s] = J;            // (an idle env slot's entries are read by nobody who stores)
        if (act && A.cost) A.cost[(size_t)s * n + ge] = J;
        __syncthreads();                               // the next round's step 0 writes buffer 0 again; the costs are visible
    }

    // ---- the first minimum per env: a NaN counts +inf, ties go to the lower index (mpc.first_minimum) ----
    float bv = __builtin_inff();
    int bi = 0x7fffffff;
    for (int s = j; s < S; s += G) {
        const float c = ts_cost[el * G + s];
        const float v = c == c ? c : __builtin_inff();
        if (s == j || v < bv) { bv = v; bi = s; }
    }
    s_redv[tid] = bv; s_redi[tid] = bi;
    __syncthreads();
    for (int off = G >> 1; off > 0; off >>= 1) {
        if (j < off) {
            const float ov = s_redv[tid + off];
            const int oi = s_redi[tid + off];
            if (ov < bv || (ov == bv && oi < bi)) { bv = ov; bi = oi; }
            s_redv[tid] = bv; s_redi[tid] = bi;
        }
        __syncthreads();
    }
    if (j == 0) {                                      // sample 0 exists, so bi is a sample
        const float bc = ts_cost[el * G + bi];         // that sample's bits (a NaN when every cost is one)
        s_bidx[el] = bi; s_bcost[el] = bc;
        if (env_ok && A.best_cost) A.best_cost[ge] = bc;
        if (env_ok && A.best_index) A.best_index[ge] = bi;
    }
    if (!A.mean_tape && !A.best_tape) return;          // block-uniform
    for (int i = lane; i < 2 * H; i += 64) s_acc[wave][i] = 0.0f;
    if (lane == 0) s_wsum[wave] = 0.0f;
    __syncthreads();

    // ---- the samples again, from the counter: sum_s w_s u_s per tape entry; the best sample's tape ----
    const int best_s = s_bidx[el];
    const float best_c = s_bcost[el];
    for (int r = 0; r < rounds; ++r) {
        const int s = r * G + j;
        const bool valid = s < S;
        N.row = id * (uint64_t)S + (uint64_t)s;
        const float w = valid ? ts_weight(ts_cost[el * G + (valid ? s : 0)], best_c, A.inv_lambda) : 0.0f;
        const bool is_best = valid && env_ok && s == best_s && A.best_tape != nullptr;
        float eps0 = 0.0f, eps1 = 0.0f;
        for (int t = 0; t < H; ++t) {
            const f2u nom = *reinterpret_cast<const f2u*>(A.nominal + 2 * ((size_t)t * n + ge));
            float u0 = 0.0f, u1 = 0.0f;
            if (valid) ts_action(N, s, t, nom.x, nom.y, eps0, eps1, u0, u1);
            if (is_best) {
                float* o = A.best_tape + 2 * ((size_t)t * n + ge);
                o[0] = u0; o[1] = u1;
            }
            const float p0 = ts_wave_sum(w > 0.0f ? w * u0 : 0.0f);            // a sample of weight 0 is left out, NaN tape or not
            const float p1 = ts_wave_sum(w > 0.0f ? w * u1 : 0.0f);
            if (lane == 0) { s_acc[wave][2 * t] += p0; s_acc[wave][2 * t + 1] += p1; }
        }
        const float ws = ts_wave_sum(w);
        if (lane == 0) s_wsum[wave] += ws;
    }
    __syncthreads();
    if (env_ok && A.mean_tape) {
        float W = s_wsum[el * WPE];
        for (int k = 1; k < WPE; ++k) W += s_wsum[el * WPE + k];
        for (int i = j; i < 2 * H; i += G) {
            float acc = s_acc[el * WPE][i];
            for (int k = 1; k < WPE; ++k) acc += s_acc[el * WPE + k][i];
            const size_t at = 2 * ((size_t)(i >> 1) * n + ge) + (i & 1);
            A.mean_tape[at] = W > 0.0f ? ts_clamp(acc / W) : ts_clamp(A.nominal[at]);   // no finite cost: sample 0
        }
    }
}

}  // namespace

hipError_t launch_rollout_tape_sample(int task, const TapeSampleArgs& A_in, hipStream_t s) {
    if (A_in.n_env <= 0 || A_in.n_samples <= 0) return hipSuccess;
    if (A_in.n_samples > TS_MAX_SAMPLES || A_in.n_veh > 64 || A_in.horizon > TS_MAX_HORIZON) return hipErrorInvalidValue;
    TapeSampleArgs A = A_in;
    A.envs_per_block = A.n_samples <= 64 ? 4 : A.n_samples <= 128 ? 2 : 1;
    const int grid = (A.n_env + A.envs_per_block - 1) / A.envs_per_block;
    const size_t lds = sizeof(float) * (size_t)(A.n_samples > TS_THREADS ? A.n_samples : TS_THREADS);
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        return launch_lds<rollout_tape_sample_kernel<decltype(t)::value>>(dim3(grid), dim3(TS_THREADS), lds, dev, s, A);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
