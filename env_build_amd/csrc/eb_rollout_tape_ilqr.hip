// eb_rollout_tape_ilqr.hip — one iLQR iteration on the model rollout in ONE launch (eb_rollout_tape_ilqr, include/envbuild_ilqr.h),
// gfx950: try the previous gains at several step lengths, keep the best trajectory, linearise along it, sweep backwards to the
// next gains.  Nothing is read on the host.
//
// A block of 256 threads owns E envs (E = 16, 8 or 4: G = 256 / E >= n_veh threads per env) for the whole launch.
//
//   records      the first E * n_veh threads keep one 16-byte (env, vehicle) record each; per step they publish the PRE-step record
//                as (x, y, sin, cos) to LDS and advance it (eb_rollout_tape_sample.hip's scheme: two buffers, one barrier per step).
//   pass 1       the first 1 + n_alpha threads of an env each roll one candidate out: candidate 0 the clamped nominal, candidate
//                j >= 1 closed-loop under the feedback law (ilqr::feedback_action) — the env's own chain and the env's slots in slot
//                order, which is the summation order of the tape kernels, so cost is eb_rollout_tape_cand's bit for bit.
//   best         thread 0 of the env takes the first minimum of its costs.
//   pass 2       the records restart from obs0; thread 0 of the env rolls the best candidate out again (the same operations, the same
//                bits), writes u_out / x_out and leaves 20 floats per step in LDS: the pre-step ego state, the tracking triple, the
//                action, and the vehicles' part of l_z and of l_zz, both summed in slot order.
//   sweep        thread 0 of the env alone, last step first: ilqr::step_model (ten grad::env_vjp evaluations and the Gauss-Newton
//                terms) and ilqr::riccati_step out of LDS; the symmetric 6 x 6 value matrix lives in registers, in double.
// One thread per env in pass 2 and in the sweep: the launch is latency-bound there, and DESIGN.md §14 says what that costs.
// The closest-point lookup is tape_closest of eb_tape_device.h, shared with the other tape kernels.
// No atomics, no scratch; fp32 state only.
#include <hip/hip_runtime.h>

#include "eb_ilqr.h"
#include "eb_env_device.h"
#include "eb_tape_device.h"
#include "eb_ilqr_device.h"

namespace eb {
namespace {

constexpr int IL_THREADS = 256;

struct IlLane {
    int tid, el, ge, p, roff;
    bool rec_lane;
    int renv, rslot;
    float w5[5];
};

// One rollout of candidate `cand` by the lanes with `act` set, the records restarted from obs0; every thread of the block calls it.
// BACK: the lane also writes u_out / x_out and leaves the sweep's 20 floats per step in tapeL.  -> the candidate's cost.
template <int TASK, bool BACK>
__device__ __forceinline__ float il_rollout(const TapeIlqrArgs& A, const IlLane& L, float4 (&s_rec)[2][IL_THREADS], const unsigned char* s_turn,
                                            bool act, int cand, float* tapeL) {
    const int E = A.envs_per_block, NV = A.n_veh, D = A.obs_dim, nd = A.nd, H = A.horizon;
    const int e0 = blockIdx.x * E;
    const size_t n = (size_t)A.n_env;
    const int ge = L.ge;
    const SinCosK SK = sincos_consts();
    const float* const orow = A.obs0 + (size_t)ge * D;
    f4u rec = f4u{1e30f, 0.0f, 0.0f, 0.0f};
    if (L.rec_lane) rec = *reinterpret_cast<const f4u*>(A.obs0 + (size_t)(e0 + L.renv) * D + nd + 4 * L.rslot);
    float st[6], trk[3];
    {
        const f4u h0 = *reinterpret_cast<const f4u*>(orow), h1 = *reinterpret_cast<const f4u*>(orow + 4);
        st[0] = h0.x; st[1] = h0.y; st[2] = h0.z; st[3] = h0.w; st[4] = h1.x; st[5] = h1.y;
        trk[0] = h1.z; trk[1] = h1.w; trk[2] = orow[8];
    }
    const bool closed = cand > 0;                      // (candidates >= 1 exist only when gains are given)
    float alpha = 0.0f;
#pragma unroll
    for (int k = 0; k < IL_MAX_ALPHA; ++k)
        if (cand == k + 1) alpha = A.alphas[k];
    const float w35 = L.w5[1], w25 = L.w5[2] + L.w5[3];
    const size_t cs = (size_t)H * E;
    float J = 0.0f;

    for (int t = 0; t < H; ++t) {
        float4* const buf = s_rec[t & 1];
        if (L.rec_lane) {
            // predict_record_tc returns sin / cos of the PRE-step heading — the pair the penalty terms need (DAM:221)
            const float px = rec.x, py = rec.y;
            float vs, vc;
            rec = predict_record_tc<float>(rec, turn_consts(s_turn[L.rslot]), SK, vs, vc);
            buf[L.tid] = make_float4(px, py, vs, vc);
        }
        __syncthreads();
        if (act) {
            const f2u nom = *reinterpret_cast<const f2u*>(A.u_nom + 2 * ((size_t)t * n + ge));
            float a0 = ilqr::clamp1(nom.x), a1 = ilqr::clamp1(nom.y);
            if (closed) {
                float g[ilqr::GAIN_ROWS], xn[6];
                const float* gp = A.gains + (size_t)t * ilqr::GAIN_ROWS * n + ge;
                const float* xp = A.x_nom + (size_t)t * 6 * n + ge;
#pragma unroll
                for (int r = 0; r < ilqr::GAIN_ROWS; ++r) g[r] = gp[(size_t)r * n];
#pragma unroll
                for (int c = 0; c < 6; ++c) xn[c] = xp[(size_t)c * n];
                ilqr::feedback_action(alpha, g, st, xn, nom.x, nom.y, a0, a1);
            }
            if (!BACK && A.cand_out) {
                float* o = A.cand_out + 2 * (((size_t)cand * H + t) * n + ge);
                o[0] = a0; o[1] = a1;
            }
            if (BACK) {
                if (A.u_out) { float* o = A.u_out + 2 * ((size_t)t * n + ge); o[0] = a0; o[1] = a1; }
                if (A.x_out) {
                    float* o = A.x_out + (size_t)t * 6 * n + ge;
#pragma unroll
                    for (int c = 0; c < 6; ++c) o[(size_t)c * n] = st[c];
                }
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
            if (L.p >= 0) {                                                 // DAM:334-353
                float rx = 0.0f, ry = 0.0f, rphi = 0.0f;
                tape_closest(A, L.p, L.roff, nx[3], nx[4], rx, ry, rphi);
                t0 = two2one<TASK>(nx[3], nx[4], rx, ry);                   // DAM:758
                t1 = deal_with_phi_diff(nx[5] - rphi);                      // DAM:759
                t2 = nx[0] - EXP_V;                                         // DAM:760
            }
            float road_t = 0.0f, road_r = 0.0f;
            road_terms<TASK>(st[3] + LWS * ec, st[4] + LWS * es, road_t, road_r);   // DAM:231-295
            road_terms<TASK>(st[3] - LWS * ec, st[4] - LWS * es, road_t, road_r);
            // ---- the env's slots in slot order: near records only (DAM:218-229; far records add exact zeros) ----
            const float4 pts = make_float4(st[3] + LWS * ec, st[4] + LWS * es, st[3] - LWS * ec, st[4] - LWS * es);
            const float4* const rb = buf + L.el * NV;
            float a35 = 0.0f, a25 = 0.0f;
            float ppx = 0.0f, ppy = 0.0f, ppphi = 0.0f;
            float hv[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            for (int k = 0; k < NV; ++k) {
                const float4 v = rb[k];
                if (grad::record_near(st[3], st[4], v.x, v.y)) {
                    float t35[4], t25[4];
                    veh2veh_terms(pts, v.x, v.y, v.z, v.w, t35, t25);
                    a35 += ((t35[0] + t35[1]) + t35[2]) + t35[3];
                    a25 += ((t25[0] + t25[1]) + t25[2]) + t25[3];
                    if (BACK) {
                        float qx, qy, qphi;
                        grad::record_partials(st[3], st[4], es, ec, v.x, v.y, v.z, v.w, w35, w25, qx, qy, qphi);
                        ppx += qx; ppy += qy; ppphi += qphi;
                        ilqr::veh_pair_gn(st[3], st[4], es, ec, v.x, v.y, v.z, v.w, w35, w25, hv);
                    }
                }
            }
            const float o1 = a35 + road_t, o2 = a25 + road_r;               // DAM:299-300
            // s_t: the rows with a non-zero weight, in row order; J: ascending t from +0 (include/envbuild_cand.h)
            float sum = 0.0f;
            bool any = false;
            if (L.w5[0] != 0.0f) { sum = rew * L.w5[0]; any = true; }
            if (L.w5[1] != 0.0f) { const float v = o1 * L.w5[1]; sum = any ? sum + v : v; any = true; }
            if (L.w5[2] != 0.0f) { const float v = o2 * L.w5[2]; sum = any ? sum + v : v; any = true; }
            if (L.w5[3] != 0.0f) { const float v = a25 * L.w5[3]; sum = any ? sum + v : v; any = true; }
            if (L.w5[4] != 0.0f) { const float v = road_r * L.w5[4]; sum = any ? sum + v : v; any = true; }
            if (any) J += sum;
            if (BACK) {
                float* T = tapeL + (size_t)t * E + L.el;
#pragma unroll
                for (int c = 0; c < 6; ++c) T[c * cs] = st[c];
#pragma unroll
                for (int c = 0; c < 3; ++c) T[(6 + c) * cs] = trk[c];
                T[9 * cs] = a0; T[10 * cs] = a1;
                T[11 * cs] = ppx; T[12 * cs] = ppy; T[13 * cs] = ppphi;
#pragma unroll
                for (int c = 0; c < 6; ++c) T[(14 + c) * cs] = hv[c];
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) st[c] = nx[c];
            trk[0] = t0; trk[1] = t1; trk[2] = t2;
        }
        // (step t + 1 writes the other buffer; step t + 2 writes this one after the barrier of step t + 1, which a lane passes only
        //  when it is through with this step's reads)
    }
    return J;
}

template <int TASK>
__global__ __launch_bounds__(IL_THREADS) void rollout_tape_ilqr_kernel(const TapeIlqrArgs A) {
    __shared__ float4 s_rec[2][IL_THREADS];            // x, y, sin, cos of the pre-step record of (env, slot)
    __shared__ float s_cost[IL_THREADS];               // (env, candidate) at env * G + candidate
    __shared__ unsigned char s_turn[64];
    extern __shared__ __align__(16) float il_tape[];   // [20][H][E]: what pass 2 leaves for the sweep
    const int tid = threadIdx.x;
    const int E = A.envs_per_block, H = A.horizon, K1 = 1 + A.n_alpha;
    const int G = IL_THREADS / E;                      // threads per env: >= n_veh and >= 8
    IlLane L;
    L.tid = tid;
    L.el = tid / G;
    const int j = tid - L.el * G;
    const int e0 = blockIdx.x * E, nE = min(E, A.n_env - e0);
    const bool env_ok = L.el < nE;
    L.ge = e0 + (env_ok ? L.el : 0);                   // idle env slots shadow the block's first env (in bounds), store nothing
    const int ge = L.ge;
    const size_t n = (size_t)A.n_env;
    // (read once, up front: a select between a global load and a member of the argument block would put the block in scratch)
    L.w5[0] = A.w5[0]; L.w5[1] = A.w5[1]; L.w5[2] = A.w5[2]; L.w5[3] = A.w5[3]; L.w5[4] = A.w5[4];
    L.rec_lane = tid < nE * A.n_veh;                   // E * n_veh <= 256
    L.renv = L.rec_lane ? tid / A.n_veh : 0;
    L.rslot = L.rec_lane ? tid - L.renv * A.n_veh : 0;
    if (tid < 64) s_turn[tid] = A.dt->turn[tid];
    L.p = A.path_id;
    if (A.training) {
        const int pr = A.ref_idx[ge];
        L.p = (pr >= 0 && pr < A.n_paths) ? pr : -1;                            // DAM:342, 352
    }
    L.roff = L.p == 1 ? A.red_off[1] : L.p == 2 ? A.red_off[2] : A.red_off[0];
    __syncthreads();

    // ---- pass 1: every candidate ----
    const bool act1 = env_ok && j < K1;
    const float J = il_rollout<TASK, false>(A, L, s_rec, s_turn, act1, j < K1 ? j : 0, nullptr);
    s_cost[tid] = J;
    if (act1 && A.cost) A.cost[(size_t)j * n + ge] = J;
    __syncthreads();                                   // the costs are visible; pass 2's step 0 writes record buffer 0 again

    // ---- the first minimum per env: a NaN counts +inf, ties go to the lower index (mpc.first_minimum) ----
    int best = 0;
    if (j == 0) {
        float bv = __builtin_inff();
        for (int k = 0; k < K1; ++k) {
            const float c = s_cost[L.el * G + k];
            if (c < bv) { bv = c; best = k; }          // strict; false for a NaN; all NaN leaves candidate 0
        }
        if (env_ok && A.best_index) A.best_index[ge] = best;
        if (env_ok && A.best_cost) A.best_cost[ge] = s_cost[L.el * G + best];
    }
    const bool back = A.gains_out != nullptr || A.dv != nullptr || A.lq_out != nullptr;
    if (!back && !A.u_out && !A.x_out) return;         // block-uniform

    // ---- pass 2: the best candidate again; u_out, x_out, the sweep's tape ----
    const bool act2 = env_ok && j == 0;
    il_rollout<TASK, true>(A, L, s_rec, s_turn, act2, best, il_tape);
    if (!back || !act2) return;

    // ---- the backward sweep: thread 0 of the env alone, out of LDS (it reads what it wrote itself) ----
    const size_t cs = (size_t)H * E;
    const float mu = A.mu ? A.mu[ge] : 0.0f;
    const bool sweep = A.gains_out != nullptr || A.dv != nullptr;
    float* const lq = A.lq_out;
    ilqr::Value V;
    ilqr::value_zero(V);
    ilqr::acc_t dv1 = 0.0, dv2 = 0.0;
    for (int t = H - 1; t >= 0; --t) {
        const float* T = il_tape + (size_t)t * E + L.el;
        ilqr::StepIn S;
#pragma unroll
        for (int c = 0; c < 6; ++c) S.st[c] = T[c * cs];
#pragma unroll
        for (int c = 0; c < 3; ++c) S.trk[c] = T[(6 + c) * cs];
        S.a0 = T[9 * cs]; S.a1 = T[10 * cs];
        S.px = T[11 * cs]; S.py = T[12 * cs]; S.pphi = T[13 * cs];
#pragma unroll
        for (int c = 0; c < 6; ++c) S.hv[c] = T[(14 + c) * cs];
        S.has_path = L.p >= 0;
        float* const lqt = lq ? lq + (size_t)t * ilqr::LQ_ROWS * n + ge : nullptr;
        ilqr::StepLQ M;
        ilqr::step_model<TASK>(S, L.w5, M, [=](int i, float a6, float a7, float a8) {
            if (lqt && i < 9) { lqt[(size_t)(9 * i + 6) * n] = a6; lqt[(size_t)(9 * i + 7) * n] = a7; lqt[(size_t)(9 * i + 8) * n] = a8; }
        });
        if (lqt) {
#pragma unroll
            for (int i = 0; i < 9; ++i) {
#pragma unroll
                for (int c = 0; c < 6; ++c) lqt[(size_t)(9 * i + c) * n] = M.F[i][c];
                lqt[(size_t)(81 + 2 * i) * n] = M.F[i][6];
                lqt[(size_t)(82 + 2 * i) * n] = M.F[i][7];
                lqt[(size_t)(99 + i) * n] = M.lz[i];
            }
            lqt[(size_t)108 * n] = M.lu[0]; lqt[(size_t)109 * n] = M.lu[1];
#pragma unroll
            for (int k = 0; k < 45; ++k) lqt[(size_t)(110 + k) * n] = 0.0f;
            lqt[(size_t)(110 + ilqr::tri<9>(2, 2)) * n] = M.h22;
            lqt[(size_t)(110 + ilqr::tri<9>(3, 3)) * n] = M.hp[0]; lqt[(size_t)(110 + ilqr::tri<9>(3, 4)) * n] = M.hp[1];
            lqt[(size_t)(110 + ilqr::tri<9>(3, 5)) * n] = M.hp[2]; lqt[(size_t)(110 + ilqr::tri<9>(4, 4)) * n] = M.hp[3];
            lqt[(size_t)(110 + ilqr::tri<9>(4, 5)) * n] = M.hp[4]; lqt[(size_t)(110 + ilqr::tri<9>(5, 5)) * n] = M.hp[5];
            lqt[(size_t)(110 + ilqr::tri<9>(6, 6)) * n] = M.hd[0]; lqt[(size_t)(110 + ilqr::tri<9>(7, 7)) * n] = M.hd[1];
            lqt[(size_t)(110 + ilqr::tri<9>(8, 8)) * n] = M.hd[2];
            lqt[(size_t)155 * n] = M.luu[0]; lqt[(size_t)156 * n] = M.luu[1];
        }
        if (sweep) {
            float g[ilqr::GAIN_ROWS];
            ilqr::acc_t d1, d2;
            ilqr::riccati_step(M, mu, S.a0, S.a1, V, g, d1, d2);
            dv1 += d1; dv2 += d2;
            if (A.gains_out) {
                float* o = A.gains_out + (size_t)t * ilqr::GAIN_ROWS * n + ge;
#pragma unroll
                for (int r = 0; r < ilqr::GAIN_ROWS; ++r) o[(size_t)r * n] = g[r];
            }
        }
    }
    if (A.dv) { A.dv[ge] = (float)dv1; A.dv[n + ge] = (float)dv2; }
}

inline int il_envs_per_block(int n_veh) {
    int G = 16;
    while (G < n_veh) G <<= 1;
    return IL_THREADS / G;
}

}  // namespace

hipError_t launch_rollout_tape_ilqr(int task, const TapeIlqrArgs& A_in, hipStream_t s) {
    if (A_in.n_env <= 0) return hipSuccess;
    if (A_in.n_alpha < 0 || A_in.n_alpha > IL_MAX_ALPHA || A_in.n_veh > 64 || A_in.horizon < 1 || A_in.horizon > IL_MAX_HORIZON)
        return hipErrorInvalidValue;
    TapeIlqrArgs A = A_in;
    A.envs_per_block = il_envs_per_block(A.n_veh);
    const int grid = (A.n_env + A.envs_per_block - 1) / A.envs_per_block;
    const bool pass2 = A.gains_out || A.dv || A.lq_out || A.u_out || A.x_out;   // pass 2 writes the sweep's tape whenever it runs
    const size_t lds = pass2 ? sizeof(float) * (size_t)ilqr::TAPE_FLOATS * A.horizon * A.envs_per_block : 0;
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        return launch_lds<rollout_tape_ilqr_kernel<decltype(t)::value>>(dim3(grid), dim3(IL_THREADS), lds, dev, s, A);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
