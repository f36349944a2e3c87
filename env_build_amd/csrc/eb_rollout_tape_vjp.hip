// eb_rollout_tape_vjp.hip — value and gradient of an open-loop rollout (eb_rollout_tape_vjp) in ONE launch, gfx950.
//
// J-type costs of an MPC caller are sums over the H steps of a tape; their gradient with respect to the tape is what a solver asks
// for tens of times per control step.  Composed from per-step launches that is H forward launches storing every pre-step obs and H
// reverse launches reading them back.  Here a block of 256 threads owns E consecutive envs (E = 32, 16 or 8) for the whole horizon:
//
//   records    every lane keeps up to RPT 16-byte (env, vehicle) records in registers and advances them step by step
//              (predict_for_a_mode, DAM:405-427) — the forward sweep of the tape kernel; records never run backwards;
//   per step t   (A) the env lanes (thread e < E) publish the ego pose (x, y, sin, cos) and the step's two penalty cotangents to LDS;
//              (B) every lane tests its records against the pose: a record whose centre is within 6.31 m (DAM:228: no circle pair
//                  is within 3.5 m otherwise) goes into the block's queue in LDS (ballot + one LDS add per wave), its queue position
//                  into a per-(env, slot) table, its bit into the env's slot mask; then the lane predicts its records;
//              (C) waves 1..3 take the queue, one entry per thread: the forward's penalty terms (DAM:218-229) and, scaled by the
//                  step's cotangents — known at launch, which is why this works in the forward direction — the record's three ego
//                  partials (x, y, heading); meanwhile the env lanes run the env's own forward chain (rewards, bicycle step,
//                  closest point, tracking, walls);
//              (D) the env lanes sum penalties and partials in SLOT order (the mask's bits, lowest first), write the step's out5
//                  and leave 12 floats in the LDS tape: pre-step ego state (6), tracking triple (3), the three partial sums;
//   reverse    after the last step the env lanes alone run grad::tape_reverse (eb_tape_grad_device.h) out of LDS: closed-form f_xu
//              transpose, clip, tracking, walls, rewards and action transform of eb_grad_device.h, last step first.
//
// Forward arithmetic and order are those of eb_rollout.hip's tape kernel (the pieces that live in that translation unit and not in a
// header — the head row, the queue's penalty sums — are restated here; closest_cell_index<0, false> is restated once for the whole
// tape family, as tape_closest in eb_tape_device.h; tests/test_gpu_tape_grad.py holds them to the original bit for bit).  Reverse arithmetic is that of eb_rollout_vjp.hip.  The queue's order varies from run to
// run; the sums do not.  A row's bits depend on nothing but the row.  No atomics to global memory, no scratch; fp32 state only.
#include <hip/hip_runtime.h>

#include "eb_grad.h"
#include "eb_tape_device.h"
#include "eb_tape_grad_device.h"

namespace eb {
namespace {

constexpr int TV_THREADS = 256;
constexpr int TV_TAPE_FLOATS = 12;                      // floats per env-step in the LDS tape
constexpr size_t TV_LDS_BUDGET = 64 * 1024;             // dynamic LDS per block: two blocks per CU at least
constexpr int TV_MAX_HORIZON = 128;
constexpr int TV_RPT_MAX = 4;                           // records a lane keeps in registers: a tile holds at most 1024

struct TvSmem {
    float4 ego[32];                       // x, y, sin phi, cos phi of the pre-step pose
    float2 w[32];                         // cotangents of the step's 3.5 m and 2.5 m penalty sums
    unsigned long long mask[32];          // per env: slots with a near record
    unsigned char turn[64];               // TURN_* per slot
    int count;                            // entries in the near-record queue
};
// dynamic LDS: [tape: 12 x horizon x E floats (gradient form only)] [queue: E * n_veh float4] [2.5 m sums: E * n_veh floats]
// [queue position of every (env, slot): 16 bits each]
inline size_t tv_queue_bytes(int E, int n_veh) { return (size_t)E * n_veh * (sizeof(float4) + sizeof(float) + sizeof(unsigned short)); }
inline size_t tv_lds_bytes(int E, int n_veh, int horizon, bool grad) {
    return tv_queue_bytes(E, n_veh) + (grad ? (size_t)TV_TAPE_FLOATS * horizon * E * sizeof(float) : 0);
}

template <int TASK, int RPT, bool GRAD>
__global__ __launch_bounds__(TV_THREADS, 3) void rollout_tape_vjp_kernel(const TapeVjpArgs A) {
    __shared__ TvSmem S;
    extern __shared__ __align__(16) unsigned char tv_dyn[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int E = A.envs_per_tile, NV = A.n_veh, D = A.obs_dim, nd = A.nd, H = A.horizon;
    const int e0 = blockIdx.x * E, nE = min(E, A.n_env - e0), items = nE * NV;
    const size_t n = (size_t)A.n_env;
    // (read once, up front: a select between a global load and a member of the argument block would put the block in scratch)
    const float w5_0 = A.w5[0], w5_1 = A.w5[1], w5_2 = A.w5[2], w5_3 = A.w5[3], w5_4 = A.w5[4];
    float* const tapeL = reinterpret_cast<float*>(tv_dyn);                      // [12][H][E]
    unsigned char* const qbase = tv_dyn + (GRAD ? (size_t)TV_TAPE_FLOATS * H * E * sizeof(float) : 0);
    float4* const queue = reinterpret_cast<float4*>(qbase);
    float* const q25 = reinterpret_cast<float*>(qbase + (size_t)E * NV * sizeof(float4));
    unsigned short* const qpos = reinterpret_cast<unsigned short*>(qbase + (size_t)E * NV * (sizeof(float4) + sizeof(float)));

    // ---- the block's records: item = k * 256 + tid -> (env, slot); requested before anything else ----
    f4u rec[RPT];
    int where[RPT];                                      // env | slot << 8 of record k
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int item = k * TV_THREADS + tid;
        const bool valid = item < items;
        const int env = valid ? item / NV : 0, slot = valid ? item - env * NV : 0;
        where[k] = env | slot << 8;
        rec[k] = *reinterpret_cast<const f4u*>(A.obs0 + (size_t)(e0 + env) * D + nd + 4 * slot);
        if (!valid) rec[k].x = 1e30f;                    // never near an ego, never predicted, never stored
    }
    if (tid < 64) S.turn[tid] = A.dt->turn[tid];
    const SinCosK SK = sincos_consts();

    // ---- the env lanes' state ----
    const bool env_lane = tid < E, act = tid < nE;
    const int ge = e0 + (act ? tid : 0);                 // idle lanes shadow the tile's first env (in bounds), store nothing
    float st[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, trk[3] = {0.0f, 0.0f, 0.0f};
    int p = -1, roff = 0;
    f2u araw = f2u{0.0f, 0.0f};
    if (env_lane) {
        const float* o = A.obs0 + (size_t)ge * D;
        const f4u h0 = *reinterpret_cast<const f4u*>(o), h1 = *reinterpret_cast<const f4u*>(o + 4);
        st[0] = h0.x; st[1] = h0.y; st[2] = h0.z; st[3] = h0.w; st[4] = h1.x; st[5] = h1.y;
        trk[0] = h1.z; trk[1] = h1.w; trk[2] = o[8];
        p = A.path_id;
        if (A.training) {
            const int pr = A.ref_idx[ge];
            p = (pr >= 0 && pr < A.n_paths) ? pr : -1;                          // DAM:342, 352
        }
        roff = p == 1 ? A.red_off[1] : p == 2 ? A.red_off[2] : A.red_off[0];
        araw = *reinterpret_cast<const f2u*>(A.tape + 2 * (size_t)ge);
    }
    float hv[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    int bi = 0;

    for (int t = 0; t < H; ++t) {
        // ---- (A) env lanes: the pose and the step's penalty cotangents ----
        float es = 0.0f, ec = 0.0f, phi_rad = 0.0f;
        f2u araw_next = araw;
        if (env_lane) {
            if (t + 1 < H) araw_next = *reinterpret_cast<const f2u*>(A.tape + 2 * ((size_t)(t + 1) * n + ge));   // prefetch
            phi_rad = deg2rad(st[5]);
            sincos_det(phi_rad, es, ec);                                        // DAM:211 and DAM:79-80
            S.ego[tid] = make_float4(st[3], st[4], es, ec);
            if (GRAD) {
                const float* g5 = A.g_out5_steps ? A.g_out5_steps + (size_t)t * 5 * n + ge : nullptr;
                const float w1 = g5 ? g5[n] : w5_1, w2 = g5 ? g5[2 * n] : w5_2, w3 = g5 ? g5[3 * n] : w5_3;
                S.w[tid] = make_float2(w1, w2 + w3);                            // DAM:299-300 and veh2veh4real itself
            }
            S.mask[tid] = 0ull;
            if (tid == 0) S.count = 0;
        }
        __syncthreads();

        // ---- (B) near records into the queue; then the prediction ----
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * TV_THREADS >= items) break;                                 // block-uniform
            const int env = where[k] & 255, slot = where[k] >> 8;
            const float4 eg = S.ego[env];
            const bool near = grad::record_near(eg.x, eg.y, rec[k].x, rec[k].y);
            const unsigned long long b = __ballot(near);
            if (b != 0ull) {                             // wave-uniform; every lane of the wave is here
                int base = 0;
                if (lane == 0) base = atomicAdd(&S.count, __popcll(b));         // an LDS add: one per wave and pass
                base = __builtin_amdgcn_readfirstlane(base);
                if (near) {
                    const int pos = base + __popcll(b & ((1ull << lane) - 1ull));   // < nE * n_veh: one entry per record at most
                    const int item = k * TV_THREADS + tid;
                    queue[pos] = make_float4(rec[k].x, rec[k].y, rec[k].w, __int_as_float(item));
                    qpos[item] = (unsigned short)pos;
                    atomicOr(&S.mask[env], 1ull << slot);                       // LDS
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * TV_THREADS + tid < items) {
                float sn_, cs_;
                rec[k] = predict_record_tc<float>(rec[k], turn_consts(S.turn[where[k] >> 8]), SK, sn_, cs_);
            }
            __builtin_amdgcn_sched_barrier(0);           // one record at a time: interleaved, their temporaries would all be live
        }
        __syncthreads();

        // ---- (C) waves 1..3: the queue, one entry per thread | the env lanes: the env's forward chain ----
        float rew = 0.0f, road_t = 0.0f, road_r = 0.0f;
        if (tid >= 64) {
            const int cnt = S.count;
            for (int q = tid - 64; q < cnt; q += TV_THREADS - 64) {
                const float4 e = queue[q];
                const int item = __float_as_int(e.w);
                const int env = item / NV;
                const float4 eg = S.ego[env];
                float vs, vc;
                sincos_det(deg2rad(e.z), vs, vc);                               // DAM:221
                float t35[4], t25[4];
                const float4 pts = make_float4(eg.x + LWS * eg.w, eg.y + LWS * eg.z, eg.x - LWS * eg.w, eg.y - LWS * eg.z);
                veh2veh_terms(pts, e.x, e.y, vs, vc, t35, t25);                 // DAM:218-229
                const float p35 = ((t35[0] + t35[1]) + t35[2]) + t35[3];
                const float p25 = ((t25[0] + t25[1]) + t25[2]) + t25[3];
                float px = 0.0f, py = 0.0f, pphi = 0.0f;
                if (GRAD) {
                    const float2 w = S.w[env];
                    grad::record_partials(eg.x, eg.y, eg.z, eg.w, e.x, e.y, vs, vc, w.x, w.y, px, py, pphi);
                }
                queue[q] = make_float4(px, py, pphi, p35);
                q25[q] = p25;
            }
        } else if (env_lane) {
            float steer, a_x;
            action_transform(araw.x, araw.y, steer, a_x);                       // DAM:120
            const float punish_steer = -sq(steer), punish_a_x = -sq(a_x);       // DAM:198-199
            const float punish_yaw_rate = -sq(st[2]);                           // DAM:202
            const float devi_y = -sq(trk[0]);                                   // DAM:205
            const float devi_phi = -sq(deg2rad(trk[1]));                        // DAM:206
            const float devi_v = -sq(trk[2]);                                   // DAM:207
            rew = 0.05f * devi_v + 0.8f * devi_y + 30.0f * devi_phi + 0.02f * punish_yaw_rate + 5.0f * punish_steer +
                  0.05f * punish_a_x;                                           // DAM:297-298
            float nx[6];
            f_xu_core(st, steer, a_x, TAU10, phi_rad, es, ec, nx);              // DAM:387
            nx[0] = __builtin_fminf(__builtin_fmaxf(nx[0], 0.0f), 35.0f);       // DAM:390
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
            bi = 0;
            if (p >= 0) {                                                       // DAM:334-353
                float rx = 0.0f, ry = 0.0f, rphi = 0.0f;
                bi = tape_closest(A, p, roff, nx[3], nx[4], rx, ry, rphi);
                t0 = two2one<TASK>(nx[3], nx[4], rx, ry);                       // DAM:758
                t1 = deal_with_phi_diff(nx[5] - rphi);                          // DAM:759
                t2 = nx[0] - EXP_V;                                             // DAM:760
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) hv[c] = nx[c];
            hv[6] = t0; hv[7] = t1; hv[8] = t2;
            road_terms<TASK>(st[3] + LWS * ec, st[4] + LWS * es, road_t, road_r);   // DAM:231-295
            road_terms<TASK>(st[3] - LWS * ec, st[4] - LWS * es, road_t, road_r);
        }
        __syncthreads();

        // ---- (D) env lanes: sums in slot order, the step's outputs, the tape ----
        if (env_lane) {
            float a35 = 0.0f, a25 = 0.0f, px = 0.0f, py = 0.0f, pphi = 0.0f;
            for (unsigned long long m = S.mask[tid]; m; m &= m - 1ull) {        // slot order: the same sum wherever the row sits
                const int q = qpos[tid * NV + (__ffsll((long long)m) - 1)];
                const float4 r = queue[q];
                a35 += r.w; a25 += q25[q];                                      // DAM:218-229: far records add exact zeros
                px += r.x; py += r.y; pphi += r.z;
            }
            if (act && A.out5_steps) {
                float* out5 = A.out5_steps + (size_t)t * 5 * n + ge;
                out5[0] = rew;
                out5[n] = a35 + road_t;                  // DAM:299
                out5[2 * n] = a25 + road_r;              // DAM:300
                out5[3 * n] = a25;
                out5[4 * n] = road_r;
            }
            if (GRAD) {
                float* T = tapeL + (size_t)t * E + tid;
                const size_t cs = (size_t)H * E;
#pragma unroll
                for (int c = 0; c < 6; ++c) T[c * cs] = st[c];
#pragma unroll
                for (int c = 0; c < 3; ++c) T[(6 + c) * cs] = trk[c];
                T[9 * cs] = px; T[10 * cs] = py; T[11 * cs] = pphi;
            }
#pragma unroll
            for (int c = 0; c < 6; ++c) st[c] = hv[c];
            trk[0] = hv[6]; trk[1] = hv[7]; trk[2] = hv[8];
            araw = araw_next;
        }
        // (the next step's (A) writes ego / w / mask / count, which (D) of this step is through with in program order on the env
        //  lanes; the other waves are past their last read of them since the barrier above)
    }

    // ---- the obs after the last step ----
    if (A.obs_out) {
#pragma unroll
        for (int k = 0; k < RPT; ++k)
            if (k * TV_THREADS + tid < items)
                *reinterpret_cast<f4u*>(A.obs_out + (size_t)(e0 + (where[k] & 255)) * D + nd + 4 * (where[k] >> 8)) = rec[k];
        if (act) {                                       // eb_rollout.hip:store_head_row, restated (DAM:717-724, 763-768)
            float* row = A.obs_out + (size_t)ge * D;
            *reinterpret_cast<f4u*>(row) = f4u{hv[0], hv[1], hv[2], hv[3]};
            *reinterpret_cast<f4u*>(row + 4) = f4u{hv[4], hv[5], hv[6], hv[7]};
            row[8] = hv[8];
            float* otrk = row + 9;
            if (p >= 0) {
                const PathTables& pt = *A.dt;
                const int len = pt.len[p];
                int cur = bi * 10;                                              // DAM:714
                for (int k = 0; k < A.n_future; ++k) {
                    cur += 80;
                    if (cur >= len - 2) cur = len - 2;
                    const int fi = clamp_index(cur, len);
                    otrk[3 * k] = pt.x[p][fi] - hv[3];
                    otrk[3 * k + 1] = pt.y[p][fi] - hv[4];
                    otrk[3 * k + 2] = deal_with_phi_diff(hv[5] - pt.phi[p][fi]);
                }
            } else {
                for (int c = 0; c < 3 * A.n_future; ++c) otrk[c] = 0.0f;       // DAM:342, 352
            }
        }
    }
    if (!GRAD || !act) return;

    // ---- the reverse sweep: env lanes alone, out of LDS (each lane reads what it wrote itself) ----
    float g_final[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float ffx = 0.0f, ffy = 0.0f, ffphi = 0.0f;
    if (A.g_obs_final) {
        const float* g = A.g_obs_final + (size_t)ge * A.ld_final;
#pragma unroll
        for (int c = 0; c < 9; ++c) g_final[c] = g[c];
        for (int k = 0; k < A.n_future; ++k) {                                  // DAM:763-768
            ffx += g[9 + 3 * k]; ffy += g[10 + 3 * k]; ffphi += g[11 + 3 * k];
        }
    }
    const size_t cs = (size_t)H * E;
    const float* const tape = A.tape;
    const float* const g5s = A.g_out5_steps;
    float* const g_tape = A.g_action_tape;
    const float* const mine = tapeL + tid;
    auto load = [=](int t, grad::TapeStep& T) {
        const float* L = mine + (size_t)t * E;
#pragma unroll
        for (int c = 0; c < 6; ++c) T.st[c] = L[c * cs];
#pragma unroll
        for (int c = 0; c < 3; ++c) T.trk[c] = L[(6 + c) * cs];
        T.px = L[9 * cs]; T.py = L[10 * cs]; T.pphi = L[11 * cs];
        const f2u a = *reinterpret_cast<const f2u*>(tape + 2 * ((size_t)t * n + ge));
        T.a0 = a.x; T.a1 = a.y;
        const float* g5 = g5s ? g5s + (size_t)t * 5 * n + ge : nullptr;
        T.w[0] = g5 ? g5[0] : w5_0; T.w[1] = g5 ? g5[n] : w5_1; T.w[2] = g5 ? g5[2 * n] : w5_2;
        T.w[3] = g5 ? g5[3 * n] : w5_3; T.w[4] = g5 ? g5[4 * n] : w5_4;
    };
    auto store = [=](int t, const float (&ga)[2]) {
        if (g_tape) *reinterpret_cast<f2u*>(g_tape + 2 * ((size_t)t * n + ge)) = f2u{ga[0], ga[1]};
    };
    float go[9];
    grad::tape_reverse<TASK>(H, p >= 0, g_final, ffx, ffy, ffphi, load, store, go);
    if (A.g_obs0) {
        float* gi = A.g_obs0 + (size_t)ge * nd;
        *reinterpret_cast<f4u*>(gi) = f4u{go[0], go[1], go[2], go[3]};
        *reinterpret_cast<f4u*>(gi + 4) = f4u{go[4], go[5], go[6], go[7]};
        gi[8] = go[8];
        for (int c = 9; c < nd; ++c) gi[c] = 0.0f;       // the pre-step look-ahead columns feed nothing (DAM:189-207, 322-333)
    }
}

// the tile: the most envs per block (32, 16, 8) whose LDS fits the budget and whose grid still gives every CU two blocks
int tv_pick_tile(int n_env, int n_veh, int horizon, bool grad, int n_cu) {
    int fit = 0;
    for (int E = 32; E >= 8; E >>= 1) {
        if (E * n_veh > TV_THREADS * TV_RPT_MAX || tv_lds_bytes(E, n_veh, horizon, grad) > TV_LDS_BUDGET) continue;
        if (!fit) fit = E;
        if ((n_env + E - 1) / E >= 2 * n_cu) return E;
    }
    return fit ? 8 : 0;
}

}  // namespace

int rollout_tape_vjp_max_horizon(int n_veh) {
    const size_t per_step = (size_t)TV_TAPE_FLOATS * 8 * sizeof(float);
    const size_t h = (TV_LDS_BUDGET - tv_queue_bytes(8, n_veh)) / per_step;
    return (int)(h < (size_t)TV_MAX_HORIZON ? h : (size_t)TV_MAX_HORIZON);
}

hipError_t launch_rollout_tape_vjp(int task, const TapeVjpArgs& A_in, int n_cu, hipStream_t s) {
    if (A_in.n_env <= 0) return hipSuccess;
    TapeVjpArgs A = A_in;
    const bool grad = A.g_obs0 != nullptr || A.g_action_tape != nullptr;
    A.envs_per_tile = tv_pick_tile(A.n_env, A.n_veh, A.horizon, grad, n_cu);
    if (A.envs_per_tile == 0) return hipErrorInvalidValue;      // beyond rollout_tape_vjp_max_horizon: refused by the caller before
    const int grid = (A.n_env + A.envs_per_tile - 1) / A.envs_per_tile;
    const size_t lds = tv_lds_bytes(A.envs_per_tile, A.n_veh, A.horizon, grad);
    const bool small = A.envs_per_tile * A.n_veh <= 2 * TV_THREADS;
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        return with_bool(grad, [&](auto g) {
            return with_bool(small, [&](auto sm) {
                constexpr int RPT = decltype(sm)::value ? 2 : TV_RPT_MAX;
                return launch_lds<rollout_tape_vjp_kernel<decltype(t)::value, RPT, decltype(g)::value>>(
                    dim3(grid), dim3(TV_THREADS), lds, dev, s, A);
            });
        });
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
