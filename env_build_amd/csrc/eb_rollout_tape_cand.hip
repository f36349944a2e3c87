// eb_rollout_tape_cand.hip — value-only open-loop rollout of K candidate action tapes per env (eb_rollout_tape_cand) in ONE launch,
// gfx950.
//
// A planner asks "what do these K tapes cost from this one state?": three candidate paths per ego (hier_decision.py:113-121), the
// step lengths of a line search, the starts of a multi-start solver.  Two facts make that cheaper than K rollouts:
//   - the vehicles do not depend on the ego (stop_gradient, DAM:195, 331, 402): a scene's records (predict_for_a_mode, DAM:405-427)
//     advance the same way under every candidate and are advanced ONCE per env and step, whatever K is;
//   - the env's own chain per step runs on one lane per env in eb_rollout_tape_vjp.hip, at most half a wave; here it runs on one lane
//     per (env, candidate), so the wave that carries it is full at the same instruction time.
// A block of 256 threads owns E consecutive envs (E = 32, 16 or 8; E * K <= 64) for the whole horizon:
//
//   records    every lane keeps up to RPT 16-byte (env, vehicle) records in registers and advances them once per step;
//   env role   lane c < E * K of wave 0 is (env = c mod E, candidate = c / E): its own copy of the row's first nine columns;
//   per step t   (A) the env role publishes its pose (x, y, sin, cos) to LDS;
//              (B) every lane tests its records against the K poses of the record's env: a record whose centre is within 6.31 m
//                  (DAM:228) goes into the block's queue as an (env, candidate, slot) entry (ballot + one LDS add per wave and
//                  candidate), its position into a per-(env, candidate, slot) table, its bit into the (env, candidate) slot mask;
//                  then the lane predicts its records;
//              (C) waves 1..3 take the queue, one entry per thread: the penalty terms (DAM:218-229); meanwhile the env role runs
//                  the env's own chain (action transform, rewards, bicycle step, closest point, tracking, walls);
//              (D) the env role sums the penalties in SLOT order (the mask's bits, lowest first), writes the step's out5 and adds
//                  the step's weighted sum to its cost.
//
// Arithmetic and order are those of the value-only eb_rollout_tape_vjp kernel, whose forward pieces are restated here as that file
// restates eb_rollout.hip's (the closest-point lookup is the family's one copy, tape_closest in eb_tape_device.h);
// tests/test_gpu_tape_cand.py holds out5_steps[k] to eb_rollout_tape bit for bit.  The queue's order
// varies from run to run; the sums do not.  A (row, candidate)'s bits depend on nothing but the row and that candidate's tape and
// path.  No atomics to global memory, no scratch; fp32 state only.
#include <hip/hip_runtime.h>

#include "eb_cand.h"
#include "eb_tape_device.h"
#include "eb_tape_grad_device.h"

namespace eb {
namespace {

constexpr int TC_THREADS = 256;
constexpr int TC_ENV_LANES = 64;                        // the env role is wave 0
constexpr size_t TC_LDS_BUDGET = 64 * 1024;             // dynamic LDS per block: two blocks per CU at least
constexpr int TC_RPT_MAX = 4;                           // records a lane keeps in registers: a tile holds at most 1024

struct TcSmem {
    float4 ego[TC_ENV_LANES];             // x, y, sin phi, cos phi of the pre-step pose of (env, candidate)
    unsigned long long mask[TC_ENV_LANES];   // per (env, candidate): slots with a near record
    unsigned char turn[64];               // TURN_* per slot
    int count;                            // entries in the near-record queue
};
// dynamic LDS: [queue: E * K * n_veh float4] [2.5 m sums: E * K * n_veh floats] [queue position of every (env, candidate, slot): 16 bits]
inline size_t tc_lds_bytes(int E, int K, int n_veh) {
    return (size_t)E * K * n_veh * (sizeof(float4) + sizeof(float) + sizeof(unsigned short));
}

template <int TASK, int RPT>
__global__ __launch_bounds__(TC_THREADS, 3) void rollout_tape_cand_kernel(const TapeCandArgs A) {
    __shared__ TcSmem S;
    extern __shared__ __align__(16) unsigned char tc_dyn[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int E = A.envs_per_tile, K = A.n_cand, NV = A.n_veh, D = A.obs_dim, nd = A.nd, H = A.horizon;
    const int e0 = blockIdx.x * E, nE = min(E, A.n_env - e0), items = nE * NV;
    const size_t n = (size_t)A.n_env;
    // (read once, up front: a select between a global load and a member of the argument block would put the block in scratch)
    const float w5_0 = A.w5[0], w5_1 = A.w5[1], w5_2 = A.w5[2], w5_3 = A.w5[3], w5_4 = A.w5[4];
    float4* const queue = reinterpret_cast<float4*>(tc_dyn);
    float* const q25 = reinterpret_cast<float*>(tc_dyn + (size_t)E * K * NV * sizeof(float4));
    unsigned short* const qpos = reinterpret_cast<unsigned short*>(tc_dyn + (size_t)E * K * NV * (sizeof(float4) + sizeof(float)));

    // ---- the block's records: item = k * 256 + tid -> (env, slot); requested before anything else ----
    f4u rec[RPT];
    int where[RPT];                                      // env | slot << 8 of record k
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int item = k * TC_THREADS + tid;
        const bool valid = item < items;
        const int env = valid ? item / NV : 0, slot = valid ? item - env * NV : 0;
        where[k] = env | slot << 8;
        rec[k] = *reinterpret_cast<const f4u*>(A.obs0 + (size_t)(e0 + env) * D + nd + 4 * slot);
        if (!valid) rec[k].x = 1e30f;                    // never near an ego, never predicted
    }
    if (tid < 64) S.turn[tid] = A.dt->turn[tid];
    const SinCosK SK = sincos_consts();

    // ---- the env role's state: lane c = candidate * E + env ----
    const bool env_lane = tid < E * K;                   // E * K <= 64: wave 0
    const int my_env = tid & (E - 1), my_cand = env_lane ? tid / E : 0;        // E is a power of two
    const bool act = env_lane && my_env < nE;
    const int ge = e0 + (act ? my_env : 0);              // idle lanes shadow the tile's first env (in bounds), store nothing
    float st[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, trk[3] = {0.0f, 0.0f, 0.0f};
    int p = -1, roff = 0;
    f2u araw = f2u{0.0f, 0.0f};
    const float* my_tape = A.tapes + 2 * ((size_t)my_cand * H * n + ge);
    if (env_lane) {
        const float* o = A.obs0 + (size_t)ge * D;
        const f4u h0 = *reinterpret_cast<const f4u*>(o), h1 = *reinterpret_cast<const f4u*>(o + 4);
        st[0] = h0.x; st[1] = h0.y; st[2] = h0.z; st[3] = h0.w; st[4] = h1.x; st[5] = h1.y;
        trk[0] = h1.z; trk[1] = h1.w; trk[2] = o[8];
        p = (int)((A.path_bits >> (2 * my_cand)) & 3u);
        if (A.training) {
            const int pr = A.ref_idx[(size_t)my_cand * A.ref_ld + ge];
            p = (pr >= 0 && pr < A.n_paths) ? pr : -1;                          // DAM:342, 352
        }
        roff = p == 1 ? A.red_off[1] : p == 2 ? A.red_off[2] : A.red_off[0];
        araw = *reinterpret_cast<const f2u*>(my_tape);
        if (A.retrack) {                                 // the row's own pose on this candidate's path (DAM:735-760; the reference
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;       // builds one obs per path, hier_decision.py:113-117)
            if (p >= 0) {
                float rx = 0.0f, ry = 0.0f, rphi = 0.0f;
                tape_closest(A, p, roff, st[3], st[4], rx, ry, rphi);
                t0 = two2one<TASK>(st[3], st[4], rx, ry);                       // DAM:758
                t1 = deal_with_phi_diff(st[5] - rphi);                          // DAM:759
                t2 = st[0] - EXP_V;                                             // DAM:760
            }
            trk[0] = t0; trk[1] = t1; trk[2] = t2;
        }
    }
    float hv[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float J = 0.0f;

    for (int t = 0; t < H; ++t) {
        // ---- (A) env role: the pose ----
        float es = 0.0f, ec = 0.0f, phi_rad = 0.0f;
        f2u araw_next = araw;
        if (env_lane) {
            if (t + 1 < H) araw_next = *reinterpret_cast<const f2u*>(my_tape + 2 * (size_t)(t + 1) * n);   // prefetch
            phi_rad = deg2rad(st[5]);
            sincos_det(phi_rad, es, ec);                                        // DAM:211 and DAM:79-80
            S.ego[tid] = make_float4(st[3], st[4], es, ec);
            S.mask[tid] = 0ull;
            if (tid == 0) S.count = 0;
        }
        __syncthreads();

        // ---- (B) near records into the queue, candidate by candidate; then the prediction ----
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * TC_THREADS >= items) break;                                 // block-uniform
            const int env = where[k] & 255, slot = where[k] >> 8;
            for (int c = 0; c < K; ++c) {
                const int cell = c * E + env;                                   // < E * K
                const float2 eg = *reinterpret_cast<const float2*>(&S.ego[cell]);
                const bool near = grad::record_near(eg.x, eg.y, rec[k].x, rec[k].y);
                const unsigned long long b = __ballot(near);
                if (b != 0ull) {                         // wave-uniform; every lane of the wave is here
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&S.count, __popcll(b));     // an LDS add: one per wave, pass and candidate
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (near) {
                        const int pos = base + __popcll(b & ((1ull << lane) - 1ull));   // < nE * K * n_veh: one entry per (record, candidate) at most
                        const int idx = cell * NV + slot;
                        queue[pos] = make_float4(rec[k].x, rec[k].y, rec[k].w, __int_as_float(idx));
                        qpos[idx] = (unsigned short)pos;
                        atomicOr(&S.mask[cell], 1ull << slot);                  // LDS
                    }
                }
            }
        }
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            if (k * TC_THREADS + tid < items) {
                float sn_, cs_;
                rec[k] = predict_record_tc<float>(rec[k], turn_consts(S.turn[where[k] >> 8]), SK, sn_, cs_);
            }
            __builtin_amdgcn_sched_barrier(0);           // one record at a time: interleaved, their temporaries would all be live
        }
        __syncthreads();

        // ---- (C) waves 1..3: the queue, one entry per thread | the env role: the env's own chain ----
        float rew = 0.0f, road_t = 0.0f, road_r = 0.0f;
        if (tid >= TC_ENV_LANES) {
            const int cnt = S.count;
            for (int q = tid - TC_ENV_LANES; q < cnt; q += TC_THREADS - TC_ENV_LANES) {
                const float4 e = queue[q];
                const int cell = __float_as_int(e.w) / NV;
                const float4 eg = S.ego[cell];
                float vs, vc;
                sincos_det(deg2rad(e.z), vs, vc);                               // DAM:221
                float t35[4], t25[4];
                const float4 pts = make_float4(eg.x + LWS * eg.w, eg.y + LWS * eg.z, eg.x - LWS * eg.w, eg.y - LWS * eg.z);
                veh2veh_terms(pts, e.x, e.y, vs, vc, t35, t25);                 // DAM:218-229
                queue[q].w = ((t35[0] + t35[1]) + t35[2]) + t35[3];
                q25[q] = ((t25[0] + t25[1]) + t25[2]) + t25[3];
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
            if (p >= 0) {                                                       // DAM:334-353
                float rx = 0.0f, ry = 0.0f, rphi = 0.0f;
                tape_closest(A, p, roff, nx[3], nx[4], rx, ry, rphi);
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

        // ---- (D) env role: sums in slot order, the step's outputs, the cost ----
        if (env_lane) {
            float a35 = 0.0f, a25 = 0.0f;
            for (unsigned long long m = S.mask[tid]; m; m &= m - 1ull) {        // slot order: the same sum wherever the row sits
                const int q = qpos[tid * NV + (__ffsll((long long)m) - 1)];
                a35 += queue[q].w; a25 += q25[q];                               // DAM:218-229: far records add exact zeros
            }
            const float o1 = a35 + road_t, o2 = a25 + road_r;                   // DAM:299-300
            if (act && A.out5_steps) {
                float* out5 = A.out5_steps + ((size_t)my_cand * H + t) * 5 * n + ge;
                out5[0] = rew;
                out5[n] = o1;
                out5[2 * n] = o2;
                out5[3 * n] = a25;
                out5[4 * n] = road_r;
            }
            // s_t: the rows with a non-zero weight, in row order; J: ascending t from +0 (include/envbuild_cand.h)
            float s = 0.0f;
            bool any = false;
            if (w5_0 != 0.0f) { s = rew * w5_0; any = true; }
            if (w5_1 != 0.0f) { const float v = o1 * w5_1; s = any ? s + v : v; any = true; }
            if (w5_2 != 0.0f) { const float v = o2 * w5_2; s = any ? s + v : v; any = true; }
            if (w5_3 != 0.0f) { const float v = a25 * w5_3; s = any ? s + v : v; any = true; }
            if (w5_4 != 0.0f) { const float v = road_r * w5_4; s = any ? s + v : v; any = true; }
            if (any) J += s;
#pragma unroll
            for (int c = 0; c < 6; ++c) st[c] = hv[c];
            trk[0] = hv[6]; trk[1] = hv[7]; trk[2] = hv[8];
            araw = araw_next;
        }
        // (the next step's (A) writes ego / mask / count, which (D) of this step is through with in program order on the env
        //  role; the other waves are past their last read of them since the barrier above)
    }
    if (act && A.cost) A.cost[(size_t)my_cand * n + ge] = J;
}

// the tile: the most envs per block (32, 16, 8) whose (env, candidate) lanes fit one wave, whose LDS fits the budget and whose grid
// still gives every CU two blocks
int tc_pick_tile(int n_env, int n_cand, int n_veh, int n_cu) {
    int fit = 0;
    for (int E = 32; E >= 8; E >>= 1) {
        if (E * n_cand > TC_ENV_LANES || E * n_veh > TC_THREADS * TC_RPT_MAX || tc_lds_bytes(E, n_cand, n_veh) > TC_LDS_BUDGET) continue;
        if (!fit) fit = E;
        if ((n_env + E - 1) / E >= 2 * n_cu) return E;
    }
    return fit ? 8 : 0;
}

}  // namespace

int rollout_tape_cand_max(int n_veh) {
    const size_t k = TC_LDS_BUDGET / tc_lds_bytes(8, 1, n_veh < 1 ? 1 : n_veh);
    return (int)(k < (size_t)TC_MAX_CAND ? k : (size_t)TC_MAX_CAND);
}

hipError_t launch_rollout_tape_cand(int task, const TapeCandArgs& A_in, int n_cu, hipStream_t s) {
    if (A_in.n_env <= 0 || A_in.n_cand <= 0) return hipSuccess;
    TapeCandArgs A = A_in;
    A.envs_per_tile = tc_pick_tile(A.n_env, A.n_cand, A.n_veh, n_cu);
    if (A.envs_per_tile == 0) return hipErrorInvalidValue;      // beyond rollout_tape_cand_max: refused by the caller before
    const int grid = (A.n_env + A.envs_per_tile - 1) / A.envs_per_tile;
    const size_t lds = tc_lds_bytes(A.envs_per_tile, A.n_cand, A.n_veh);
    const bool small = A.envs_per_tile * A.n_veh <= 2 * TC_THREADS;
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        return with_bool(small, [&](auto sm) {
            constexpr int RPT = decltype(sm)::value ? 2 : TC_RPT_MAX;
            return launch_lds<rollout_tape_cand_kernel<decltype(t)::value, RPT>>(dim3(grid), dim3(TC_THREADS), lds, dev, s, A);
        });
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
