// eb_policy_rollout.hip — the closed-loop rollout (eb_policy_rollout, include/envbuild_policy_rollout.h): H steps of
// [policy(obs) -> rollout_out] for a batch in ONE launch, gfx950.
//
// The shield (hier_decision.py:89-107, multi_ego.py:187-209) and every look-ahead under a policy alternate two launches per step:
// the policy kernel reads the observations and writes the actions, the rollout step reads both and writes the next observations.
// With binary16 operands the policy is short enough that the ten launch boundaries of a 5-step look-ahead and the
// rows' round trips through memory are a third of the pass.  Here a block of 256 threads owns 64 consecutive envs — the policy
// kernel's tile — for the whole horizon, and the rows never leave the CU:
//
//   rows        the tile's fp32 rows [64][D] live in LDS from the first load to the last store;
//   per step t  (1) input: x0 = f16(row * scale) into the binary16 activation buffer (one fp32 multiply, then one conversion), and the
//                   env role (thread e < 64 = env e) publishes its pose (x, y, sin, cos);
//               (2) the policy: eb_policy_f16_device.h's hidden layers on v_mfma_f32_32x32x16_f16, the output layer on
//                   v_mfma_f32_16x16x32_f16 (restated from eb_policy_f16.hip), eb_policy_run_batch's head on eb_mlp_device.h's
//                   activations; the 64 actions go to LDS;
//               (3) every thread tests its share of the tile's records against the record's env: a near one (DAM:228) goes into the
//                   block's queue as an INDEX — the record itself stays where it is, in the rows;
//               (4) waves 1..3 take the queue, one entry per thread: the circle-pair terms (DAM:218-229); meanwhile the env role runs
//                   the env's own chain (action transform, rewards, bicycle step, closest point, tracking, walls);
//               (5) the env role sums the penalties in SLOT order, writes the step's out5, adds the shield's penalty and puts the
//                   new head into its row; every thread predicts its records in place (DAM:405-427);
//               (6) the rows go to obs_steps[t] when asked for.
//
// The activation buffer is dead during (3)-(5) and the near-record scratch during (1)-(2): one region of LDS holds both.  Two blocks
// fit a CU at 32 slots x 256 units (static + dynamic LDS 71 504 B): one block's matrix phase runs under the other's model step.
// Synchronisation is __syncthreads() only — no flags, no polling, nothing between blocks, no atomics to global memory.
//
// Arithmetic and order are those of eb_policy_run_batch's binary16 kernel and of eb_rollout_step: the model step restates
// eb_rollout_tape_cand.hip's env chain at K = 1 (as every tape file does; eb_tape_device.h says why it is not shared), the penalty
// sums keep eb_rollout.hip's rule (a record with a non-zero 3.5 m sum, in slot order).  tests/test_gpu_policy_rollout.py holds every
// output to the loop of single calls bit for bit.  The queue's order varies from run to run; the sums do not.
#include "eb_policy_rollout.h"

#include "eb_policy_f16_device.h"
#include "eb_tape_device.h"
#include "eb_tape_grad_device.h"

namespace eb {
namespace {

constexpr int PR_ROWS = MLP_ROWS;         // envs per block
constexpr int PR_THREADS = MLP_THREADS;   // 4 waves

struct PrSmem {
    float4 ego[PR_ROWS];                  // x, y, sin phi, cos phi of the pre-step pose
    unsigned long long mask[PR_ROWS];     // per env: slots whose record has a non-zero penalty sum
    float2 act[PR_ROWS];                  // the step's raw actions
    int path[PR_ROWS];                    // the env's path, -1: none (DAM:342, 352)
    float pacc[PR_ROWS];                  // the shield's running penalty.  (Both are the env role's own, kept here and not in registers:
                                          //  the <2, 2> matrix phase has none to spare for values that live across it)
    unsigned char turn[64];               // TURN_* per slot
    int count;                            // entries in the near-record queue
};

__host__ __device__ inline size_t pr_rows_bytes(int obs_dim) { return ((size_t)PR_ROWS * obs_dim * sizeof(float) + 15) & ~(size_t)15; }
// the model step's scratch per (env, slot): 3.5 m sum, 2.5 m sum, one queue entry (an index)
__host__ __device__ inline size_t pr_scratch_bytes(int n_veh) { return (size_t)PR_ROWS * n_veh * (2 * sizeof(float) + sizeof(unsigned short)); }

template <int TASK, int RT, int CT>
__global__ __launch_bounds__(PR_THREADS, 2) void policy_rollout_kernel(const PolicyRolloutArgs A) {
    __shared__ PrSmem S;
    extern __shared__ __attribute__((aligned(16))) unsigned char pr_dyn[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int D = A.obs_dim, NV = A.n_veh, nd = A.nd, H = A.horizon, RS = A.row_stride;
    const int e0 = blockIdx.x * PR_ROWS, nE = min(PR_ROWS, A.n_env - e0), items = nE * NV;
    const size_t n = (size_t)A.n_env;
    float* const rows = reinterpret_cast<float*>(pr_dyn);
    unsigned char* const region = pr_dyn + pr_rows_bytes(D);
    _Float16* const lds = reinterpret_cast<_Float16*>(region);                 // steps (1)-(2)
    float* const pen35 = reinterpret_cast<float*>(region);                     // steps (3)-(5)
    float* const pen25 = pen35 + PR_ROWS * NV;
    unsigned short* const queue = reinterpret_cast<unsigned short*>(pen25 + PR_ROWS * NV);

    // ---- the tile's rows: consecutive in memory, so one coalesced sweep; rows beyond the batch are zeros and are never stored ----
    {
        const float* src = A.obs0 + (size_t)e0 * D;
        const int live = nE * D;
        for (int idx = tid; idx < PR_ROWS * D; idx += PR_THREADS) rows[idx] = idx < live ? src[idx] : 0.0f;
    }
    if (tid < 64) S.turn[tid] = A.dt->turn[tid];

    // ---- the env role: thread e of wave 0 is env e ----
    if (tid < PR_ROWS) {
        int p = -1;
        if (tid < nE) {
            p = A.path_id;
            if (A.training) {
                const int pr = A.ref_idx[e0 + tid];
                p = (pr >= 0 && pr < A.n_paths) ? pr : -1;                      // DAM:342, 352
            }
        }
        S.path[tid] = p;
        S.pacc[tid] = 0.0f;                                                     // hier_decision.py:93-97
    }
    __syncthreads();

    for (int t = 0; t < H; ++t) {
        // ---- (1) input: a wave takes 16 rows, lanes stride over a row; zero beyond obs_dim.  The env role: the pose ----
        {
            constexpr int RPW = PR_ROWS / 4;
            int st_ = tid;                                                      // (opaque, as `mt` below)
            asm volatile("" : "+v"(st_));
            const int rbase = (st_ >> 6) * RPW, K0 = A.hid[0].k_pad;
            for (int k = st_ & 63; k < K0; k += 64) {
                const int kc = k < D ? k : D - 1;
                const float sc = A.scale ? A.scale[kc] : 1.0f;                  // x * 1.0f is x, bit for bit
                const float* srow = rows + rbase * D + kc;
                _Float16* dst = lds + rbase * RS + k;
#pragma unroll
                for (int rr = 0; rr < RPW; ++rr) {
                    float x = srow[rr * D] * sc;                                // one fp32 multiply (preprocessor.py:121), THEN one conversion:
                    asm("" : "+v"(x));                                          // not the fused v_fma_mixlo_f16 the compiler would make of the two
                    dst[rr * RS] = (_Float16)((rbase + rr < nE && k < D) ? x : 0.0f);
                }
            }
            if (st_ < PR_ROWS) {
                const float* o = rows + st_ * D;
                float es, ec;
                sincos_det(deg2rad(o[5]), es, ec);                              // DAM:211 and DAM:79-80
                S.ego[st_] = make_float4(o[3], o[4], es, ec);
                S.mask[st_] = 0ull;
                if (st_ == 0) S.count = 0;
            }
        }
        __syncthreads();

        // ---- (2) the policy: hidden layers (eb_policy_f16.hip:mlp_f16_kernel's loop) ----
        {
            const int rt0 = RT == 2 ? 0 : (wave & 1);
            const int ct0 = RT == 2 ? wave * CT : (wave >> 1);
            for (int L = 0; L < A.n_hidden; ++L) {
                const MlpF16Layer& ly = A.hid[L];
                mlp::f32x16 acc[RT][CT];
#pragma unroll
                for (int c = 0; c < CT; ++c) {
                    const mlp::f32x4* bsrc = reinterpret_cast<const mlp::f32x4*>(ly.b + (ct0 + c) * 32 + 4 * h);   // units 8 g + 4 h + e
#pragma unroll
                    for (int g = 0; g < 4; ++g) {
                        const mlp::f32x4 b = bsrc[2 * g];
#pragma unroll
                        for (int r = 0; r < RT; ++r)
#pragma unroll
                            for (int e = 0; e < 4; ++e) acc[r][c][4 * g + e] = b[e];
                    }
                }
                layer_chain_f16<RT, CT>(lds + (rt0 * 32 + i) * RS + 8 * h, 32 * RS, reinterpret_cast<const f16x8*>(ly.w), ly.k_pad >> 4, ct0,
                                        lane, acc);
                __syncthreads();                                              // every wave has read this layer's inputs
                switch (A.hidden_act) {
                    case MLP_ACT_RELU: store_hidden_f16<RT, CT, MLP_ACT_RELU>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
                    case MLP_ACT_ELU: store_hidden_f16<RT, CT, MLP_ACT_ELU>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
                    case MLP_ACT_TANH: store_hidden_f16<RT, CT, MLP_ACT_TANH>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
                    default: store_hidden_f16<RT, CT, MLP_ACT_LINEAR>(lds, RS, rt0, ct0, i, h, A.n_units, acc); break;
                }
                __syncthreads();
            }
        }
        // the output layer (eb_policy_f16.hip, restated for out_dim = 4: one 16 x 16 x 32 column tile, row tile = wave).  Lane l
        // supplies A[observation l & 15][k = 32 s + 8 (l >> 4) + j] and B[k][column l & 15], j = 0..7; it receives D[4 (l >> 4) + v][l & 15]
        {
            const int i16 = lane & 15, kq = lane >> 4;
            const int steps = A.outl.k_pad >> 5;
            const _Float16* a_ptr = lds + (wave * 16 + i16) * RS + 8 * kq;
            const f16x8* wsrc = reinterpret_cast<const f16x8*>(A.outl.w) + lane;
            const float b = A.outl.b[i16];
            mlp::f32x4 acc = {b, b, b, b};
            f16x8 bq = wsrc[0];
            for (int s = 0; s < steps; ++s) {
                const f16x8 bn = wsrc[(size_t)(s + 1 < steps ? s + 1 : s) * 64];                 // the next step's weights under this MFMA
                const f16x8 aq = *reinterpret_cast<const f16x8*>(a_ptr + 32 * s);
                acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(aq, bq, acc, 0, 0, 0);
                bq = bn;
            }
            if (i16 < 2) {                                                     // deterministic action: action_range * tanh(mean), utils/policy.py:89-92
#pragma unroll
                for (int v = 0; v < 4; ++v) {
                    const int row = wave * 16 + 4 * kq + v;
                    const float mean = mlp::activate_rt(A.out_act, acc[v]);
                    const float a = A.action_range > 0.0f ? A.action_range * mlp::tanh_det(mean) : mean;
                    reinterpret_cast<float*>(&S.act[row])[i16] = a;
                    if (row < nE && A.actions_steps) A.actions_steps[((size_t)t * n + e0 + row) * 2 + i16] = a;
                }
            }
        }
        __syncthreads();                                                      // the activations are dead, the actions in LDS

        // (the thread's index, opaque from here to the end of the step: what the model step derives from it is then computed here, per
        //  step, and not once in front of the loop — where it would be held in registers through the matrix phase, which has none)
        int mt = tid;
        asm volatile("" : "+v"(mt));

        // ---- (3) near records into the queue, by index ----
        for (int base = 0; base < items; base += PR_THREADS) {                 // block-uniform
            const int item = base + mt;
            const bool valid = item < items;
            const int env = valid ? (A.nv_magic ? (int)__umulhi((unsigned)item, A.nv_magic) : item) : 0;
            const int slot = valid ? item - env * NV : 0;
            const float* r = rows + env * D + nd + 4 * slot;
            const float2 eg = *reinterpret_cast<const float2*>(&S.ego[env]);
            const bool near = valid && grad::record_near(eg.x, eg.y, r[0], r[1]);
            const unsigned long long b = __ballot(near);
            if (b != 0ull) {                                                    // wave-uniform; every lane of the wave is here
                int qb = 0;
                if (lane == 0) qb = atomicAdd(&S.count, __popcll(b));           // an LDS add: one per wave and pass
                qb = __builtin_amdgcn_readfirstlane(qb);
                if (near) queue[qb + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)item;   // < items: an entry per record at most
            }
        }
        __syncthreads();

        // ---- (4) waves 1..3: the queue, one entry per thread | the env role: the env's own chain ----
        float rew = 0.0f, road_t = 0.0f, road_r = 0.0f;
        float hv[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        if (mt >= PR_ROWS) {
            const int cnt = S.count;
            for (int q = mt - PR_ROWS; q < cnt; q += PR_THREADS - PR_ROWS) {
                const int item = queue[q];
                const int env = A.nv_magic ? (int)__umulhi((unsigned)item, A.nv_magic) : item, slot = item - env * NV;
                const float* r = rows + env * D + nd + 4 * slot;
                const float4 eg = S.ego[env];
                float vs, vc;
                sincos_det(deg2rad(r[3]), vs, vc);                              // DAM:221
                float t35[4], t25[4];
                const float4 pts = make_float4(eg.x + LWS * eg.w, eg.y + LWS * eg.z, eg.x - LWS * eg.w, eg.y - LWS * eg.z);
                veh2veh_terms(pts, r[0], r[1], vs, vc, t35, t25);               // DAM:218-229
                const float p35 = ((t35[0] + t35[1]) + t35[2]) + t35[3];
                const float p25 = ((t25[0] + t25[1]) + t25[2]) + t25[3];
                if (p35 != 0.0f) {                                              // p25 != 0 implies p35 != 0
                    pen35[item] = p35;
                    pen25[item] = p25;
                    atomicOr(&S.mask[env], 1ull << slot);                       // LDS
                }
            }
        } else {
            const float* o = rows + mt * D;
            const float st[6] = {o[0], o[1], o[2], o[3], o[4], o[5]};
            const float trk0 = o[6], trk1 = o[7], trk2 = o[8];
            const float2 araw = S.act[mt];
            const float4 eg = S.ego[mt];
            const float es = eg.z, ec = eg.w, phi_rad = deg2rad(st[5]);
            float steer, a_x;
            action_transform(araw.x, araw.y, steer, a_x);                       // DAM:120
            const float punish_steer = -sq(steer), punish_a_x = -sq(a_x);       // DAM:198-199
            const float punish_yaw_rate = -sq(st[2]);                           // DAM:202
            const float devi_y = -sq(trk0);                                     // DAM:205
            const float devi_phi = -sq(deg2rad(trk1));                          // DAM:206
            const float devi_v = -sq(trk2);                                     // DAM:207
            rew = 0.05f * devi_v + 0.8f * devi_y + 30.0f * devi_phi + 0.02f * punish_yaw_rate + 5.0f * punish_steer +
                  0.05f * punish_a_x;                                           // DAM:297-298
            float nx[6];
            f_xu_core(st, steer, a_x, TAU10, phi_rad, es, ec, nx);              // DAM:387
            nx[0] = __builtin_fminf(__builtin_fmaxf(nx[0], 0.0f), 35.0f);       // DAM:390
            float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f;
            const int p = S.path[mt];
            if (p >= 0) {                                                       // DAM:334-353
                const int roff = p == 1 ? A.red_off[1] : p == 2 ? A.red_off[2] : A.red_off[0];
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

        // ---- (5) env role: sums in slot order, the step's outputs, the new head | every thread: its records, in place ----
        if (mt < PR_ROWS) {
            float a35 = 0.0f, a25 = 0.0f;
            for (unsigned long long m = S.mask[mt]; m; m &= m - 1ull) {        // slot order: the same sum wherever the row sits
                const int it = mt * NV + (__ffsll((long long)m) - 1);
                a35 += pen35[it]; a25 += pen25[it];                             // DAM:218-229: every other record adds exact zeros
            }
            const float o1 = a35 + road_t, o2 = a25 + road_r;                   // DAM:299-300
            if (mt < nE && A.out5_steps) {
                float* out5 = A.out5_steps + (size_t)t * 5 * n + e0 + mt;
                out5[0] = rew;
                out5[n] = o1;
                out5[2 * n] = o2;
                out5[3 * n] = a25;
                out5[4 * n] = road_r;
            }
            S.pacc[mt] = S.pacc[mt] + (A.penalty_row == 3 ? a25 : o2);        // punish += penalty, ascending t from +0
            float* o = rows + mt * D;
#pragma unroll
            for (int c = 0; c < 9; ++c) o[c] = hv[c];
        }
        const SinCosK SK = sincos_consts();
        for (int base = 0; base < items; base += PR_THREADS) {
            const int item = base + mt;
            if (item < items) {
                const int env = A.nv_magic ? (int)__umulhi((unsigned)item, A.nv_magic) : item, slot = item - env * NV;
                float* r = rows + env * D + nd + 4 * slot;
                float sn_, cs_;
                const f4u nv = predict_record_tc<float>(f4u{r[0], r[1], r[2], r[3]}, turn_consts(S.turn[slot]), SK, sn_, cs_);
                r[0] = nv.x; r[1] = nv.y; r[2] = nv.z; r[3] = nv.w;
            }
        }
        __syncthreads();

        // ---- (6) the state after step t ----
        if (A.obs_steps) {
            float* dst = A.obs_steps + ((size_t)t * n + e0) * D;
            const int live = nE * D;
            for (int idx = tid; idx < live; idx += PR_THREADS) dst[idx] = rows[idx];
        }
        // (the next step's (1) only reads the rows; its writes to the activation buffer, ego, mask and count come after the barrier
        //  above, which every reader of the scratch and of this step's poses has passed)
    }

    {
        float* dst = A.obs_out + (size_t)e0 * D;
        const int live = nE * D;
        for (int idx = tid; idx < live; idx += PR_THREADS) dst[idx] = rows[idx];
    }
    if (tid < nE) {                                                             // (nE <= 64: the env role)
        const float pacc = S.pacc[tid];
        if (A.punish) A.punish[e0 + tid] = pacc;
        if (A.safe) A.safe[e0 + tid] = pacc > 0.0f ? 0 : 1;                           // safe = !(punish > 0), hier_decision.py:97
    }
}

}  // namespace

size_t policy_rollout_lds_bytes(int obs_dim, int n_veh, int row_stride) {
    const size_t actb = (size_t)PR_ROWS * row_stride * sizeof(uint16_t), scr = pr_scratch_bytes(n_veh);
    return pr_rows_bytes(obs_dim) + (actb > scr ? actb : scr);
}

hipError_t launch_policy_rollout(int task, const PolicyRolloutArgs& A, hipStream_t s) {
    if (A.n_env <= 0) return hipSuccess;
    if (A.units != 64 && A.units != 128 && A.units != 256) return hipErrorInvalidValue;   // refused by the caller before
    const dim3 g((A.n_env + PR_ROWS - 1) / PR_ROWS), b(PR_THREADS);
    const size_t lds = policy_rollout_lds_bytes(A.obs_dim, A.n_veh, A.row_stride);
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        constexpr int T = decltype(t)::value;
        return A.units == 64 ? launch_lds<&policy_rollout_kernel<T, 1, 1>>(g, b, lds, dev, s, A)
               : A.units == 128 ? launch_lds<&policy_rollout_kernel<T, 2, 1>>(g, b, lds, dev, s, A)
                                : launch_lds<&policy_rollout_kernel<T, 2, 2>>(g, b, lds, dev, s, A);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
