// eb_policy_rollout_sample.hip — the closed-loop rollout under the fp32 policy's STOCHASTIC head (tanh-Gaussian actions, their
// log-probabilities) and, on request, its reverse sweep with the noise held fixed (eb_policy_rollout_sample,
// include/envbuild_policy_rollout_sample.h) in ONE launch, gfx950.
//
// policy_rollout_sample_kernel is policy_rollout_sample_kernel (eb_policy_rollout_sample.hip: read its header comment for the block's
// layout, the steps (1)-(6) of the forward and (R1)-(R3) of the reverse) with three differences:
//
//   the head    after the 16 x 16 x 4 output chain a row's mean0, mean1, ls0, ls1 sit in four lanes.  Once every wave has left the
//               chain (a __syncthreads) the activation buffer is dead: the 64 x 4 activated logits go there with eb_policy_sample.hip's
//               row stride of 33 floats, and after a second __syncthreads lanes 0..15 of each wave — the wave's own 16 rows, so the
//               four SIMDs share the logarithms and exponentials — run psample::sample_row with key_t = splitmix64(seed + GOLDEN *
//               (counter + t)), formed as eb_policy_sample's kernel forms it.  The lane puts the actions into LDS for the model step
//               and writes actions / logp / eps with plain vector stores;
//   the tape    PRS_TAPE_FLOATS = 20 per (step, env): the parent's 14, then the activated means, log-stds and the eps used;
//   (R2)        d_out has four live columns: psample::sample_vjp_elem from g_a_t and w_logp, each times the output activation's
//               derivative (eb_policy_sample_vjp followed by eb_mlp_backward's head 0); exact zeros beyond column 3 and the batch.
// With A.with_grad == 0 (a kernarg: block-uniform) the x_l / tape stores and the whole reverse are skipped and the workspace is never
// touched.  Synchronisation is __syncthreads() only; no atomics to global memory; nothing between blocks.  The parent's translation
// unit is untouched: this one is written against the shared device headers only.
#include "eb_policy_rollout_sample.h"

#include "eb_mlp_device.h"
#include "eb_policy_sample_device.h"
#include "eb_tape_device.h"
#include "eb_tape_grad_device.h"

namespace eb {
namespace {

constexpr int PS_ROWS = MLP_ROWS;         // envs per block
constexpr int PS_THREADS = MLP_THREADS;   // 4 waves

struct PsSmem {
    float4 ego[PS_ROWS];                  // x, y, sin phi, cos phi of the pre-step pose
    unsigned long long mask[PS_ROWS];     // per env: slots with a near record
    float2 act[PS_ROWS];                  // forward: the step's raw actions; reverse: their cotangent
    float lam[9][PS_ROWS];                // reverse: the cotangent of the state's columns 0..8
    float J[PS_ROWS];                     // the env's running cost
    int path[PS_ROWS];                    // the env's path, -1: none (DAM:342, 352)
    unsigned char turn[64];               // TURN_* per slot
    int count;                            // entries in the near-record queue
};

__host__ __device__ inline size_t ps_rows_bytes(int obs_dim) { return ((size_t)PS_ROWS * obs_dim * sizeof(float) + 15) & ~(size_t)15; }
// the model step's scratch per (env, slot): 3.5 m sum, 2.5 m sum, three partials, one queue entry (an index)
__host__ __device__ inline size_t ps_scratch_bytes(int n_veh) { return (size_t)PS_ROWS * n_veh * (5 * sizeof(float) + sizeof(unsigned short)); }

template <int TASK, int RT, int CT>
__global__ __launch_bounds__(PS_THREADS, 1) void policy_rollout_sample_kernel(const PolicyRolloutSampleArgs A) {
    __shared__ PsSmem S;
    extern __shared__ __attribute__((aligned(16))) unsigned char ps_dyn[];
    const int tid = threadIdx.x, wave = __builtin_amdgcn_readfirstlane(tid >> 6), lane = tid & 63;
    const int i = lane & 31, h = lane >> 5;
    const int D = A.obs_dim, NV = A.n_veh, nd = A.nd, H = A.horizon, NH = A.n_hidden, U = A.units;
    const int RS = A.row_stride, HS = (RS - 4) >> 1, K0 = A.hid[0].k_pad;
    const int e0 = blockIdx.x * PS_ROWS, nE = min(PS_ROWS, A.n_env - e0), items = nE * NV;
    const size_t n = (size_t)A.n_env, np = (size_t)A.n_pad;
    float* const rows = reinterpret_cast<float*>(ps_dyn);
    unsigned char* const region = ps_dyn + ps_rows_bytes(D);
    float* const lds = reinterpret_cast<float*>(region);                       // the policy, both ways
    float* const pen35 = reinterpret_cast<float*>(region);                     // steps (3)-(5)
    float* const pen25 = pen35 + PS_ROWS * NV;
    float* const ppx = pen25 + PS_ROWS * NV;
    float* const ppy = ppx + PS_ROWS * NV;
    float* const ppphi = ppy + PS_ROWS * NV;
    unsigned short* const queue = reinterpret_cast<unsigned short*>(ppphi + PS_ROWS * NV);
    float* const tape = A.ws + A.tape_off + e0;                                // record c of step t, env e: [(t * PRS_TAPE_FLOATS + c) * n_pad + e]
    float w5_0 = A.w5[0], w5_1 = A.w5[1], w5_2 = A.w5[2], w5_3 = A.w5[3], w5_4 = A.w5[4];
    asm volatile("" : "+v"(w5_0), "+v"(w5_1), "+v"(w5_2), "+v"(w5_3), "+v"(w5_4));   // vector registers, for the reason given below
    const float w35 = w5_1, w25 = w5_2 + w5_3;                                 // DAM:299-300 and veh2veh4real itself
    const bool WG = A.with_grad != 0;                                          // block-uniform: a kernarg
    // the head's arguments, moved to vector registers once: only 16 lanes per wave and step use them, and as scalars they would be
    // spilled across the whole step (the block has 512 VGPRs and few SGPRs to spare)
    unsigned long long hv_row_ids = (unsigned long long)A.row_ids, hv_eps = (unsigned long long)A.eps_steps;
    unsigned long long hv_logp = (unsigned long long)A.logp_steps, hv_eps_out = (unsigned long long)A.eps_out_steps;
    unsigned long long hv_seed = A.seed, hv_counter = A.counter;
    float hv_log_ar = A.log_ar;
    asm volatile("" : "+v"(hv_row_ids), "+v"(hv_eps), "+v"(hv_logp), "+v"(hv_eps_out), "+v"(hv_seed), "+v"(hv_counter), "+v"(hv_log_ar));

    // ---- the tile's rows: consecutive in memory, so one coalesced sweep; rows beyond the batch are zeros and are never stored ----
    {
        const float* src = A.obs0 + (size_t)e0 * D;
        const int live = nE * D;
        for (int idx = tid; idx < PS_ROWS * D; idx += PS_THREADS) rows[idx] = idx < live ? src[idx] : 0.0f;
    }
    if (tid < 64) S.turn[tid] = A.dt->turn[tid];

    // ---- the env role: thread e of wave 0 is env e ----
    if (tid < PS_ROWS) {
        int p = -1;
        if (tid < nE) {
            p = A.path_id;
            if (A.training) {
                const int pr = A.ref_idx[e0 + tid];
                p = (pr >= 0 && pr < A.n_paths) ? pr : -1;                      // DAM:342, 352
            }
        }
        S.path[tid] = p;
        S.J[tid] = 0.0f;
#pragma unroll
        for (int c = 0; c < 9; ++c) S.lam[c][tid] = 0.0f;                       // no cotangent of the final state in this entry
    }
    __syncthreads();

    const int rt0 = RT == 2 ? 0 : (wave & 1);
    const int ct0 = RT == 2 ? wave * CT : (wave >> 1);
    const float* const a_row = lds + (rt0 * 32 + i) * RS + h * HS;

    // =================================================== forward ===================================================
    for (int t = 0; t < H; ++t) {
        const size_t trow = (size_t)t * np + e0;                                // the tile's first row of step t in the workspace
        // ---- (1) input: a wave takes 16 rows, lanes stride over a row; zero beyond obs_dim and beyond the batch.  The env role: the pose ----
        {
            constexpr int RPW = PS_ROWS / 4;
            const int rbase = wave * RPW;
            float* x0g = A.ws + A.x_off[0] + (trow + rbase) * K0;
            for (int k = lane; k < K0; k += 64) {
                const int kc = k < D ? k : D - 1;
                const float sc = A.scale ? A.scale[kc] : 1.0f;                  // x * 1.0f is x, bit for bit
                const float* srow = rows + rbase * D + kc;
                float* dst = lds + rbase * RS + (k & 1) * HS + (k >> 1);
#pragma unroll
                for (int rr = 0; rr < RPW; ++rr) {
                    const float x = (rbase + rr < nE && k < D) ? srow[rr * D] * sc : 0.0f;
                    dst[rr * RS] = x;
                    if (WG) x0g[(size_t)rr * K0 + k] = x;
                }
            }
            if (tid < PS_ROWS) {
                const float* o = rows + tid * D;
                float es, ec;
                sincos_det(deg2rad(o[5]), es, ec);                              // DAM:211 and DAM:79-80
                S.ego[tid] = make_float4(o[3], o[4], es, ec);
                S.mask[tid] = 0ull;
                if (tid == 0) S.count = 0;
            }
        }
        __syncthreads();

        // ---- (2) the policy: hidden layers (mlp_bwd_data_kernel's forward loop) ----
        for (int L = 0; L < NH; ++L) {
            const MlpLayer& ly = A.hid[L];
            mlp::f32x16 acc[RT][CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                const float b = ly.b[(ct0 + c) * 32 + i];
#pragma unroll
                for (int r = 0; r < RT; ++r)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[r][c][v] = b;
            }
            mlp::layer_chain<RT, CT>(a_row, 32 * RS, reinterpret_cast<const mlp::f32x4*>(ly.w), ly.k_pad >> 3, ct0, lane, acc);
            __syncthreads();                                              // every wave has read this layer's inputs
            if (WG) {
                float* xg = A.ws + A.x_off[L + 1] + trow * U;
                switch (A.hidden_act) {
                    case MLP_ACT_RELU: mlp::store_hidden<RT, CT, MLP_ACT_RELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
                    case MLP_ACT_ELU: mlp::store_hidden<RT, CT, MLP_ACT_ELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
                    case MLP_ACT_TANH: mlp::store_hidden<RT, CT, MLP_ACT_TANH>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
                    default: mlp::store_hidden<RT, CT, MLP_ACT_LINEAR>(lds, RS, HS, rt0, ct0, i, h, acc, xg, U); break;
                }
            } else {                                                      // forward only: the same values, LDS alone
                switch (A.hidden_act) {
                    case MLP_ACT_RELU: mlp::store_hidden<RT, CT, MLP_ACT_RELU>(lds, RS, HS, rt0, ct0, i, h, acc); break;
                    case MLP_ACT_ELU: mlp::store_hidden<RT, CT, MLP_ACT_ELU>(lds, RS, HS, rt0, ct0, i, h, acc); break;
                    case MLP_ACT_TANH: mlp::store_hidden<RT, CT, MLP_ACT_TANH>(lds, RS, HS, rt0, ct0, i, h, acc); break;
                    default: mlp::store_hidden<RT, CT, MLP_ACT_LINEAR>(lds, RS, HS, rt0, ct0, i, h, acc); break;
                }
            }
            __syncthreads();
        }
        // the output layer as mlp_kernel runs it (16 x 16 x 4 tiles, row tile = wave; out_dim = 4: one column tile)
        {
            const int i16 = lane & 15, kq = lane >> 4, hsel = kq >> 1;
            const int steps4 = A.outl.k_pad >> 4;
            const float* a_ptr = lds + (wave * 16 + i16) * RS + (kq & 1) * HS;
            const float b = A.outl.b[i16];
            mlp::f32x4 acc = {b, b, b, b};
            const mlp::f32x4* wsrc = reinterpret_cast<const mlp::f32x4*>(A.outl.w) + lane;
            mlp::f32x4 bq = wsrc[0];
            for (int s4 = 0; s4 < steps4; ++s4) {
                const mlp::f32x4 bn = wsrc[(size_t)(s4 + 1 < steps4 ? s4 + 1 : s4) * 64];
                const mlp::f32x4 a01 = *reinterpret_cast<const mlp::f32x4*>(a_ptr + 8 * s4);
                const mlp::f32x4 a23 = *reinterpret_cast<const mlp::f32x4*>(a_ptr + 8 * s4 + 4);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a01[1] : a01[0], bq[0], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a01[3] : a01[2], bq[1], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a23[1] : a23[0], bq[2], acc, 0, 0, 0);
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(hsel ? a23[3] : a23[2], bq[3], acc, 0, 0, 0);
                bq = bn;
            }
            __syncthreads();                                                   // every wave has read x_H: the activation buffer is free
            if (i16 < 4) {                                                     // the row's activated mean0, mean1, ls0, ls1: one lane each
#pragma unroll
                for (int v = 0; v < 4; ++v) lds[(wave * 16 + 4 * kq + v) * PRS_LS + i16] = mlp::activate_rt(A.out_act, acc[v]);
            }
        }
        __syncthreads();
        // the stochastic head (eb_policy_sample.hip's epilogue): one lane per row, lanes 0..15 of each wave take the wave's own rows
        if (lane < 16) {
            const int row = wave * 16 + lane;
            float* y = lds + row * PRS_LS;                                     // [0..3] the logits; [4..6] the lane's eps and logp
            float* act = reinterpret_cast<float*>(&S.act[row]);
            const bool live = row < nE;
            if (live) {
                const size_t e = (size_t)(e0 + row), te = (size_t)t * n + e;
                const int32_t* row_ids = reinterpret_cast<const int32_t*>(hv_row_ids);
                const float* eps_in = reinterpret_cast<const float*>(hv_eps);
                float* logp_out = reinterpret_cast<float*>(hv_logp);
                float* eps_out = reinterpret_cast<float*>(hv_eps_out);
                const uint64_t key = splitmix64(hv_seed + 0x9E3779B97F4A7C15ull * (hv_counter + (uint64_t)t));
                const uint64_t id = (uint64_t)(uint32_t)(row_ids ? row_ids[e] : (int32_t)e);
                psample::sample_row(y, 2, eps_in ? eps_in + te * 2 : nullptr, key, id, A.action_range, hv_log_ar, act, y + 6, y + 4);
                if (A.actions_steps) *reinterpret_cast<float2*>(A.actions_steps + te * 2) = make_float2(act[0], act[1]);
                if (logp_out) logp_out[te] = y[6];
                if (eps_out) *reinterpret_cast<float2*>(eps_out + te * 2) = make_float2(y[4], y[5]);
            } else {
                act[0] = 0.0f; act[1] = 0.0f;                                  // rows beyond the batch: zero actions, a zero record
            }
            if (WG) {                                                          // what (R2) needs of the head
                float* T = tape + ((size_t)t * PRS_TAPE_FLOATS + 14) * np + row;
#pragma unroll
                for (int c = 0; c < 6; ++c) T[c * np] = live ? y[c] : 0.0f;    // mean0, mean1, ls0, ls1, eps0, eps1
            }
        }
        __syncthreads();                                                      // the logits are dead, the actions in LDS

        // (the thread's index, opaque from here to the end of the step: eb_policy_rollout.hip says why)
        int mt = tid;
        asm volatile("" : "+v"(mt));

        // ---- (3) near records into the queue, by index ----
        for (int base = 0; base < items; base += PS_THREADS) {                 // block-uniform
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
                if (near) {
                    queue[qb + __popcll(b & ((1ull << lane) - 1ull))] = (unsigned short)item;   // < items: an entry per record at most
                    atomicOr(&S.mask[env], 1ull << slot);                       // LDS
                }
            }
        }
        __syncthreads();

        // ---- (4) waves 1..3: the queue, one entry per thread | the env role: the env's own chain ----
        float rew = 0.0f, road_t = 0.0f, road_r = 0.0f;
        float hv[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        float st[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, trk[3] = {0.0f, 0.0f, 0.0f};
        float2 araw = make_float2(0.0f, 0.0f);
        if (mt >= PS_ROWS) {
            const int cnt = S.count;
            for (int q = mt - PS_ROWS; q < cnt; q += PS_THREADS - PS_ROWS) {
                const int item = queue[q];
                const int env = A.nv_magic ? (int)__umulhi((unsigned)item, A.nv_magic) : item, slot = item - env * NV;
                const float* r = rows + env * D + nd + 4 * slot;
                const float4 eg = S.ego[env];
                float vs, vc;
                sincos_det(deg2rad(r[3]), vs, vc);                              // DAM:221
                float t35[4], t25[4];
                const float4 pts = make_float4(eg.x + LWS * eg.w, eg.y + LWS * eg.z, eg.x - LWS * eg.w, eg.y - LWS * eg.z);
                veh2veh_terms(pts, r[0], r[1], vs, vc, t35, t25);               // DAM:218-229
                float px = 0.0f, py = 0.0f, pphi = 0.0f;
                grad::record_partials(eg.x, eg.y, eg.z, eg.w, r[0], r[1], vs, vc, w35, w25, px, py, pphi);
                pen35[item] = ((t35[0] + t35[1]) + t35[2]) + t35[3];
                pen25[item] = ((t25[0] + t25[1]) + t25[2]) + t25[3];
                ppx[item] = px; ppy[item] = py; ppphi[item] = pphi;
            }
        } else {
            const float* o = rows + mt * D;
#pragma unroll
            for (int c = 0; c < 6; ++c) st[c] = o[c];
            trk[0] = o[6]; trk[1] = o[7]; trk[2] = o[8];
            araw = S.act[mt];
            const float4 eg = S.ego[mt];
            const float es = eg.z, ec = eg.w, phi_rad = deg2rad(st[5]);
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

        // ---- (5) env role: sums in slot order, the step's outputs, the cost, the tape, the new head | every thread: its records ----
        if (mt < PS_ROWS) {
            float a35 = 0.0f, a25 = 0.0f, px = 0.0f, py = 0.0f, pphi = 0.0f;
            for (unsigned long long m = S.mask[mt]; m; m &= m - 1ull) {        // slot order: the same sum wherever the row sits
                const int it = mt * NV + (__ffsll((long long)m) - 1);
                a35 += pen35[it]; a25 += pen25[it];                             // DAM:218-229: far records add exact zeros
                px += ppx[it]; py += ppy[it]; pphi += ppphi[it];
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
            // s_t: the rows with a non-zero weight, in row order; J: ascending t from +0 (include/envbuild_cand.h)
            float s = 0.0f;
            bool any = false;
            if (w5_0 != 0.0f) { s = rew * w5_0; any = true; }
            if (w5_1 != 0.0f) { const float v = o1 * w5_1; s = any ? s + v : v; any = true; }
            if (w5_2 != 0.0f) { const float v = o2 * w5_2; s = any ? s + v : v; any = true; }
            if (w5_3 != 0.0f) { const float v = a25 * w5_3; s = any ? s + v : v; any = true; }
            if (w5_4 != 0.0f) { const float v = road_r * w5_4; s = any ? s + v : v; any = true; }
            if (any) S.J[mt] = S.J[mt] + s;
            if (WG) {
                float* T = tape + (size_t)t * PRS_TAPE_FLOATS * np + mt;       // mt < 64 <= n_pad - e0, t < H: inside the tape
#pragma unroll
                for (int c = 0; c < 6; ++c) T[c * np] = st[c];
#pragma unroll
                for (int c = 0; c < 3; ++c) T[(6 + c) * np] = trk[c];
                T[9 * np] = px; T[10 * np] = py; T[11 * np] = pphi;
                T[12 * np] = araw.x; T[13 * np] = araw.y;
            }
            float* o = rows + mt * D;
#pragma unroll
            for (int c = 0; c < 9; ++c) o[c] = hv[c];
        }
        const SinCosK SK = sincos_consts();
        for (int base = 0; base < items; base += PS_THREADS) {
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
            for (int idx = tid; idx < live; idx += PS_THREADS) dst[idx] = rows[idx];
        }
    }

    if (A.obs_out) {
        float* dst = A.obs_out + (size_t)e0 * D;
        const int live = nE * D;
        for (int idx = tid; idx < live; idx += PS_THREADS) dst[idx] = rows[idx];
    }
    if (tid < nE && A.cost) A.cost[e0 + tid] = S.J[tid];

    // =================================================== reverse ===================================================
    if (!WG) return;                                                           // block-uniform: forward only
    for (int t = H - 1; t >= 0; --t) {
        const size_t trow = (size_t)t * np + e0;
        const float* T = tape + (size_t)t * PRS_TAPE_FLOATS * np;
        // ---- (R1) the env role: tape_reverse's loop body on the step's record ----
        if (tid < PS_ROWS) {
            grad::EnvIn I;
            const float* Te = T + tid;
#pragma unroll
            for (int c = 0; c < 6; ++c) I.st[c] = Te[c * np];
#pragma unroll
            for (int c = 0; c < 3; ++c) I.trk[c] = Te[(6 + c) * np];
            I.px = Te[9 * np]; I.py = Te[10 * np]; I.pphi = Te[11 * np];
            I.a0 = Te[12 * np]; I.a1 = Te[13 * np];
            I.w[0] = w5_0; I.w[1] = w5_1; I.w[2] = w5_2; I.w[3] = w5_3; I.w[4] = w5_4;
            I.has_path = S.path[tid] >= 0;
#pragma unroll
            for (int c = 0; c < 9; ++c) I.g[c] = S.lam[c][tid];
            I.fx = I.fy = I.fphi = 0.0f;                                        // n_future == 0: no look-ahead columns
            grad::sincos_hd(grad::deg2rad_hd(I.st[5]), I.es, I.ec);             // DAM:211
            float go[9], ga[2];
            grad::env_vjp<TASK>(I, go, ga);
#pragma unroll
            for (int c = 0; c < 9; ++c) S.lam[c][tid] = go[c];
            S.act[tid] = make_float2(ga[0], ga[1]);
            if (tid < nE && A.g_actions_steps) {
                float* g = A.g_actions_steps + ((size_t)t * n + e0 + tid) * 2;
                g[0] = ga[0]; g[1] = ga[1];
            }
        }
        __syncthreads();                                                       // (also: waves 0, 1 are through with the last step's d_0)

        // ---- (R2) the cotangent of the output layer's pre-activations: eb_policy_sample_vjp's row (psample::sample_vjp_elem from g_a_t
        //      and w_logp), then mlp_bwd_data_kernel's head 0; exact zeros beyond the four logit columns and beyond the batch ----
        {
            float* dg = A.ws + A.d_off[NH] + trow * 32;
            for (int idx = tid; idx < PS_ROWS * 32; idx += PS_THREADS) {
                const int row = idx >> 5, col = idx & 31;
                float d = 0.0f;
                if (col < 4 && row < nE) {
                    const int a = col & 1;
                    const float mean = T[(size_t)(14 + a) * np + row], ls = T[(size_t)(16 + a) * np + row];
                    const float e = T[(size_t)(18 + a) * np + row];
                    float g_mean, g_ls;
                    psample::sample_vjp_elem(mean, ls, e, A.action_range, reinterpret_cast<const float*>(&S.act[row])[a], A.w_logp, g_mean, g_ls);
                    d = (col < 2 ? g_mean : g_ls) * mlp::derivative_rt(A.out_act, col < 2 ? mean : ls);
                }
                if (col < A.kt_out) lds[row * RS + (col & 1) * HS + (col >> 1)] = d;
                dg[idx] = d;
            }
        }
        __syncthreads();

        // ---- backwards: d_{L-1} = (d_L * W_L^T) (.) act'(x_L), the transposed packing as the B operand, no bias ----
        for (int L = NH; L >= 1; --L) {
            mlp::f32x16 acc[RT][CT];
#pragma unroll
            for (int c = 0; c < CT; ++c)
#pragma unroll
                for (int r = 0; r < RT; ++r)
#pragma unroll
                    for (int v = 0; v < 16; ++v) acc[r][c][v] = 0.0f;
            mlp::layer_chain<RT, CT>(a_row, 32 * RS, reinterpret_cast<const mlp::f32x4*>(A.wt[L]), (L == NH ? A.kt_out : U) >> 3, ct0, lane, acc);
            __syncthreads();                                              // every wave has read d_L
            const float* xg = A.ws + A.x_off[L] + trow * U;
            float* dg = A.ws + A.d_off[L - 1] + trow * U;
            switch (A.hidden_act) {
                case MLP_ACT_RELU: mlp::store_delta<RT, CT, MLP_ACT_RELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
                case MLP_ACT_ELU: mlp::store_delta<RT, CT, MLP_ACT_ELU>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
                case MLP_ACT_TANH: mlp::store_delta<RT, CT, MLP_ACT_TANH>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
                default: mlp::store_delta<RT, CT, MLP_ACT_LINEAR>(lds, RS, HS, rt0, ct0, i, h, acc, xg, dg, U); break;
            }
            __syncthreads();
        }

        // ---- (R3) (d_0 * W_0^T) (.) scale for column tile 0, one row tile per wave 0 and 1; columns 0..8 into lambda ----
        if (wave < 2) {
            mlp::f32x16 acc[1][1];
#pragma unroll
            for (int v = 0; v < 16; ++v) acc[0][0][v] = 0.0f;
            mlp::layer_chain<1, 1>(lds + (wave * 32 + i) * RS + h * HS, 32 * RS, reinterpret_cast<const mlp::f32x4*>(A.wt[0]), U >> 3, 0, lane, acc);
            if (i < 9) {
                const float sc = A.scale ? A.scale[i] : 1.0f;
#pragma unroll
                for (int v = 0; v < 16; ++v) {
                    const int row = wave * 32 + (v & 3) + 8 * (v >> 2) + 4 * h;
                    S.lam[i][row] = S.lam[i][row] + acc[0][0][v] * sc;          // lambda_t = s_t + p_t
                }
            }
        }
        __syncthreads();
    }

    if (tid < nE && A.g_obs0) {
        float* g = A.g_obs0 + (size_t)(e0 + tid) * 9;
#pragma unroll
        for (int c = 0; c < 9; ++c) g[c] = S.lam[c][tid];
    }
}

}  // namespace

size_t policy_rollout_sample_lds_bytes(int obs_dim, int n_veh, int row_stride) {
    const size_t actb = (size_t)PS_ROWS * row_stride * sizeof(float), scr = ps_scratch_bytes(n_veh);
    return ps_rows_bytes(obs_dim) + (actb > scr ? actb : scr);
}

size_t policy_rollout_sample_lds_limit() { return 160 * 1024 - sizeof(PsSmem) - 256; }   // a CU's LDS less the block's static part

hipError_t launch_policy_rollout_sample(int task, const PolicyRolloutSampleArgs& A, hipStream_t s) {
    if (A.n_env <= 0) return hipSuccess;
    if (A.units != 64 && A.units != 128 && A.units != 256) return hipErrorInvalidValue;   // refused by the caller before
    const dim3 g((A.n_env + PS_ROWS - 1) / PS_ROWS), b(PS_THREADS);
    const size_t lds = policy_rollout_sample_lds_bytes(A.obs_dim, A.n_veh, A.row_stride);
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        constexpr int T = decltype(t)::value;
        return A.units == 64 ? launch_lds<&policy_rollout_sample_kernel<T, 1, 1>>(g, b, lds, dev, s, A)
               : A.units == 128 ? launch_lds<&policy_rollout_sample_kernel<T, 2, 1>>(g, b, lds, dev, s, A)
                                : launch_lds<&policy_rollout_sample_kernel<T, 2, 2>>(g, b, lds, dev, s, A);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
