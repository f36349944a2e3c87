// eb_rollout_vjp.hip — reverse pass of the fused rollout step (eb_rollout_step): one launch per step, gfx950.
//
// Recomputes from the pre-step obs and the raw actions; the forward kernels save nothing for it.  fp32 state only.
//
// A block of 256 threads owns 64 consecutive envs:
//   first    every lane requests its (env, vehicle) records — 2^lg lanes per env (2^lg >= n_veh, at most 64), one 16-byte record
//            per lane and pass over the block, up to eight passes in flight — so that their latency hides behind phase 0;
//   phase 0  thread e < 64 (wave 0) loads env e's head (ego 6 | tracking 3), action, path id and cotangents, and publishes the
//            ego pose (x, y, sin phi, cos phi) and the two penalty weights to LDS;
//   phase 1  all four waves test their records: a record whose centre is within 6.31 m of the ego (DAM:228: no circle pair can
//            be closer than 3.5 m otherwise) goes into the block's near-record queue in LDS (ballot + one LDS add per wave), its
//            queue position into a per-(env, slot) table, its bit into the env's slot mask.  A few per cent of the records are
//            near, spread over every wave: evaluated in place, each wave would run the four-distance code for a handful of lanes.
//            With ld_in == D the same lanes zero-fill the vehicle columns (stop_gradient, DAM:195, 331, 402);
//   phase 1b the queue, one entry per thread: the four circle distances x two thresholds of that record (DAM:218-229) -> its
//            three ego partials (x, y, heading), left in the entry's place;
//   phase 2  wave 0, one lane per env: the env's partials summed in SLOT order (its mask's bits, lowest first), then dynamics,
//            tracking, walls, rewards and the action transform transposed (eb_grad_device.h), plain vector stores of the
//            nd + 2 results.
// The queue's order varies from run to run; the sums do not: a row's bits depend on nothing but the row.  No atomics to global
// memory, no scratch.
#include <hip/hip_runtime.h>

#include "eb_grad.h"
#include "eb_grad_device.h"

namespace eb {
namespace {

constexpr int VJP_THREADS = 256, VJP_ENVS = 64;
typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));

struct VjpSmem {
    float4 ego[VJP_ENVS];                 // x, y, sin phi, cos phi of the pre-step pose
    float2 w[VJP_ENVS];                   // cotangents of the 3.5 m and the 2.5 m penalty sums
    unsigned long long mask[VJP_ENVS];    // per env: slots with a near record
    int count;                            // entries in the near-record queue
};
// dynamic LDS: the queue — 64 * n_veh entries (x, y, heading, env) that become (gx, gy, gphi, -) — then the queue position of
// every (env, slot), 16 bits each
inline size_t vjp_lds_bytes(int n_veh) { return (size_t)VJP_ENVS * n_veh * (sizeof(float4) + sizeof(unsigned short)); }

template <int TASK>
__global__ __launch_bounds__(VJP_THREADS) void rollout_step_vjp_kernel(const VjpArgs A) {
    __shared__ VjpSmem S;
    extern __shared__ __align__(16) unsigned char vjp_dyn[];
    float4* const queue = reinterpret_cast<float4*>(vjp_dyn);
    unsigned short* const qpos = reinterpret_cast<unsigned short*>(vjp_dyn + (size_t)VJP_ENVS * A.n_veh * sizeof(float4));
    const int tid = threadIdx.x;
    const int e0 = blockIdx.x * VJP_ENVS;
    const int D = A.obs_dim, nd = A.nd, NV = A.n_veh;
    const size_t n = (size_t)A.n_env;

    // ---- the block's records: requested before anything else, used after phase 0 (2^lg lanes per env, one record per lane and pass) ----
    const int lg = A.lg, L = 1 << lg, l = tid & (L - 1);
    const int per_pass = VJP_THREADS >> lg, grp = tid >> lg;      // envs per pass over the block; this lane's env in a pass
    const int passes = per_pass >= VJP_ENVS ? 1 : VJP_ENVS / per_pass;
    const bool pen = A.g_out5 != nullptr;
    const bool fill = A.ld_in == D;          // full-width rows: the vehicle columns are zero-filled
    constexpr int CH = 8;                    // records in flight per lane: all of them up to 32 slots, two rounds at 64
    f4u rec[CH];
    auto request = [&](int pass0) {
#pragma unroll
        for (int u = 0; u < CH; ++u) {
            const int el = grp + (pass0 + u) * per_pass;
            rec[u] = f4u{0.0f, 0.0f, 0.0f, 0.0f};
            if (pass0 + u < passes && el < VJP_ENVS && l < NV)
                rec[u] = *reinterpret_cast<const f4u*>(A.obs + (size_t)min(e0 + el, A.n_env - 1) * D + nd + 4 * l);
        }
    };
    if (pen) request(0);

    // ---- phase 0: wave 0, one lane per env ----
    grad::EnvIn I;
    const bool env_lane = tid < VJP_ENVS;
    const bool act = env_lane && e0 + tid < A.n_env;
    const int ge = min(e0 + tid, A.n_env - 1);       // inactive lanes re-read the last env (in bounds), store nothing
    if (env_lane) {
        const float* o = A.obs + (size_t)ge * D;
        const f4u h0 = *reinterpret_cast<const f4u*>(o), h1 = *reinterpret_cast<const f4u*>(o + 4);
        const float h8 = o[8];
        const f2u araw = *reinterpret_cast<const f2u*>(A.actions + 2 * (size_t)ge);
        I.st[0] = h0.x; I.st[1] = h0.y; I.st[2] = h0.z; I.st[3] = h0.w; I.st[4] = h1.x; I.st[5] = h1.y;
        I.trk[0] = h1.z; I.trk[1] = h1.w; I.trk[2] = h8;
        I.a0 = araw.x; I.a1 = araw.y;
        int p = A.path_id;
        if (A.training) p = A.ref_idx[ge];
        I.has_path = p >= 0 && p < A.n_paths;                                  // DAM:342, 352
#pragma unroll
        for (int c = 0; c < 9; ++c) I.g[c] = 0.0f;
        I.fx = I.fy = I.fphi = 0.0f;
        if (A.g_obs_out) {
            const float* g = A.g_obs_out + (size_t)ge * A.ld_out;
#pragma unroll
            for (int c = 0; c < 9; ++c) I.g[c] = g[c];
            for (int k = 0; k < A.n_future; ++k) {                             // DAM:763-768
                I.fx += g[9 + 3 * k]; I.fy += g[10 + 3 * k]; I.fphi += g[11 + 3 * k];
            }
        }
#pragma unroll
        for (int k = 0; k < 5; ++k) I.w[k] = A.g_out5 ? A.g_out5[k * n + ge] : 0.0f;
        grad::sincos_hd(grad::deg2rad_hd(I.st[5]), I.es, I.ec);               // DAM:211
        S.ego[tid] = make_float4(I.st[3], I.st[4], I.es, I.ec);
        S.w[tid] = make_float2(I.w[1], I.w[2] + I.w[3]);                       // DAM:299-300 and veh2veh4real itself
        S.mask[tid] = 0ull;
        if (tid == 0) S.count = 0;
    }
    __syncthreads();

    // ---- phase 1: near records into the queue ----
    if (pen || fill) {
        const int lane = tid & 63;
        for (int pass0 = 0; pass0 < passes; pass0 += CH) {
            if (pen && pass0 > 0) request(pass0);
#pragma unroll
            for (int u = 0; u < CH; ++u) {
                const int el = grp + (pass0 + u) * per_pass;
                if (pass0 + u >= passes || el >= VJP_ENVS) break;        // wave-uniform: a wave's lanes share the pass count
                const bool valid = e0 + el < A.n_env && l < NV;          // (trailing envs of the last block idle)
                bool near = false;
                if (pen && valid) {
                    const float4 eg = S.ego[el];
                    const float cx = eg.x - rec[u].x, cy = eg.y - rec[u].y;
                    near = cx * cx + cy * cy < grad::NEAR_R * grad::NEAR_R;
                }
                if (fill && valid)
                    *reinterpret_cast<f4u*>(A.g_obs_in + (size_t)(e0 + el) * D + nd + 4 * l) = f4u{0.0f, 0.0f, 0.0f, 0.0f};
                const unsigned long long b = __ballot(near);
                if (b != 0ull) {                 // wave-uniform; every lane of the wave is here
                    int base = 0;
                    if (lane == 0) base = atomicAdd(&S.count, __popcll(b));      // an LDS add: one per wave and pass
                    base = __builtin_amdgcn_readfirstlane(base);
                    if (near) {
                        const int pos = base + __popcll(b & ((1ull << lane) - 1ull));   // < 64 * n_veh: one entry per record at most
                        queue[pos] = make_float4(rec[u].x, rec[u].y, rec[u].w, __int_as_float(el));
                        qpos[el * NV + l] = (unsigned short)pos;
                    }
                    if (l == 0) S.mask[el] = (b >> lane) & (L == 64 ? ~0ull : (1ull << L) - 1ull);   // the env's lanes start at this one
                }
            }
        }
    }
    __syncthreads();

    // ---- phase 1b: the queue, one entry per thread ----
    for (int q = tid; q < S.count; q += VJP_THREADS) {
        const float4 e = queue[q];
        const int el = __float_as_int(e.w);
        const float4 eg = S.ego[el];
        const float2 w = S.w[el];
        float vs, vc, px = 0.0f, py = 0.0f, pphi = 0.0f;
        grad::sincos_hd(grad::deg2rad_hd(e.z), vs, vc);                          // DAM:221
        grad::veh_pair_vjp(eg.x, eg.y, eg.z, eg.w, e.x, e.y, vs, vc, w.x, w.y, px, py, pphi);
        queue[q] = make_float4(px, py, pphi, 0.0f);
    }
    __syncthreads();
    if (!act) return;

    // ---- phase 2: the env's own part ----
    I.px = I.py = I.pphi = 0.0f;
    for (unsigned long long m = S.mask[tid]; m; m &= m - 1ull) {                 // slot order: the same sum wherever the row sits
        const float4 r = queue[qpos[tid * NV + (__ffsll((long long)m) - 1)]];
        I.px += r.x; I.py += r.y; I.pphi += r.z;
    }
    float go[9], ga[2];
    grad::env_vjp<TASK>(I, go, ga);
    float* gi = A.g_obs_in + (size_t)ge * A.ld_in;
    *reinterpret_cast<f4u*>(gi) = f4u{go[0], go[1], go[2], go[3]};
    *reinterpret_cast<f4u*>(gi + 4) = f4u{go[4], go[5], go[6], go[7]};
    gi[8] = go[8];
    for (int c = 9; c < nd; ++c) gi[c] = 0.0f;       // the pre-step look-ahead columns feed nothing (DAM:189-207, 322-333)
    *reinterpret_cast<f2u*>(A.g_actions + 2 * (size_t)ge) = f2u{ga[0], ga[1]};
}

}  // namespace

hipError_t launch_rollout_step_vjp(int task, const VjpArgs& A_in, hipStream_t s) {
    if (A_in.n_env <= 0) return hipSuccess;
    VjpArgs A = A_in;
    A.lg = 0;
    while ((1 << A.lg) < A.n_veh && A.lg < 6) ++A.lg;
    const int grid = (A.n_env + VJP_ENVS - 1) / VJP_ENVS;
    const size_t lds = vjp_lds_bytes(A.n_veh);       // 36 KB at 32 slots; 72 KB at 64 (behind the opt-in)
    const int dev = current_device_index();
    const hipError_t e = with_task(task, [&](auto t) {
        return launch_lds<rollout_step_vjp_kernel<decltype(t)::value>>(dim3(grid), dim3(VJP_THREADS), lds, dev, s, A);
    });
    return e != hipSuccess ? e : hipGetLastError();
}

}  // namespace eb
