// eb_norm.hip — the only translation unit of libenvbuild_norm.so (include/envbuild_norm.h), gfx950: the running normalisation of
// observations and rewards — the batch sums, the merge into the running statistics and the normalisation itself.  None of the other six
// libraries holds this code, and it runs no network.
//
// norm_partial_kernel: block b takes the runs of 32 rows from 32 (b + k * blocks).  A run's 32 x D floats are ONE contiguous piece of x:
// all 256 lanes stage it in LDS, consecutive lanes on consecutive elements, as float4s when x is 16-byte aligned (a run starts 128 D
// bytes further, so the alignment of the base is the alignment of every run) and as dwords otherwise; the floats behind the last whole
// quad of a partial run go as dwords.  Lane g * D + d then reads column d of the rows g, g + G, ... from LDS — consecutive lanes on
// consecutive banks — and sums (x - K) and its square in double.  The G sums of a column are folded by halving in LDS and one partial per
// block and column goes to the workspace.  The return column: the block's first 32 lanes, one row of every run each, their two loads
// issued ahead of the run's staging so that one memory latency covers both.
// norm_fold_kernel: one block; all 256 lanes fetch the partials into LDS, 64 KiB of whole blocks at a time with 32 independent loads per lane
// (a lane per column alone would wait one memory latency per handful of partials), and lane d adds column d's in ascending block order
// and merges (eb_norm_device.h: merge).
// norm_apply_kernel: block k takes the 32 rows from 32 k: mean_f and den_f once into LDS, then the block's contiguous 32 x D floats as
// float4s (x and y 16-byte aligned) or dwords; the selected rows the way collect_record_kernel copies its truncated ones — each of the
// four waves walks the rows wave, wave + 4, ..., and a row that is not selected costs one load of its mark; the rewards one lane per row.
// 32 rows: 4 096 envs are 128 blocks, 65 536 envs 2 048 (apply) or the partial kernel's cap of 512, each walking four runs.
// Plain C++, __syncthreads only, plain vector stores, 256-thread blocks, rows indexed in 64 bits.
#include "eb_norm.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_norm_device.h"

namespace eb {

__global__ __launch_bounds__(norm::THREADS) void norm_partial_kernel(const NormUpdateArgs A) {
    __shared__ __attribute__((aligned(16))) float tile[norm::ROWS * norm::MAX_DIM];
    __shared__ double s1[norm::THREADS], s2[norm::THREADS];
    const int t = threadIdx.x, D = A.D, W = D + 1;
    double* out = A.work + (size_t)blockIdx.x * 2 * W;
    const long long first = (long long)blockIdx.x * norm::ROWS, stride = (long long)gridDim.x * norm::ROWS;
    const bool has_x = A.x != nullptr, has_r = A.reward != nullptr;      // uniform over the launch
    const int G = norm::groups(D);
    const int g = t / D, d = t - g * D;
    const bool mine = has_x && g < G;                            // lane (g, d) owns column d
    const bool r_lane = has_r && t < norm::ROWS;                 // lane t owns row t of every run
    const double K = mine ? (double)A.obs_scale[d] : 0.0;
    const double Kr = r_lane ? (double)A.ret_scale[0] : 0.0;
    double a1 = 0.0, a2 = 0.0, r1 = 0.0, r2 = 0.0;
    for (long long row0 = first; row0 < A.n; row0 += stride) {  // uniform over the block
        const int rows = A.n - row0 < norm::ROWS ? (int)(A.n - row0) : norm::ROWS;
        const bool r_mine = r_lane && t < rows;
        float run = 0.0f, rew = 0.0f;
        if (r_mine) {                                            // in flight together with the run's observations
            run = A.ret_run[row0 + t];
            rew = A.reward[row0 + t];
        }
        if (has_x) {
            __syncthreads();                                     // the tile is free
            norm::stage_run(tile, A.x + row0 * D, rows * D, A.wide != 0, t);
            __syncthreads();
            if (mine) {
                for (int r = g; r < rows; r += G) {
                    const double v = (double)tile[r * D + d] - K;
                    a1 = a1 + v;
                    a2 = a2 + v * v;
                }
            }
        }
        if (r_mine) {
            const float R = run * A.gamma + rew;
            A.ret_run[row0 + t] = R;
            const double v = (double)R - Kr;
            r1 = r1 + v;
            r2 = r2 + v * v;
        }
    }
    if (has_x) {
        s1[t] = a1;
        s2[t] = a2;
        norm::fold_groups(s1, s2, g, d, G, D, mine);
        if (mine && g == 0) {
            out[d] = s1[d];
            out[W + d] = s2[d];
        }
    }
    if (has_r) {
        __syncthreads();                                         // s1 and s2 are free
        s1[t] = r1;
        s2[t] = r2;
        norm::fold_groups(s1, s2, t, 0, norm::ROWS, 1, r_lane);
        if (t == 0) {
            out[D] = s1[0];
            out[W + D] = s2[0];
        }
    }
}

__global__ __launch_bounds__(norm::THREADS) void norm_fold_kernel(const NormUpdateArgs A) {
    __shared__ double part[norm::FOLD_CHUNK];
    const int t = threadIdx.x, D = A.D, W = D + 1;
    const double N = (double)A.n;
    const bool obs_lane = A.x != nullptr && t < D;
    const bool ret_lane = A.reward != nullptr && t == (D < norm::THREADS ? D : 0);    // a lane without an observation column, if any
    const double count_obs = A.x != nullptr ? A.obs_stat[2 * D] : 0.0;               // (held before lane 0 rewrites it: a barrier follows)
    // the partials through LDS, a chunk of whole blocks at a time: all 256 lanes fetch — FOLD_DEPTH independent loads each — what the
    // few column lanes then add in ascending block order
    const int per = norm::FOLD_CHUNK / (2 * W);
    double S1 = 0.0, S2 = 0.0, R1 = 0.0, R2 = 0.0;
    for (int b0 = 0; b0 < A.blocks; b0 += per) {                // uniform over the block
        const int nb = A.blocks - b0 < per ? A.blocks - b0 : per;
        const int count = nb * 2 * W;
        const double* src = A.work + (size_t)b0 * 2 * W;
        double v[norm::FOLD_DEPTH];
#pragma unroll
        for (int j = 0; j < norm::FOLD_DEPTH; ++j) {
            const int i = t + j * norm::THREADS;
            v[j] = i < count ? src[i] : 0.0;
        }
        __syncthreads();                                         // part is free
#pragma unroll
        for (int j = 0; j < norm::FOLD_DEPTH; ++j) part[t + j * norm::THREADS] = v[j];
        __syncthreads();
        if (obs_lane) {
            for (int b = 0; b < nb; ++b) {
                S1 = S1 + part[(2 * b) * W + t];
                S2 = S2 + part[(2 * b + 1) * W + t];
            }
        }
        if (ret_lane) {
            for (int b = 0; b < nb; ++b) {
                R1 = R1 + part[(2 * b) * W + D];
                R2 = R2 + part[(2 * b + 1) * W + D];
            }
        }
    }
    if (obs_lane) {
        double mean = A.obs_stat[t], var = A.obs_stat[D + t];
        const double tot = norm::merge(S1, S2, (double)A.obs_scale[t], N, count_obs, mean, var);
        A.obs_stat[t] = mean;
        A.obs_stat[D + t] = var;
        A.obs_scale[t] = (float)mean;
        A.obs_scale[D + t] = norm::den_of(var, A.eps);
        if (t == 0) A.obs_stat[2 * D] = tot;
    }
    if (ret_lane) {
        double mean = A.ret_stat[0], var = A.ret_stat[1];
        const double tot = norm::merge(R1, R2, (double)A.ret_scale[0], N, A.ret_stat[2], mean, var);
        A.ret_stat[0] = mean;
        A.ret_stat[1] = var;
        A.ret_stat[2] = tot;
        A.ret_scale[0] = (float)mean;
        A.ret_scale[1] = norm::den_of(var, A.eps);
    }
}

hipError_t launch_norm_update(const NormUpdateArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(norm_partial_kernel, dim3((unsigned)A.blocks), dim3(norm::THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(norm_fold_kernel, dim3(1), dim3(norm::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(norm::THREADS) void norm_apply_kernel(const NormApplyArgs A) {
    __shared__ float mean_s[norm::MAX_DIM], den_s[norm::MAX_DIM];
    const int t = threadIdx.x, D = A.D;
    const long long row0 = (long long)blockIdx.x * norm::ROWS;
    const int rows = A.n - row0 < norm::ROWS ? (int)(A.n - row0) : norm::ROWS;
    if (A.x != nullptr || A.sel_x != nullptr) {                 // uniform over the launch
        for (int c = t; c < D; c += norm::THREADS) {
            mean_s[c] = A.obs_scale[c];
            den_s[c] = A.obs_scale[D + c];
        }
        __syncthreads();
    }
    if (A.reward != nullptr && t < rows) {
        const long long i = row0 + t;
        A.reward_out[i] = norm::clip(A.reward[i] / A.ret_scale[1], A.clip_rew);
        if (A.done_code != nullptr) {
            const float R = A.ret_run[i];
            A.ret_run[i] = A.done_code[i] != 0 ? 0.0f : R;
        }
    }
    if (A.x != nullptr) {
        const long long at = row0 * D;
        const float* src = A.x + at;                             // (y may be x: no __restrict__)
        float* dst = A.y + at;
        const int n = rows * D;
        int done = 0;
        if (A.wide) {
            const int quads = n >> 2;
            const float4* s4 = reinterpret_cast<const float4*>(src);
            float4* d4 = reinterpret_cast<float4*>(dst);
            for (int q = t; q < quads; q += norm::THREADS) {
                float4 v = s4[q];
                int c = (int)((unsigned)(4 * q) % (unsigned)D);  // the run starts at a row's first column
                v.x = norm::normalise(v.x, mean_s[c], den_s[c], A.clip_obs);
                c = c + 1 == D ? 0 : c + 1;
                v.y = norm::normalise(v.y, mean_s[c], den_s[c], A.clip_obs);
                c = c + 1 == D ? 0 : c + 1;
                v.z = norm::normalise(v.z, mean_s[c], den_s[c], A.clip_obs);
                c = c + 1 == D ? 0 : c + 1;
                v.w = norm::normalise(v.w, mean_s[c], den_s[c], A.clip_obs);
                d4[q] = v;
            }
            done = quads << 2;
        }
        for (int e = done + t; e < n; e += norm::THREADS) {
            const int c = (int)((unsigned)e % (unsigned)D);
            dst[e] = norm::normalise(src[e], mean_s[c], den_s[c], A.clip_obs);
        }
    }
    if (A.sel_x != nullptr) {
        const int wave = t >> 6, lane = t & 63;
        for (int r = wave; r < rows; r += norm::THREADS / 64) {
            if (A.sel[row0 + r] == A.sel_value) {                // uniform over the wave
                const long long row = (row0 + r) * D;
                for (int c = lane; c < D; c += 64) A.sel_x[row + c] = norm::normalise(A.sel_x[row + c], mean_s[c], den_s[c], A.clip_obs);
            }
        }
    }
}

hipError_t launch_norm_apply(const NormApplyArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.n + norm::ROWS - 1) / norm::ROWS);
    hipLaunchKernelGGL(norm_apply_kernel, dim3(blocks), dim3(norm::THREADS), 0, s, A);
    return hipGetLastError();
}

}  // namespace eb

// ---- the C-ABI ----
namespace {

thread_local char g_err[512];

int fail(int code, const char* msg) {
    std::snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}
int fail_hip(const char* what, hipError_t e) {
    std::snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return EB_EDEVICE;
}
bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }
bool ok4(const void* p) { return p != nullptr && aligned(p, 4); }       // a needed pointer to 4-byte elements
bool ok8(const void* p) { return p != nullptr && aligned(p, 8); }       // ... to doubles
constexpr long long MOST = 2147483647LL;

}  // namespace

extern "C" {

int eb_norm_abi_version(void) { return EB_NORM_ABI_VERSION; }
const char* eb_norm_last_error(void) { return g_err; }

size_t eb_norm_workspace_bytes(int32_t dim) {
    if (dim < 1 || dim > EB_NORM_MAX_DIM) return 0;
    return (size_t)EB_NORM_MAX_BLOCKS * 2 * ((size_t)dim + 1) * sizeof(double);
}

int eb_norm_update(const eb_norm_update_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_norm_update: null args");
    if (a->n < 0) return fail(EB_EINVAL, "eb_norm_update: n must be in 0 .. 2^31 - 1");
    if (a->dim < 1 || a->dim > EB_NORM_MAX_DIM) return fail(EB_EINVAL, "eb_norm_update: dim must be in 1 .. 256");
    if ((long long)a->n * a->dim > MOST) return fail(EB_EINVAL, "eb_norm_update: n * dim exceeds 2^31 - 1");
    if (!std::isfinite(a->gamma) || !std::isfinite(a->eps)) return fail(EB_EINVAL, "eb_norm_update: gamma and eps must be finite");
    if (a->n == 0) return EB_OK;
    if (!a->x && !a->reward) return fail(EB_EINVAL, "eb_norm_update: neither x nor reward: nothing to update");
    if (!aligned(a->x, 4) || !aligned(a->reward, 4)) return fail(EB_EINVAL, "eb_norm_update: x or reward is not 4-byte aligned");
    if (a->x && (!ok8(a->obs_stat) || !ok4(a->obs_scale)))
        return fail(EB_EINVAL, "eb_norm_update: with x, null or misaligned obs_stat (8 bytes) or obs_scale (4)");
    if (a->reward && (!ok8(a->ret_stat) || !ok4(a->ret_scale) || !ok4(a->ret_run)))
        return fail(EB_EINVAL, "eb_norm_update: with reward, null or misaligned ret_stat (8 bytes), ret_scale or ret_run (4)");
    if (!ok8(a->workspace)) return fail(EB_EINVAL, "eb_norm_update: null or not 8-byte aligned workspace");
    eb::NormUpdateArgs A;
    A.x = a->x;
    A.obs_stat = a->obs_stat;
    A.obs_scale = a->obs_scale;
    A.reward = a->reward;
    A.ret_run = a->ret_run;
    A.ret_stat = a->ret_stat;
    A.ret_scale = a->ret_scale;
    A.work = a->workspace;
    A.n = a->n;
    A.D = a->dim;
    const long long runs = ((long long)a->n + eb::norm::ROWS - 1) / eb::norm::ROWS;
    A.blocks = (int)(runs < EB_NORM_MAX_BLOCKS ? runs : EB_NORM_MAX_BLOCKS);
    A.wide = aligned(a->x, 16) ? 1 : 0;
    A.gamma = a->gamma;
    A.eps = a->eps;
    const hipError_t e = eb::launch_norm_update(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_norm_update: launch", e);
    return EB_OK;
}

int eb_norm_apply(const eb_norm_apply_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_norm_apply: null args");
    if (a->n < 0) return fail(EB_EINVAL, "eb_norm_apply: n must be in 0 .. 2^31 - 1");
    if (a->dim < 1 || a->dim > EB_NORM_MAX_DIM) return fail(EB_EINVAL, "eb_norm_apply: dim must be in 1 .. 256");
    if ((long long)a->n * a->dim > MOST) return fail(EB_EINVAL, "eb_norm_apply: n * dim exceeds 2^31 - 1");
    if (!std::isfinite(a->clip_obs) || !std::isfinite(a->clip_rew)) return fail(EB_EINVAL, "eb_norm_apply: clip_obs and clip_rew must be finite");
    if (a->n == 0) return EB_OK;
    if (!a->x && !a->sel_x && !a->reward) return fail(EB_EINVAL, "eb_norm_apply: none of x, sel_x and reward: nothing to normalise");
    if (!aligned(a->x, 4) || !aligned(a->sel_x, 4) || !aligned(a->reward, 4))
        return fail(EB_EINVAL, "eb_norm_apply: x, sel_x or reward is not 4-byte aligned");
    if ((a->x || a->sel_x) && !ok4(a->obs_scale)) return fail(EB_EINVAL, "eb_norm_apply: with x or sel_x, null or not 4-byte aligned obs_scale");
    if (a->x && !ok4(a->y)) return fail(EB_EINVAL, "eb_norm_apply: with x, null or not 4-byte aligned y");
    if (a->sel_x && !ok4(a->sel)) return fail(EB_EINVAL, "eb_norm_apply: with sel_x, null or not 4-byte aligned sel");
    if (a->reward && (!ok4(a->ret_scale) || !ok4(a->reward_out)))
        return fail(EB_EINVAL, "eb_norm_apply: with reward, null or not 4-byte aligned ret_scale or reward_out");
    if ((a->done_code != nullptr) != (a->ret_run != nullptr) || !aligned(a->ret_run, 4))
        return fail(EB_EINVAL, "eb_norm_apply: done_code and ret_run (4-byte aligned) go together or not at all");
    if (a->done_code && !a->reward) return fail(EB_EINVAL, "eb_norm_apply: done_code and ret_run belong to the reward part");
    eb::NormApplyArgs A;
    A.obs_scale = a->obs_scale;
    A.x = a->x;
    A.y = a->y;
    A.sel_x = a->sel_x;
    A.sel = a->sel;
    A.ret_scale = a->ret_scale;
    A.reward = a->reward;
    A.reward_out = a->reward_out;
    A.done_code = a->done_code;
    A.ret_run = a->ret_run;
    A.n = a->n;
    A.D = a->dim;
    A.sel_value = a->sel_value;
    A.wide = a->x && aligned(a->x, 16) && aligned(a->y, 16) ? 1 : 0;
    A.clip_obs = a->clip_obs;
    A.clip_rew = a->clip_rew;
    const hipError_t e = eb::launch_norm_apply(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_norm_apply: launch", e);
    return EB_OK;
}

}  // extern "C"
