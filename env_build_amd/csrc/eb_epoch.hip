// eb_epoch.hip — the only translation unit of libenvbuild_epoch.so (include/envbuild_epoch.h), gfx950: what the update phase of a PPO
// iteration needs around the minibatch chain of libenvbuild_train.so — the minibatch gather under a keyed shuffle, the advantage
// statistics, the logging sums and the iteration counter.  Neither of the other two libraries holds this code.
//
// minibatch_gather_kernel: block k takes 32 destination rows.  Its first 32 lanes compute index(key, n_total, offset + row) — or read
// perm[offset + row] and check it — ONCE per row and share the 32 source rows through LDS.  Then, source by source, the block's
// 32 x width destination floats are one contiguous run that consecutive lanes write as coalesced dwords, 256 per pass; a lane's (row,
// column) moves from pass to pass by the host's THREADS / width and THREADS % width, so there is one division per source, not per float.
// The reads are coalesced inside each source row.  A source of width 1 or 2 goes one lane per row, each such source on another group of
// 32 lanes.  32 rows: a narrow source's 32 dwords are one 128-byte line, a 41-float source has five passes in flight per lane, and
// 4 x 4096 rows are 128 blocks.  Rows are views aligned to 4 bytes only, so there is no wider access.
// adv_stats_partial_kernel / adv_stats_fold_kernel: Adam's two-launch sum (eb_train.hip) on two doubles, S and Q, of the deviations from
// the first element.
// ppo_log_kernel: 64 blocks; lane t of block b walks the rows b * 256 + t + k * 16384 and the block folds its eight doubles by halving.
// epoch_advance_kernel: one lane adds to the counter.
// Plain C++, __syncthreads only, plain vector stores, 256-thread blocks, rows indexed in 64 bits.
#include "eb_epoch.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_epoch_device.h"

namespace eb {

__global__ __launch_bounds__(epoch::THREADS) void minibatch_gather_kernel(const GatherArgs A) {
    constexpr int ROWS = EB_EPOCH_GATHER_ROWS;
    __shared__ int from_row[ROWS];
    const int t = threadIdx.x;
    const long long row0 = (long long)blockIdx.x * ROWS;
    const int rows = A.count - row0 < ROWS ? (int)(A.count - row0) : ROWS;
    if (t < rows) {
        const long long slot = A.offset + row0 + t;
        int from;
        if (A.perm) {
            const long long v = A.perm_bytes == 8 ? ((const long long*)A.perm)[slot] : (long long)((const int*)A.perm)[slot];
            from = v >= 0 && v < (long long)A.n_total ? (int)v : -1;
        } else {
            const uint64_t base = A.counter ? (uint64_t)*A.counter : 0;
            from = (int)epoch::index(epoch::epoch_key(A.seed, A.epoch, base), A.n_total, A.h, A.mask, (uint32_t)slot);
        }
        from_row[t] = from;
        if (A.index_out) A.index_out[row0 + t] = from;
    }
    __syncthreads();
    const float quiet_nan = __int_as_float(0x7FC00000);
    int narrow = 0;
    for (int k = 0; k < A.n_sources; ++k) {
        const GatherSource S = A.s[k];
        float* dst = S.dst + (size_t)row0 * (size_t)S.width;
        if (S.width <= 2) {                                      // uniform over the launch: one lane per row
            const int r = t - ROWS * (narrow & 7);
            ++narrow;
            if (r >= 0 && r < rows) {
                const int from = from_row[r];
                for (int c = 0; c < S.width; ++c) {
                    float x = quiet_nan;
                    if (from >= 0) x = S.src[(size_t)from * (size_t)S.width + c];
                    dst[r * S.width + c] = x;
                }
            }
            continue;
        }
        const int total = rows * S.width;
        int r = t / S.width, c = t - r * S.width;
        for (int e = t; e < total; e += epoch::THREADS) {
            const int from = from_row[r];
            float x = quiet_nan;
            if (from >= 0) x = S.src[(size_t)from * (size_t)S.width + c];
            dst[e] = x;
            r += S.rows_per_pass;
            c += S.rest_per_pass;
            if (c >= S.width) {
                c -= S.width;
                ++r;
            }
        }
    }
}

hipError_t launch_gather(const GatherArgs& A, hipStream_t s) {
    if (A.count <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)((A.count + EB_EPOCH_GATHER_ROWS - 1) / EB_EPOCH_GATHER_ROWS);
    hipLaunchKernelGGL(minibatch_gather_kernel, dim3(blocks), dim3(epoch::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(epoch::THREADS) void adv_stats_partial_kernel(const AdvStatsArgs A) {
    __shared__ double red[epoch::THREADS];
    const int t = threadIdx.x;
    const double shift = (double)A.x[0];                        // uniform: every deviation below is taken from the first element
    double s = 0.0, q = 0.0;
    for (int c = blockIdx.x; c < A.chunks; c += A.parts) {
        const long long base = (long long)c * epoch::CHUNK + t;
#pragma unroll
        for (int k = 0; k < epoch::CHUNK / epoch::THREADS; ++k) {
            const long long i = base + k * epoch::THREADS;
            if (i < A.n) {
                const double d = (double)A.x[i] - shift;
                s = s + d;
                q = q + d * d;
            }
        }
    }
    const double S = epoch::fold(red, t, s);
    const double Q = epoch::fold(red, t, q);
    if (t == 0) {
        A.partials[blockIdx.x] = S;
        A.partials[EB_EPOCH_PARTIALS + blockIdx.x] = Q;
    }
}

__global__ __launch_bounds__(epoch::THREADS) void adv_stats_fold_kernel(const AdvStatsArgs A) {
    __shared__ double red[epoch::THREADS];
    const int t = threadIdx.x;
    const double S = epoch::fold(red, t, t < A.parts ? A.partials[t] : 0.0);
    const double Q = epoch::fold(red, t, t < A.parts ? A.partials[EB_EPOCH_PARTIALS + t] : 0.0);
    if (t == 0) {
        const double n = (double)A.n;
        const double v = (Q - S * S / n) / (n - 1.0);
        const double var = v < 0.0 ? 0.0 : v;                    // a select: a NaN travels
        const float sd = (float)sqrt(var);
        A.out[0] = (float)((double)A.x[0] + S / n);
        A.out[1] = 1.0f / (sd + A.eps);
        if (A.std_out) A.std_out[0] = sd;
    }
}

hipError_t launch_adv_stats(const AdvStatsArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(adv_stats_partial_kernel, dim3(A.parts), dim3(epoch::THREADS), 0, s, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(adv_stats_fold_kernel, dim3(1), dim3(epoch::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(epoch::THREADS) void ppo_log_kernel(const PpoLogArgs A) {
    __shared__ double red[epoch::THREADS];
    const int t = threadIdx.x;
    const bool kl = A.logp != nullptr && A.logp_old != nullptr;
    double surr = 0.0, vloss = 0.0, ent = 0.0, clipped = 0.0, diff = 0.0, top = 0.0, bad = 0.0, rows = 0.0;
    for (long long i = (long long)blockIdx.x * epoch::THREADS + t; i < A.n; i += (long long)EB_EPOCH_LOG_BLOCKS * epoch::THREADS) {
        bool ok = true;
        if (A.surr) {
            const float x = A.surr[i];
            surr = surr + (double)x;
            ok = ok && epoch::finite(x);
        }
        if (A.vloss) {
            const float x = A.vloss[i];
            vloss = vloss + (double)x;
            ok = ok && epoch::finite(x);
        }
        if (A.ent) {
            const float x = A.ent[i];
            ent = ent + (double)x;
            ok = ok && epoch::finite(x);
        }
        if (A.ratio) {
            const float x = A.ratio[i];
            const float dev = fabsf(x - 1.0f);
            if (dev > A.clip) clipped = clipped + 1.0;
            const double d = (double)dev;
            top = d > top ? d : top;                             // a NaN is passed over
            ok = ok && epoch::finite(x);
        }
        float lp = 0.0f, lo = 0.0f;
        if (A.logp) {
            lp = A.logp[i];
            ok = ok && epoch::finite(lp);
        }
        if (A.logp_old) {
            lo = A.logp_old[i];
            ok = ok && epoch::finite(lo);
        }
        if (kl) diff = diff + (double)(lo - lp);
        if (!ok) bad = bad + 1.0;
        rows = rows + 1.0;
    }
    double out[EB_EPOCH_LOG_FIELDS];
    out[0] = epoch::fold(red, t, surr);
    out[1] = epoch::fold(red, t, vloss);
    out[2] = epoch::fold(red, t, ent);
    out[3] = epoch::fold(red, t, clipped);
    out[4] = epoch::fold(red, t, diff);
    out[5] = epoch::fold_max(red, t, top);
    out[6] = epoch::fold(red, t, bad);
    out[7] = epoch::fold(red, t, rows);
    if (t < EB_EPOCH_LOG_FIELDS) {
        double mine = out[0];
#pragma unroll
        for (int k = 1; k < EB_EPOCH_LOG_FIELDS; ++k) mine = t == k ? out[k] : mine;
        A.out[blockIdx.x * EB_EPOCH_LOG_FIELDS + t] = mine;
    }
}

hipError_t launch_ppo_log(const PpoLogArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ppo_log_kernel, dim3(EB_EPOCH_LOG_BLOCKS), dim3(epoch::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(epoch::THREADS) void epoch_advance_kernel(unsigned long long* counter, unsigned long long by) {
    if (blockIdx.x == 0 && threadIdx.x == 0) counter[0] = counter[0] + by;
}

hipError_t launch_epoch_advance(unsigned long long* counter, unsigned long long by, hipStream_t s) {
    hipLaunchKernelGGL(epoch_advance_kernel, dim3(1), dim3(epoch::THREADS), 0, s, counter, by);
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
bool count_ok(long long n) { return n >= 0 && n <= 2147483647LL; }

}  // namespace

static_assert(sizeof(eb::GatherArgs) <= 4096, "kernel arguments");

extern "C" {

int eb_epoch_abi_version(void) { return EB_EPOCH_ABI_VERSION; }
const char* eb_epoch_last_error(void) { return g_err; }

int eb_minibatch_gather(const eb_gather_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_minibatch_gather: null args");
    if (!count_ok(a->n_total) || !count_ok(a->offset) || !count_ok(a->count))
        return fail(EB_EINVAL, "eb_minibatch_gather: n_total, offset and count must be in 0 .. 2^31 - 1");
    if (a->offset + a->count > a->n_total) return fail(EB_EINVAL, "eb_minibatch_gather: offset + count exceeds n_total");
    if (a->n_sources < 1 || a->n_sources > EB_EPOCH_MAX_SOURCES)
        return fail(EB_EINVAL, "eb_minibatch_gather: n_sources must be in 1 .. EB_EPOCH_MAX_SOURCES (8)");
    for (int k = 0; k < a->n_sources; ++k)
        if (a->sources[k].width < 1 || a->sources[k].width > EB_EPOCH_MAX_WIDTH)
            return fail(EB_EINVAL, "eb_minibatch_gather: a source's width must be in 1 .. EB_EPOCH_MAX_WIDTH (4096)");
    if (a->count == 0) return EB_OK;
    eb::GatherArgs A;
    for (int k = 0; k < EB_EPOCH_MAX_SOURCES; ++k) {
        if (k >= a->n_sources) {
            A.s[k] = eb::GatherSource{nullptr, nullptr, 1, 0, 0};
            continue;
        }
        const eb_gather_source& g = a->sources[k];
        if (!g.src || !g.dst || !aligned(g.src, 4) || !aligned(g.dst, 4))
            return fail(EB_EINVAL, "eb_minibatch_gather: null or not 4-byte aligned src or dst of a source");
        A.s[k] = eb::GatherSource{g.src, g.dst, g.width, eb::epoch::THREADS / g.width, eb::epoch::THREADS % g.width};
    }
    if (a->perm && a->perm_bytes != 4 && a->perm_bytes != 8) return fail(EB_EINVAL, "eb_minibatch_gather: perm_bytes must be 4 or 8");
    if (a->perm && !aligned(a->perm, (uintptr_t)a->perm_bytes)) return fail(EB_EINVAL, "eb_minibatch_gather: perm is not aligned to its element");
    if (!aligned(a->counter, 8) || !aligned(a->index_out, 4))
        return fail(EB_EINVAL, "eb_minibatch_gather: counter must be 8-byte and index_out 4-byte aligned");
    int bits = 0;                                                // bit_length(n_total - 1)
    for (unsigned long long v = (unsigned long long)(a->n_total - 1); v; v >>= 1) ++bits;
    if (bits < 2) bits = 2;
    bits += bits & 1;
    A.h = bits / 2;
    A.mask = (1u << A.h) - 1u;
    A.perm = a->perm;
    A.perm_bytes = a->perm ? a->perm_bytes : 0;
    A.counter = (const unsigned long long*)a->counter;
    A.index_out = a->index_out;
    A.seed = a->seed;
    A.epoch = a->epoch;
    A.offset = a->offset;
    A.count = a->count;
    A.n_total = (unsigned)a->n_total;
    A.n_sources = a->n_sources;
    const hipError_t e = eb::launch_gather(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_minibatch_gather: launch", e);
    return EB_OK;
}

int eb_adv_stats(const eb_adv_stats_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_adv_stats: null args");
    if (!count_ok(a->n) || a->n == 1) return fail(EB_EINVAL, "eb_adv_stats: n must be 0 or in 2 .. 2^31 - 1 (the unbiased variance needs two)");
    if (a->eps != a->eps) return fail(EB_EINVAL, "eb_adv_stats: eps is NaN");
    if (a->n == 0) return EB_OK;
    if (!a->x || !a->out || !aligned(a->x, 4) || !aligned(a->out, 4) || !aligned(a->std_out, 4))
        return fail(EB_EINVAL, "eb_adv_stats: null or not 4-byte aligned x or out, or std_out not 4-byte aligned");
    if (!a->partials || !aligned(a->partials, 8)) return fail(EB_EINVAL, "eb_adv_stats: null or not 8-byte aligned partials");
    eb::AdvStatsArgs A;
    A.x = a->x;
    A.out = a->out;
    A.std_out = a->std_out;
    A.partials = a->partials;
    A.n = a->n;
    const long long chunks = (a->n + eb::epoch::CHUNK - 1) / eb::epoch::CHUNK;
    A.chunks = (int)chunks;
    A.parts = chunks < EB_EPOCH_PARTIALS ? (int)chunks : EB_EPOCH_PARTIALS;
    A.eps = (float)a->eps;
    const hipError_t e = eb::launch_adv_stats(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_adv_stats: launch", e);
    return EB_OK;
}

int eb_ppo_log(const eb_ppo_log_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_ppo_log: null args");
    if (!count_ok(a->n)) return fail(EB_EINVAL, "eb_ppo_log: n must be in 0 .. 2^31 - 1");
    if (a->clip != a->clip) return fail(EB_EINVAL, "eb_ppo_log: clip is NaN");
    if (a->n == 0) return EB_OK;
    if (!aligned(a->logp, 4) || !aligned(a->logp_old, 4) || !aligned(a->ratio, 4) || !aligned(a->surr, 4) || !aligned(a->ent, 4) ||
        !aligned(a->vloss, 4))
        return fail(EB_EINVAL, "eb_ppo_log: an input is not 4-byte aligned");
    if (!a->out || !aligned(a->out, 8)) return fail(EB_EINVAL, "eb_ppo_log: null or not 8-byte aligned out");
    const eb::PpoLogArgs A{a->logp, a->logp_old, a->ratio, a->surr, a->ent, a->vloss, a->out, (long long)a->n, a->clip};
    const hipError_t e = eb::launch_ppo_log(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_ppo_log: launch", e);
    return EB_OK;
}

int eb_epoch_advance(const eb_epoch_advance_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_epoch_advance: null args");
    if (!a->counter || !aligned(a->counter, 8)) return fail(EB_EINVAL, "eb_epoch_advance: null or not 8-byte aligned counter");
    const hipError_t e = eb::launch_epoch_advance((unsigned long long*)a->counter, (unsigned long long)a->by, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_epoch_advance: launch", e);
    return EB_OK;
}

}  // extern "C"
