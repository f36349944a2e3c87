// eb_ctl.hip — the only translation unit of libenvbuild_ctl.so (include/envbuild_ctl.h), gfx950: the two controls of a PPO update phase
// that must live on the device for a captured graph to obey them — the learning-rate factor of the iteration and the approximate-KL
// stop.  None of the other four libraries holds this code.
//
// ctl_begin_kernel: one lane opens the iteration — the factor from the caller's table, the stop cleared, the counter advanced.
// kl_partial_kernel: eb_ppo_log's field 4 alone, in its order — 64 blocks; lane t of block b walks the rows b * 256 + t + k * 16384 and the
// block folds its 256 doubles by halving into ONE partial.
// kl_fold_kernel: one lane adds the 64 partials in ascending order, decides, and writes the control block and the log slot.
// adam_norm_ctl_kernel / adam_update_ctl_kernel: eb_train.hip's two Adam launches on train::adam_element and train::fold, with the control
// block read first: stopped, launch 1 leaves the state alone and launch 2 returns before its first store (uniform over the launch); not
// stopped, the step's learning rate is lr * (double)lr_scale.
// Plain C++, __syncthreads only, no atomics, plain vector stores, 256-thread blocks, rows indexed in 64 bits.
#include "eb_ctl.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_ctl_device.h"

namespace eb {

__global__ __launch_bounds__(ctl::THREADS) void ctl_begin_kernel(const CtlBeginArgs A) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    eb_update_ctl* c = A.ctl;
    const unsigned long long it = c->iteration;
    float scale = 1.0f;
    if (A.table) {
        const unsigned long long last = (unsigned long long)(A.n_table - 1);
        scale = A.table[it < last ? it : last];
    }
    c->lr_scale = scale;
    c->stopped = 0u;
    c->slot = 0;
    c->stopped_at = -1;
    c->last_kl = 0.0;
    c->iteration = it + 1ull;
}

hipError_t launch_ctl_begin(const CtlBeginArgs& A, hipStream_t s) {
    hipLaunchKernelGGL(ctl_begin_kernel, dim3(1), dim3(ctl::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(ctl::THREADS) void kl_partial_kernel(const KlStopArgs A) {
    __shared__ double red[ctl::THREADS];
    const int t = threadIdx.x;
    double diff = 0.0;
    for (long long i = (long long)blockIdx.x * ctl::THREADS + t; i < A.n; i += (long long)ctl::KL_BLOCKS * ctl::THREADS)
        diff = diff + ctl::kl_row(A.logp_old[i], A.logp[i]);
    const double sum = train::fold(red, t, diff);
    if (t == 0) A.partials[blockIdx.x] = sum;
}

__global__ __launch_bounds__(ctl::THREADS) void kl_fold_kernel(const KlStopArgs A) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    double sum = A.partials[0];
    for (int b = 1; b < ctl::KL_BLOCKS; ++b) sum = sum + A.partials[b];
    const double kl = sum / (double)A.n;
    const bool stop_now = !(kl <= A.limit);                      // a NaN stops
    eb_update_ctl* c = A.ctl;
    const int s = c->slot;
    unsigned stopped = c->stopped;
    if (stopped == 0u && stop_now) {
        stopped = 1u;
        c->stopped = 1u;
        c->stopped_at = s;
    }
    if (A.log && s >= 0 && s < A.max_slots) {
        A.log[2 * (long long)s] = kl;
        A.log[2 * (long long)s + 1] = stopped ? 0.0 : 1.0;
    }
    c->slot = s + 1;
    c->last_kl = kl;
}

hipError_t launch_kl_stop(const KlStopArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(kl_partial_kernel, dim3(ctl::KL_BLOCKS), dim3(ctl::THREADS), 0, s, A);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(kl_fold_kernel, dim3(1), dim3(ctl::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(ctl::THREADS) void adam_norm_ctl_kernel(const CtlAdamArgs A) {
    __shared__ double red[ctl::THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int c = blockIdx.x; c < A.chunks; c += A.parts) {
        const int s = ctl::segment_of(A, c);
        const float* g = A.seg[s].g;
        const long long count = A.seg[s].count;
        const long long base = (long long)(c - A.chunk0[s]) * train::CHUNK + t;
#pragma unroll
        for (int k = 0; k < train::CHUNK / train::THREADS; ++k) {
            const long long i = base + k * train::THREADS;
            if (i < count) {
                const double x = (double)g[i];
                acc = acc + x * x;
            }
        }
    }
    const double sum = train::fold(red, t, acc);
    if (t == 0) {
        A.partials[blockIdx.x] = sum;                            // scratch: written whether stopped or not
        if (blockIdx.x == 0 && A.ctl->stopped == 0u) {           // the one lane that reads and advances the state
            eb_adam_state* S = A.state;
            const bool was0 = S->step == 0;
            const double b1t = (was0 ? 1.0 : S->b1t) * A.beta1;
            const double b2t = (was0 ? 1.0 : S->b2t) * A.beta2;
            S->step = S->step + 1;
            S->b1t = b1t;
            S->b2t = b2t;
        }
    }
}

__global__ __launch_bounds__(ctl::THREADS) void adam_update_ctl_kernel(const CtlAdamArgs A) {
    __shared__ double red[ctl::THREADS];
    if (A.ctl->stopped != 0u) return;                            // uniform over the launch: before the first store
    const int t = threadIdx.x;
    const double sum = train::fold(red, t, t < A.parts ? A.partials[t] : 0.0);
    const float gnorm = (float)sqrt(sum);
    train::AdamUniform U;
    U.coef = 1.0f;
    if (A.clip) {
        const float q = A.max_norm / (gnorm + 1e-6f);
        U.coef = q > 1.0f ? 1.0f : q;        // a select: a NaN q travels
    }
    const double b1t = A.state->b1t, b2t = A.state->b2t;     // as launch 1 left them; this launch only reads them
    const double lr = A.lr * (double)A.ctl->lr_scale;
    U.ss = (float)(lr / (1.0 - b1t));
    U.sb = (float)sqrt(1.0 - b2t);
    U.b1 = A.b1; U.b2 = A.b2; U.o1 = A.o1; U.o2 = A.o2; U.eps = A.eps; U.decay = A.decay;
    U.lwd = (float)(lr * A.weight_decay);
    if (blockIdx.x == 0 && t == 0) {
        A.state->gnorm = gnorm;
        A.state->coef = U.coef;
    }
    for (int c = blockIdx.x; c < A.chunks; c += gridDim.x) {
        const int s = ctl::segment_of(A, c);
        const CtlAdamSeg S = A.seg[s];
        const long long base = (long long)(c - A.chunk0[s]) * train::CHUNK + t;
#pragma unroll
        for (int k = 0; k < train::CHUNK / train::THREADS; ++k) {
            const long long i = base + k * train::THREADS;
            if (i < S.count) {
                float p = S.p[i], m = S.m[i], v = S.v[i];
                train::adam_element(U, S.g[i], p, m, v);
                S.p[i] = p;
                S.m[i] = m;
                S.v[i] = v;
            }
        }
    }
}

hipError_t launch_adam_step_ctl(const CtlAdamArgs& A, hipStream_t s) {
    if (A.chunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_norm_ctl_kernel, dim3(A.parts), dim3(ctl::THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int blocks = A.chunks < 65536 ? A.chunks : 65536;      // beyond that a block walks its chunks with the grid's stride
    hipLaunchKernelGGL(adam_update_ctl_kernel, dim3(blocks), dim3(ctl::THREADS), 0, s, A);
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

}  // namespace

static_assert(sizeof(eb_update_ctl) == 32, "eb_update_ctl is 32 bytes");
static_assert(sizeof(eb_adam_state) == 32, "eb_adam_state is 32 bytes");
static_assert(sizeof(eb::CtlAdamArgs) <= 4096, "kernel arguments");
static_assert(eb::train::THREADS == 256 && EB_CTL_KL_BLOCKS == 64, "eb_ppo_log's cut of the rows");

extern "C" {

int eb_ctl_abi_version(void) { return EB_CTL_ABI_VERSION; }
const char* eb_ctl_last_error(void) { return g_err; }

int eb_ctl_begin(const eb_ctl_begin_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_ctl_begin: null args");
    if (!a->ctl || !aligned(a->ctl, 8)) return fail(EB_EINVAL, "eb_ctl_begin: null or not 8-byte aligned ctl");
    if (a->lr_table && (!aligned(a->lr_table, 4) || a->n_table < 1))
        return fail(EB_EINVAL, "eb_ctl_begin: lr_table must be 4-byte aligned and hold n_table >= 1 factors");
    const eb::CtlBeginArgs A{a->ctl, a->lr_table, a->lr_table ? a->n_table : 0};
    const hipError_t e = eb::launch_ctl_begin(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_ctl_begin: launch", e);
    return EB_OK;
}

int eb_kl_stop(const eb_kl_stop_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_kl_stop: null args");
    if (a->n < 0 || a->n > 2147483647LL) return fail(EB_EINVAL, "eb_kl_stop: n must be in 0 .. 2^31 - 1");
    if (a->limit != a->limit) return fail(EB_EINVAL, "eb_kl_stop: limit is NaN");
    if (a->max_slots < 0) return fail(EB_EINVAL, "eb_kl_stop: max_slots must be >= 0");
    if (!a->ctl || !aligned(a->ctl, 8)) return fail(EB_EINVAL, "eb_kl_stop: null or not 8-byte aligned ctl");
    if (!aligned(a->log, 8)) return fail(EB_EINVAL, "eb_kl_stop: log is not 8-byte aligned");
    if (a->n == 0) return EB_OK;
    if (!a->logp || !a->logp_old || !aligned(a->logp, 4) || !aligned(a->logp_old, 4))
        return fail(EB_EINVAL, "eb_kl_stop: null or not 4-byte aligned logp or logp_old");
    if (!a->partials || !aligned(a->partials, 8)) return fail(EB_EINVAL, "eb_kl_stop: null or not 8-byte aligned partials");
    const eb::KlStopArgs A{a->logp, a->logp_old, a->partials, a->log, a->ctl, a->limit, (long long)a->n, a->max_slots};
    const hipError_t e = eb::launch_kl_stop(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_kl_stop: launch", e);
    return EB_OK;
}

int eb_adam_step_ctl(const eb_adam_ctl_args* c) {
    if (!c) return fail(EB_EINVAL, "eb_adam_step_ctl: null args");
    if (!c->ctl || !aligned(c->ctl, 8)) return fail(EB_EINVAL, "eb_adam_step_ctl: null or not 8-byte aligned ctl");
    const eb_adam_args* a = &c->adam;
    if (a->n_segments < 0 || a->n_segments > EB_TRAIN_MAX_SEGMENTS)
        return fail(EB_EINVAL, "eb_adam_step_ctl: n_segments must be in 0 .. EB_TRAIN_MAX_SEGMENTS (32)");
    if (!(a->lr >= 0.0) || !(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0) ||
        !(a->weight_decay >= 0.0) || a->max_grad_norm != a->max_grad_norm)
        return fail(EB_EINVAL, "eb_adam_step_ctl: bad scalar (lr, eps, weight_decay >= 0, beta1 and beta2 in [0, 1), none of them or "
                               "max_grad_norm NaN)");
    eb::CtlAdamArgs A;
    long long chunks = 0;
    for (int s = 0; s < EB_TRAIN_MAX_SEGMENTS; ++s) {
        A.chunk0[s] = (int)chunks;
        if (s >= a->n_segments) {
            A.seg[s] = eb::CtlAdamSeg{nullptr, nullptr, nullptr, nullptr, 0};
            continue;
        }
        const eb_adam_segment& g = a->segments[s];
        if (g.count < 0 || g.count > 2147483647LL) return fail(EB_EINVAL, "eb_adam_step_ctl: a segment's count must be in 0 .. 2^31 - 1");
        if (g.count > 0 && (!g.params || !g.grads || !g.m || !g.v || !aligned(g.params, 4) || !aligned(g.grads, 4) || !aligned(g.m, 4) ||
                            !aligned(g.v, 4)))
            return fail(EB_EINVAL, "eb_adam_step_ctl: null or not 4-byte aligned params, grads, m or v of a segment with count > 0");
        A.seg[s] = eb::CtlAdamSeg{g.params, g.grads, g.m, g.v, (long long)g.count};
        chunks += (g.count + eb::train::CHUNK - 1) / eb::train::CHUNK;
    }
    A.chunk0[EB_TRAIN_MAX_SEGMENTS] = (int)chunks;
    if (chunks == 0) return EB_OK;
    if (!a->state || !a->partials || !aligned(a->state, 8) || !aligned(a->partials, 8))
        return fail(EB_EINVAL, "eb_adam_step_ctl: null or not 8-byte aligned state or partials");
    A.n_seg = a->n_segments;
    A.chunk0[A.n_seg] = (int)chunks;
    A.chunks = (int)chunks;
    A.parts = chunks < EB_TRAIN_ADAM_PARTIALS ? (int)chunks : EB_TRAIN_ADAM_PARTIALS;
    A.clip = a->max_grad_norm > 0.0 && !std::isinf(a->max_grad_norm);
    A.max_norm = (float)a->max_grad_norm;
    A.b1 = (float)a->beta1; A.b2 = (float)a->beta2;
    A.o1 = (float)(1.0 - a->beta1); A.o2 = (float)(1.0 - a->beta2);
    A.eps = (float)a->eps;
    A.decay = a->weight_decay != 0.0;
    A.lr = a->lr; A.weight_decay = a->weight_decay; A.beta1 = a->beta1; A.beta2 = a->beta2;
    A.state = a->state; A.partials = a->partials;
    A.ctl = c->ctl;
    const hipError_t e = eb::launch_adam_step_ctl(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_adam_step_ctl: launch", e);
    return EB_OK;
}

}  // extern "C"
