// eb_train.hip — the only translation unit of libenvbuild_train.so (include/envbuild_train.h), gfx950: the value loss of a PPO minibatch
// with its gradient in one launch, and Adam / AdamW with global-norm clipping in two, the step count and the bias-correction powers on
// the device.  Training-only code: libenvbuild_hip.so does not hold it and an inference deployment never loads it.
//
// value_loss_kernel: one lane per row, train::value_loss_row (eb_train_device.h) on the row's three loads; the loads and stores of a wave
// are one coalesced line each at stride 1.
// adam_norm_kernel: block b adds the squares of the chunks b, b + P, ... of the concatenated gradients in double, lane by lane, folds its
// 256 doubles by halving in LDS and writes ONE double partial; one lane of block 0 advances the state.  The order is a pure function of
// the segment counts (the header states it).
// adam_update_kernel: every block folds the P <= 256 partials in the same order — one load per lane, the same LDS halving — so all blocks
// hold the same norm, forms the step's uniforms in double, and updates its chunks with train::adam_element.  Block 0 stores gnorm and
// coef into the state.
// Segments are views into larger tensors and aligned to 4 bytes only, so loads and stores are dwords; a wave's 64 lanes take 64
// consecutive floats.  Plain C++, __syncthreads only, no atomics, plain vector stores.
#include "eb_train.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_train_device.h"

namespace eb {

__global__ __launch_bounds__(train::THREADS) void value_loss_kernel(const ValueLossArgs A) {
    const size_t i = (size_t)blockIdx.x * train::THREADS + threadIdx.x;      // 64 bits: every n up to 2^31 - 1 is accepted
    if (i >= (size_t)A.n) return;
    const size_t at = i * (size_t)A.stride;
    const bool clipped = A.v_old != nullptr;
    float loss, g;
    train::value_loss_row(A.values[at], A.ret[i], clipped ? A.v_old[i] : 0.0f, clipped, A.clip_v, A.scale, loss, g);
    if (A.loss) A.loss[i] = loss;
    if (A.g_values) A.g_values[at] = g;
}

hipError_t launch_value_loss(const ValueLossArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(value_loss_kernel, dim3((unsigned)(((long long)A.n + train::THREADS - 1) / train::THREADS)), dim3(train::THREADS), 0, s, A);
    return hipGetLastError();
}

namespace {

// the segment that holds chunk c (uniform over the block): the one with chunk0[s] <= c < chunk0[s + 1]; empty segments are passed over
__device__ __forceinline__ int segment_of(const AdamArgs& A, int c) {
    int s = 0;
    while (s + 1 < A.n_seg && c >= A.chunk0[s + 1]) ++s;
    return s;
}

}  // namespace

__global__ __launch_bounds__(train::THREADS) void adam_norm_kernel(const AdamArgs A) {
    __shared__ double red[train::THREADS];
    const int t = threadIdx.x;
    double acc = 0.0;
    for (int c = blockIdx.x; c < A.chunks; c += A.parts) {
        const int s = segment_of(A, c);
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
        A.partials[blockIdx.x] = sum;
        if (blockIdx.x == 0) {               // the one lane that reads and advances the state; nothing else in this launch reads it
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

__global__ __launch_bounds__(train::THREADS) void adam_update_kernel(const AdamArgs A) {
    __shared__ double red[train::THREADS];
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
    U.ss = (float)(A.lr / (1.0 - b1t));
    U.sb = (float)sqrt(1.0 - b2t);
    U.b1 = A.b1; U.b2 = A.b2; U.o1 = A.o1; U.o2 = A.o2; U.eps = A.eps; U.lwd = A.lwd; U.decay = A.decay;
    if (blockIdx.x == 0 && t == 0) {
        A.state->gnorm = gnorm;
        A.state->coef = U.coef;
    }
    for (int c = blockIdx.x; c < A.chunks; c += gridDim.x) {
        const int s = segment_of(A, c);
        const AdamSeg S = A.seg[s];
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

hipError_t launch_adam_step(const AdamArgs& A, hipStream_t s) {
    if (A.chunks <= 0) return hipSuccess;
    hipLaunchKernelGGL(adam_norm_kernel, dim3(A.parts), dim3(train::THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const int blocks = A.chunks < 65536 ? A.chunks : 65536;      // beyond that a block walks its chunks with the grid's stride
    hipLaunchKernelGGL(adam_update_kernel, dim3(blocks), dim3(train::THREADS), 0, s, A);
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

static_assert(sizeof(eb_adam_state) == 32, "eb_adam_state is 32 bytes");
static_assert(sizeof(eb::AdamArgs) <= 4096, "kernel arguments");

extern "C" {

int eb_train_abi_version(void) { return EB_TRAIN_ABI_VERSION; }
const char* eb_train_last_error(void) { return g_err; }

int eb_value_loss(const eb_value_loss_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_value_loss: null args");
    if (a->n < 0 || a->stride < 1 || a->scale != a->scale || (a->v_old && !(a->clip_v >= 0.0f)))
        return fail(EB_EINVAL, "eb_value_loss: bad argument (n >= 0, stride >= 1, scale not NaN, clip_v >= 0 and not NaN with v_old)");
    if (a->n > 0 && (!a->values || !a->ret)) return fail(EB_EINVAL, "eb_value_loss: null values or ret");
    if (a->n == 0) return EB_OK;
    const eb::ValueLossArgs A{a->values, a->ret, a->v_old, a->loss, a->g_values, a->clip_v, a->scale, a->n, a->stride};
    const hipError_t e = eb::launch_value_loss(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_value_loss: launch", e);
    return EB_OK;
}

int eb_adam_step(const eb_adam_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_adam_step: null args");
    if (a->n_segments < 0 || a->n_segments > EB_TRAIN_MAX_SEGMENTS)
        return fail(EB_EINVAL, "eb_adam_step: n_segments must be in 0 .. EB_TRAIN_MAX_SEGMENTS (32)");
    if (!(a->lr >= 0.0) || !(a->beta1 >= 0.0 && a->beta1 < 1.0) || !(a->beta2 >= 0.0 && a->beta2 < 1.0) || !(a->eps >= 0.0) ||
        !(a->weight_decay >= 0.0) || a->max_grad_norm != a->max_grad_norm)
        return fail(EB_EINVAL, "eb_adam_step: bad scalar (lr, eps, weight_decay >= 0, beta1 and beta2 in [0, 1), none of them or "
                               "max_grad_norm NaN)");
    eb::AdamArgs A;
    long long chunks = 0;
    for (int s = 0; s < EB_TRAIN_MAX_SEGMENTS; ++s) {
        A.chunk0[s] = (int)chunks;
        if (s >= a->n_segments) {
            A.seg[s] = eb::AdamSeg{nullptr, nullptr, nullptr, nullptr, 0};
            continue;
        }
        const eb_adam_segment& g = a->segments[s];
        if (g.count < 0 || g.count > 2147483647LL) return fail(EB_EINVAL, "eb_adam_step: a segment's count must be in 0 .. 2^31 - 1");
        if (g.count > 0 && (!g.params || !g.grads || !g.m || !g.v || !aligned(g.params, 4) || !aligned(g.grads, 4) || !aligned(g.m, 4) ||
                            !aligned(g.v, 4)))
            return fail(EB_EINVAL, "eb_adam_step: null or not 4-byte aligned params, grads, m or v of a segment with count > 0");
        A.seg[s] = eb::AdamSeg{g.params, g.grads, g.m, g.v, (long long)g.count};
        chunks += (g.count + eb::train::CHUNK - 1) / eb::train::CHUNK;
    }
    A.chunk0[EB_TRAIN_MAX_SEGMENTS] = (int)chunks;
    if (chunks == 0) return EB_OK;
    if (!a->state || !a->partials || !aligned(a->state, 8) || !aligned(a->partials, 8))
        return fail(EB_EINVAL, "eb_adam_step: null or not 8-byte aligned state or partials");
    A.n_seg = a->n_segments;
    A.chunk0[A.n_seg] = (int)chunks;
    A.chunks = (int)chunks;
    A.parts = chunks < EB_TRAIN_ADAM_PARTIALS ? (int)chunks : EB_TRAIN_ADAM_PARTIALS;
    A.clip = a->max_grad_norm > 0.0 && !std::isinf(a->max_grad_norm);
    A.max_norm = (float)a->max_grad_norm;
    A.b1 = (float)a->beta1; A.b2 = (float)a->beta2;
    A.o1 = (float)(1.0 - a->beta1); A.o2 = (float)(1.0 - a->beta2);
    A.eps = (float)a->eps;
    A.lwd = (float)(a->lr * a->weight_decay);
    A.decay = a->weight_decay != 0.0;
    A.lr = a->lr; A.beta1 = a->beta1; A.beta2 = a->beta2;
    A.state = a->state; A.partials = a->partials;
    const hipError_t e = eb::launch_adam_step(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_adam_step: launch", e);
    return EB_OK;
}

}  // extern "C"
