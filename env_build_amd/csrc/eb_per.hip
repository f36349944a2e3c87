// eb_per.hip — the only translation unit of libenvbuild_per.so (include/envbuild_per.h), gfx950: prioritised experience replay on the
// device — a radix-32 sum tree of doubles over the replay ring's slots, the stratified draw that descends it, the importance weights and
// the deterministic write-back of priorities.  None of the other eight libraries holds this code; it gathers no rows and runs no network.
//
// per_reset_kernel: a grid-stride sweep; lane i zeroes leaf i and node i and puts stamp i to rest; lane 0 of block 0 stores max_prio.
// per_set_range_kernel: one lane per pushed slot, (start + i) mod C takes *max_prio.
// per_stamp_kernel / per_write_kernel: one lane per row.  The first leaves max(row number) of the valid rows of a leaf in stamp[leaf] (an
// integer atomicMax: the result does not depend on arrival order); the second, behind the kernel boundary, lets exactly that row store
// the clamped value and put the stamp back to rest; every valid row raises *max_prio with an integer atomicMax on its clamped value's bits.
// per_repair_range_kernel / per_repair_rows_kernel: ONE big level per launch, ascending; a lane recomputes one touched node from its 32
// children (node_sum) and stores it — on the range route one lane per node of the one or two contiguous pieces, on the indexed route
// one lane per valid row (rows under the same node store the same bits).
// per_repair_top_kernel: ONE block recomputes the small levels (at most 1024, 32 and 1 nodes) whole, ascending, a barrier between levels.
// per_sample_kernel: 64 blocks, one lane per draw; the small levels are staged in LDS once per block; the descent scans a node's children
// sequentially (scan_children) — a cross-lane scan would add in another order; the block's minimum of the drawn priorities goes to
// min_partials[block].
// per_weigh_kernel: one lane per row.
// Plain C++, __syncthreads only, plain vector stores, 256-thread blocks, slots and rows indexed in 64 bits.
#include "eb_per.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_per_device.h"

namespace eb {

__global__ __launch_bounds__(per::THREADS) void per_reset_kernel(const eb_per_reset_args A, const per::Geometry G) {
    const long long stride = (long long)gridDim.x * per::THREADS;
    for (long long i = (long long)blockIdx.x * per::THREADS + threadIdx.x; i < A.capacity; i += stride) {
        A.prio[i] = 0.0f;
        A.stamp[i] = -1;
        if (i < G.doubles) A.tree[i] = 0.0;                             // doubles <= capacity: n_1 + ... + n_L <= C for every C >= 1
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) A.max_prio[0] = 1.0f;
}

__global__ __launch_bounds__(per::THREADS) void per_set_range_kernel(const eb_per_set_args A) {
    const long long i = (long long)blockIdx.x * per::THREADS + threadIdx.x;
    if (i >= A.n) return;
    const long long slot = ((long long)A.start + i) % A.capacity;
    A.prio[slot] = A.max_prio[0];
}

__global__ __launch_bounds__(per::THREADS) void per_stamp_kernel(const eb_per_set_args A) {
    const long long r = (long long)blockIdx.x * per::THREADS + threadIdx.x;
    if (r >= A.n) return;
    const int j = A.index[r];
    if (per::valid_row(j, A.value[r], A.capacity)) atomicMax(A.stamp + j, (int)r);
}

__global__ __launch_bounds__(per::THREADS) void per_write_kernel(const eb_per_set_args A) {
    const long long r = (long long)blockIdx.x * per::THREADS + threadIdx.x;
    if (r >= A.n) return;
    const int j = A.index[r];
    const float v = A.value[r];
    if (!per::valid_row(j, v, A.capacity)) return;
    const float p = per::clamp_prio(v);
    atomicMax(reinterpret_cast<int*>(A.max_prio), __float_as_int(p));   // every valid row; positive floats: the bits' order is the values' order
    if (A.stamp[j] != (int)r) return;                                   // the one row of this leaf that wins; the others see its number or -1
    A.prio[j] = p;
    A.stamp[j] = -1;
}

// the touched nodes of level k on the range route: those above the slots [a0, a1) and, behind the wrap, [0, b1)
__global__ __launch_bounds__(per::THREADS) void per_repair_range_kernel(const eb_per_set_args A, const per::Geometry G, int k, long long first_a,
                                                                         long long count_a, long long count_b) {
    const long long i = (long long)blockIdx.x * per::THREADS + threadIdx.x;
    if (i >= count_a + count_b) return;
    const long long node = i < count_a ? first_a + i : i - count_a;
    A.tree[G.off[k] + node] = per::node_sum(G, A.prio, A.tree, k, node);
}

__global__ __launch_bounds__(per::THREADS) void per_repair_rows_kernel(const eb_per_set_args A, const per::Geometry G, int k, int shift) {
    const long long r = (long long)blockIdx.x * per::THREADS + threadIdx.x;
    if (r >= A.n) return;
    const int j = A.index[r];
    if (!per::valid_row(j, A.value[r], A.capacity)) return;
    const long long node = (long long)j >> shift;
    A.tree[G.off[k] + node] = per::node_sum(G, A.prio, A.tree, k, node);
}

__global__ __launch_bounds__(per::THREADS) void per_repair_top_kernel(const eb_per_set_args A, const per::Geometry G) {
    for (int k = G.first_small; k <= G.levels; ++k) {
        for (int i = threadIdx.x; i < G.n[k]; i += per::THREADS) A.tree[G.off[k] + i] = per::node_sum(G, A.prio, A.tree, k, i);
        __syncthreads();                                                // the level is there for the one above
    }
}

hipError_t launch_per_reset(const eb_per_reset_args& A, hipStream_t s) {
    const per::Geometry G = per::geometry(A.capacity);
    long long blocks = ((long long)A.capacity + per::THREADS - 1) / per::THREADS;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(per_reset_kernel, dim3((unsigned)blocks), dim3(per::THREADS), 0, s, A, G);
    return hipGetLastError();
}

hipError_t launch_per_set(const eb_per_set_args& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const per::Geometry G = per::geometry(A.capacity);
    const unsigned row_blocks = (unsigned)(((long long)A.n + per::THREADS - 1) / per::THREADS);
    hipError_t e;
    if (A.route == EB_PER_ROUTE_RANGE) {
        hipLaunchKernelGGL(per_set_range_kernel, dim3(row_blocks), dim3(per::THREADS), 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        const long long a0 = A.start, end = (long long)A.start + A.n;
        const long long a1 = end < A.capacity ? end : A.capacity, b1 = end - a1;       // [a0, a1) and [0, b1)
        for (int k = 1; k < G.first_small; ++k) {
            const int shift = 5 * k;
            const long long first_a = a0 >> shift, count_a = ((a1 - 1) >> shift) - first_a + 1;
            long long count_b = b1 > 0 ? ((b1 - 1) >> shift) + 1 : 0;
            if (count_b > first_a) count_b = first_a;                                   // n == C: the pieces' nodes must not overlap
            const unsigned blocks = (unsigned)((count_a + count_b + per::THREADS - 1) / per::THREADS);
            hipLaunchKernelGGL(per_repair_range_kernel, dim3(blocks), dim3(per::THREADS), 0, s, A, G, k, first_a, count_a, count_b);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    } else {
        hipLaunchKernelGGL(per_stamp_kernel, dim3(row_blocks), dim3(per::THREADS), 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        hipLaunchKernelGGL(per_write_kernel, dim3(row_blocks), dim3(per::THREADS), 0, s, A);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        for (int k = 1; k < G.first_small; ++k) {
            hipLaunchKernelGGL(per_repair_rows_kernel, dim3(row_blocks), dim3(per::THREADS), 0, s, A, G, k, 5 * k);
            if ((e = hipGetLastError()) != hipSuccess) return e;
        }
    }
    hipLaunchKernelGGL(per_repair_top_kernel, dim3(1), dim3(per::THREADS), 0, s, A, G);
    return hipGetLastError();
}

__global__ __launch_bounds__(per::THREADS) void per_sample_kernel(const eb_per_sample_args A, const per::Geometry G) {
    __shared__ double top[per::TOP_DOUBLES];
    __shared__ float red[per::THREADS];
    const int t = threadIdx.x;
    const int top_off = G.off[G.first_small];
    for (int i = t; i < G.doubles - top_off; i += per::THREADS) top[i] = A.tree[top_off + i];
    __syncthreads();
    const double total = top[G.doubles - 1 - top_off];                  // the root is the last double
    const uint64_t base = A.counter ? *A.counter : 0;
    const uint64_t key = offp::draw_key(A.seed, A.draw, base);
    const double per_row = total / (double)A.m;
    const float quiet_nan = __int_as_float(0x7FC00000);
    float least = __builtin_inff();
    for (long long r = (long long)blockIdx.x * per::THREADS + t; r < A.m; r += (long long)per::MIN_BLOCKS * per::THREADS) {
        const uint64_t word = offp::draw_word(key, (uint64_t)r);
        const double U = A.u_in ? A.u_in[r] : (double)(word >> 11) * 1.1102230246251565e-16;    // 2^-53
        const double at = (double)r + U;
        double u = at * per_row;
        long long node = total > 0.0 ? 0 : -1;
        for (int k = G.levels; k >= 1 && node >= 0; --k) {
            const long long first = node * per::RADIX;
            const long long rest = (long long)G.n[k - 1] - first;
            const int cnt = rest < per::RADIX ? (int)rest : per::RADIX;
            int c;
            if (k == 1) c = per::scan_children(A.prio + first, cnt, u);
            else if (k - 1 >= G.first_small) c = per::scan_children(top + (G.off[k - 1] - top_off) + first, cnt, u);
            else c = per::scan_children(A.tree + G.off[k - 1] + first, cnt, u);
            node = c >= 0 ? first + c : -1;
        }
        const float p = node >= 0 ? A.prio[node] : quiet_nan;
        A.index_out[r] = (int)node;
        if (A.prio_out) A.prio_out[r] = p;
        if (A.noise_id_out) A.noise_id_out[r] = (uint32_t)word;
        if (node >= 0) least = p < least ? p : least;
    }
    const float block_least = per::fold_min(red, t, least);
    if (A.min_partials && t == 0) A.min_partials[blockIdx.x] = block_least;
}

hipError_t launch_per_sample(const eb_per_sample_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    hipLaunchKernelGGL(per_sample_kernel, dim3(per::MIN_BLOCKS), dim3(per::THREADS), 0, s, A, per::geometry(A.capacity));
    return hipGetLastError();
}

__global__ __launch_bounds__(per::THREADS) void per_weigh_kernel(const eb_per_weigh_args A) {
    const long long r = (long long)blockIdx.x * per::THREADS + threadIdx.x;
    if (r >= A.m) return;
    float beta = A.beta;
    if (A.counter) {
        const float b = __builtin_fmaf(A.beta_step, (float)*A.counter, A.beta);
        beta = b < 1.0f ? b : 1.0f;
    }
    float p_min = __builtin_inff();
    for (int b = 0; b < per::MIN_BLOCKS; ++b) {
        const float x = A.min_partials[b];
        p_min = x < p_min ? x : p_min;
    }
    const bool drawn = A.index[r] >= 0;
    float w = 0.0f;
    if (drawn) {
        const float d = psample::log_det(p_min) - psample::log_det(A.prio[r]);
        const float e = beta * d;
        w = mlp::exp_det(e);
    }
    if (A.w_out) A.w_out[r] = w;
    if (A.g_q1) A.g_q1[r] = A.g_q1[r] * w;
    if (A.g_q2) A.g_q2[r] = A.g_q2[r] * w;
    if (A.loss1) A.loss1[r] = A.loss1[r] * w;
    if (A.loss2) A.loss2[r] = A.loss2[r] * w;
    if (A.prio_new) {
        const float y = A.y[r];
        const float d1 = A.q1[r] - y;
        float a = __builtin_fabsf(d1);
        if (A.q2) {
            const float d2 = A.q2[r] - y;
            const float both = a + __builtin_fabsf(d2);
            a = 0.5f * both;
        }
        const float sum = a + A.eps;
        float pn = sum;
        if (A.alpha != 1.0f) {
            const float l = A.alpha * psample::log_det(sum);
            pn = mlp::exp_det(l);
        }
        A.prio_new[r] = drawn ? pn : __int_as_float(0x7FC00000);
    }
}

hipError_t launch_per_weigh(const eb_per_weigh_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.m + per::THREADS - 1) / per::THREADS);
    hipLaunchKernelGGL(per_weigh_kernel, dim3(blocks), dim3(per::THREADS), 0, s, A);
    return hipGetLastError();
}

}  // namespace eb

// ---- the C-ABI ----
namespace {

thread_local char g_err[512];

int fail2(const char* entry, const char* msg) {
    std::snprintf(g_err, sizeof g_err, "%s: %s", entry, msg);
    return EB_EINVAL;
}
int fail_hip(const char* what, hipError_t e) {
    std::snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return EB_EDEVICE;
}
bool aligned(const void* p, uintptr_t to) { return ((uintptr_t)p & (to - 1)) == 0; }
bool ok4(const void* p) { return p != nullptr && aligned(p, 4); }       // a needed pointer to 4-byte elements
bool ok8(const void* p) { return p != nullptr && aligned(p, 8); }       // ... to 8-byte words

}  // namespace

extern "C" {

int eb_per_abi_version(void) { return EB_PER_ABI_VERSION; }
const char* eb_per_last_error(void) { return g_err; }

int64_t eb_per_tree_doubles(int32_t capacity) {
    if (capacity < 1) return -1;
    return eb::per::geometry(capacity).doubles;
}

int eb_per_set_launches(int32_t capacity, int32_t route) {
    if (capacity < 1 || (route != EB_PER_ROUTE_RANGE && route != EB_PER_ROUTE_INDEXED)) return -1;
    const int big = eb::per::geometry(capacity).first_small - 1;
    return big + (route == EB_PER_ROUTE_RANGE ? 2 : 3);
}

int eb_per_reset(const eb_per_reset_args* a) {
    const char* E = "eb_per_reset";
    if (!a) return fail2(E, "null args");
    if (a->capacity < 1) return fail2(E, "capacity must be in 1 .. 2^31 - 1");
    if (!ok4(a->prio) || !ok4(a->max_prio) || !ok4(a->stamp)) return fail2(E, "null or not 4-byte aligned prio, max_prio or stamp");
    if (!ok8(a->tree)) return fail2(E, "null or not 8-byte aligned tree");
    const hipError_t e = eb::launch_per_reset(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_per_reset: launch", e);
    return EB_OK;
}

int eb_per_set(const eb_per_set_args* a) {
    const char* E = "eb_per_set";
    if (!a) return fail2(E, "null args");
    if (a->capacity < 1) return fail2(E, "capacity must be in 1 .. 2^31 - 1");
    if (a->route != EB_PER_ROUTE_RANGE && a->route != EB_PER_ROUTE_INDEXED) return fail2(E, "route must be EB_PER_ROUTE_RANGE or EB_PER_ROUTE_INDEXED");
    if (a->n < 0) return fail2(E, "n must be in 0 .. 2^31 - 1");
    if (a->route == EB_PER_ROUTE_RANGE) {
        if (a->n > a->capacity) return fail2(E, "on the range route n must be in 0 .. capacity");
        if (a->start < 0 || a->start >= a->capacity) return fail2(E, "on the range route start must be in 0 .. capacity - 1");
    }
    if (a->n == 0) return EB_OK;
    if (!ok4(a->prio) || !ok4(a->max_prio)) return fail2(E, "null or not 4-byte aligned prio or max_prio");
    if (!ok8(a->tree)) return fail2(E, "null or not 8-byte aligned tree");
    if (a->route == EB_PER_ROUTE_INDEXED && (!ok4(a->stamp) || !ok4(a->index) || !ok4(a->value)))
        return fail2(E, "on the indexed route, null or not 4-byte aligned stamp, index or value");
    const hipError_t e = eb::launch_per_set(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_per_set: launch", e);
    return EB_OK;
}

int eb_per_sample(const eb_per_sample_args* a) {
    const char* E = "eb_per_sample";
    if (!a) return fail2(E, "null args");
    if (a->capacity < 1) return fail2(E, "capacity must be in 1 .. 2^31 - 1");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (a->m == 0) return EB_OK;
    if (!ok4(a->prio) || !ok4(a->index_out)) return fail2(E, "null or not 4-byte aligned prio or index_out");
    if (!ok8(a->tree)) return fail2(E, "null or not 8-byte aligned tree");
    if (!aligned(a->counter, 8) || !aligned(a->u_in, 8)) return fail2(E, "counter or u_in is not 8-byte aligned");
    if (!aligned(a->prio_out, 4) || !aligned(a->noise_id_out, 4) || !aligned(a->min_partials, 4))
        return fail2(E, "prio_out, noise_id_out or min_partials is not 4-byte aligned");
    const hipError_t e = eb::launch_per_sample(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_per_sample: launch", e);
    return EB_OK;
}

int eb_per_weigh(const eb_per_weigh_args* a) {
    const char* E = "eb_per_weigh";
    if (!a) return fail2(E, "null args");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (std::isnan(a->beta) || std::isnan(a->beta_step) || std::isnan(a->alpha) || std::isnan(a->eps))
        return fail2(E, "beta, beta_step, alpha or eps is NaN");
    if (a->m == 0) return EB_OK;
    if (!a->g_q1 && !a->g_q2 && !a->loss1 && !a->loss2 && !a->w_out && !a->prio_new) return fail2(E, "no output: nothing to compute");
    if (!ok4(a->index) || !ok4(a->prio) || !ok4(a->min_partials)) return fail2(E, "null or not 4-byte aligned index, prio or min_partials");
    if (!aligned(a->counter, 8)) return fail2(E, "counter is not 8-byte aligned");
    if (!aligned(a->q1, 4) || !aligned(a->q2, 4) || !aligned(a->y, 4) || !aligned(a->g_q1, 4) || !aligned(a->g_q2, 4) || !aligned(a->loss1, 4) ||
        !aligned(a->loss2, 4) || !aligned(a->w_out, 4) || !aligned(a->prio_new, 4))
        return fail2(E, "q1, q2, y or an output is not 4-byte aligned");
    if (a->prio_new && (!a->q1 || !a->y)) return fail2(E, "with prio_new, null q1 or y");
    const hipError_t e = eb::launch_per_weigh(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_per_weigh: launch", e);
    return EB_OK;
}

}  // extern "C"
