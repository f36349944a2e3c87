// eb_ac.hip — the only translation unit of libenvbuild_ac.so (include/envbuild_ac.h), gfx950: the two row kernels of a shared-trunk
// actor-critic, whose network writes y [n, W = 2 * act_dim + 1] — the policy's logits in columns 0 .. 2A-1 and the value in column 2A.
// None of the other five libraries holds this code.
//
// ac_loss_kernel: one lane per row.  The lane copies its row's 2A logits to an LDS row of its own (stride 33 floats: lane r reads
// r * 33 + a, every bank once) — ppo_surrogate_logits_kernel's staging, because plogp::logp_row is handed the row as its z_out — and
// runs the PPO row on it, then train::value_loss_row on column 2A, and writes the whole cotangent row g_y[e, 0 .. W-1].
// ac_sample_kernel: one lane per row; psample::sample_row reads the row's logits from global memory as policy_sample_logits_kernel
// does, and the lane copies the 2A logits to the dense logits_out and column 2A to values.
//
// WHAT IS RESTATED.  The arithmetic is called, not written: plogp::logp_row, plogp::logp_vjp_elem (eb_policy_logp_device.h),
// mlp::exp_det (eb_mlp_device.h), psample::sample_row (eb_policy_sample_device.h) and train::value_loss_row (eb_train_device.h).
// ppo::surrogate_row (eb_ppo_device.h) cannot be called: it hard-codes g_logits' row stride as 2 * act_dim.  Only its lines between
// the call of logp_row and the calls of logp_vjp_elem — the advantage's normalisation, the ratio, the clamp, the minimum, `blocked`
// and g_lp — and its loop's stores are therefore restated below, with the stride W; the expressions are its own, operation for
// operation, so the bits are eb_ppo_surrogate_from_logits'.  The key of the noise and the row id are policy_sample_logits_kernel's
// two lines.
// Plain C++, no __syncthreads, no atomics, plain vector stores, rows indexed in 64 bits.  Rows of y and g_y are aligned to 4 bytes
// only (W is odd): every load and store is a dword.
#include "eb_ac.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_policy_logp_device.h"
#include "eb_train_device.h"

#pragma clang fp contract(off)

namespace eb {
namespace {

constexpr int AC_LS = 33;             // row stride of the logits in LDS (eb_policy_head_device.h's)
constexpr int AC_LOSS_THREADS = 128;  // 128 LDS rows of AC_LS floats
constexpr int AC_SAMPLE_THREADS = 256;

}  // namespace

__global__ __launch_bounds__(AC_LOSS_THREADS) void ac_loss_kernel(const AcLossArgs S) {
    __shared__ float rows[AC_LOSS_THREADS * AC_LS];
    const size_t e = (size_t)blockIdx.x * AC_LOSS_THREADS + threadIdx.x;
    if (e >= (size_t)S.n) return;
    const int act_dim = S.act_dim, W = 2 * act_dim + 1;
    float* y = rows + threadIdx.x * AC_LS;
    const float* src = S.y + e * (size_t)W;
    for (int c = 0; c < 2 * act_dim; ++c) y[c] = src[c];
    const float value = src[2 * act_dim];

    // ---- the policy columns: ppo::surrogate_row with g's stride W ----
    float logp;
    plogp::logp_row(y, act_dim, S.actions + e * act_dim, S.action_range, S.log_ar, &logp, y);   // y[a] becomes z[a]
    float A = S.adv[e];
    if (S.adv_norm) A = (A - S.adv_norm[0]) * S.adv_norm[1];
    const float d = logp - S.logp_old[e];
    const float r = mlp::exp_det(d);
    const float s1 = r * A;
    const float rc = r < S.lo ? S.lo : (r > S.hi ? S.hi : r);            // a NaN falls through both compares
    const float s2 = rc * A;
    const float surr = s2 < s1 ? s2 : s1;
    const bool blocked = (r < S.lo || r > S.hi) && (s2 <= s1);           // a NaN in r or A: not blocked
    const float g_lp = blocked ? 0.0f : (S.w * A) * r;
    S.logp[e] = logp;
    if (S.ratio) S.ratio[e] = r;
    if (S.surr) S.surr[e] = surr;
    float sum = 0.0f;
    float* g = S.g_y ? S.g_y + e * (size_t)W : nullptr;
    for (int a = 0; a < act_dim; ++a) {
        const float z = y[a], ls = y[act_dim + a];
        sum = sum + ls;
        if (S.z_out) S.z_out[e * act_dim + a] = z;
        if (g) {
            float g_mean, g_ls;
            plogp::logp_vjp_elem(ls, z, g_lp, g_mean, g_ls);
            g[a] = g_mean;
            g[act_dim + a] = g_ls + S.g_ent;
        }
    }
    if (S.ent) S.ent[e] = sum + (float)act_dim * 1.4189385332f;

    // ---- the value column: value_loss_kernel's row ----
    const bool clipped = S.v_old != nullptr;
    float loss, gv;
    train::value_loss_row(value, S.ret[e], clipped ? S.v_old[e] : 0.0f, clipped, S.clip_v, S.v_scale, loss, gv);
    if (S.vloss) S.vloss[e] = loss;
    if (g) g[2 * act_dim] = gv;
}

hipError_t launch_ac_loss(const AcLossArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ac_loss_kernel, dim3((A.n + AC_LOSS_THREADS - 1) / AC_LOSS_THREADS), dim3(AC_LOSS_THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(AC_SAMPLE_THREADS) void ac_sample_kernel(const AcSampleArgs S) {
    const size_t e = (size_t)blockIdx.x * AC_SAMPLE_THREADS + threadIdx.x;
    if (e >= (size_t)S.n) return;
    const int act_dim = S.act_dim, W = 2 * act_dim + 1;
    const float* y = S.y + e * (size_t)W;
    if (S.actions) {
        const uint64_t key = splitmix64(S.seed + 0x9E3779B97F4A7C15ull * S.counter);
        const uint64_t id = (uint64_t)(uint32_t)(S.row_ids ? S.row_ids[e] : (int32_t)e);
        psample::sample_row(y, act_dim, S.eps ? S.eps + e * act_dim : nullptr, key, id, S.action_range, S.log_ar, S.actions + e * act_dim,
                            S.logp ? S.logp + e : nullptr, S.eps_out ? S.eps_out + e * act_dim : nullptr);
    }
    if (S.logits_out) {
        float* dst = S.logits_out + e * (size_t)(2 * act_dim);
        for (int c = 0; c < 2 * act_dim; ++c) dst[c] = y[c];
    }
    if (S.values) S.values[e] = y[2 * act_dim];
}

hipError_t launch_ac_sample(const AcSampleArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(ac_sample_kernel, dim3((A.n + AC_SAMPLE_THREADS - 1) / AC_SAMPLE_THREADS), dim3(AC_SAMPLE_THREADS), 0, s, A);
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
bool aligned4(const void* p) { return ((uintptr_t)p & 3u) == 0; }

}  // namespace

static_assert(2 * EB_AC_MAX_ACT_DIM + 1 <= 32, "eb_mlp_backward's cotangent row is 32 floats wide");
static_assert(2 * EB_AC_MAX_ACT_DIM <= 33, "a row of logits fits its LDS row");

extern "C" {

int eb_ac_abi_version(void) { return EB_AC_ABI_VERSION; }
const char* eb_ac_last_error(void) { return g_err; }

int eb_ac_loss(const eb_ac_loss_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_ac_loss: null args");
    if (a->n < 0 || a->act_dim < 1 || a->act_dim > EB_AC_MAX_ACT_DIM)
        return fail(EB_EINVAL, "eb_ac_loss: bad argument (n >= 0, act_dim in 1 .. 15)");
    if (a->action_range != a->action_range || !(a->clip >= 0.0f) || a->ent_coef != a->ent_coef || a->scale != a->scale ||
        a->v_scale != a->v_scale || (a->v_old && !(a->clip_v >= 0.0f)))
        return fail(EB_EINVAL, "eb_ac_loss: bad scalar (clip >= 0, clip_v >= 0 with v_old, action_range, clip, ent_coef, scale and v_scale "
                               "not NaN)");
    const void* ptrs[] = {a->y, a->actions, a->logp_old, a->adv, a->adv_norm, a->ret, a->v_old, a->logp, a->ratio, a->surr, a->ent,
                          a->vloss, a->g_y, a->z_out};
    for (const void* p : ptrs)
        if (!aligned4(p)) return fail(EB_EINVAL, "eb_ac_loss: a pointer is not 4-byte aligned");
    if (a->n == 0) return EB_OK;
    if (!a->y || !a->actions || !a->logp_old || !a->adv || !a->ret || !a->logp)
        return fail(EB_EINVAL, "eb_ac_loss: null y, actions, logp_old, adv, ret or logp");
    eb::AcLossArgs A;
    A.y = a->y; A.actions = a->actions; A.logp_old = a->logp_old; A.adv = a->adv; A.adv_norm = a->adv_norm; A.ret = a->ret;
    A.v_old = a->v_old;
    A.action_range = a->action_range;
    A.log_ar = a->action_range > 0.0f ? (float)std::log((double)a->action_range) : 0.0f;
    A.lo = 1.0f - a->clip; A.hi = 1.0f + a->clip;
    A.w = -a->scale;
    A.g_ent = -(a->scale * a->ent_coef);
    A.clip_v = a->v_old ? a->clip_v : 0.0f;
    A.v_scale = a->v_scale;
    A.logp = a->logp; A.ratio = a->ratio; A.surr = a->surr; A.ent = a->ent; A.vloss = a->vloss; A.g_y = a->g_y; A.z_out = a->z_out;
    A.n = a->n; A.act_dim = a->act_dim;
    const hipError_t e = eb::launch_ac_loss(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_ac_loss: launch", e);
    return EB_OK;
}

int eb_ac_sample(const eb_ac_sample_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_ac_sample: null args");
    if (a->n < 0 || a->act_dim < 1 || a->act_dim > EB_AC_MAX_ACT_DIM || a->action_range != a->action_range)
        return fail(EB_EINVAL, "eb_ac_sample: bad argument (n >= 0, act_dim in 1 .. 15, action_range not NaN)");
    const void* ptrs[] = {a->y, a->eps, a->row_ids, a->actions, a->logits_out, a->values, a->logp, a->eps_out};
    for (const void* p : ptrs)
        if (!aligned4(p)) return fail(EB_EINVAL, "eb_ac_sample: a pointer is not 4-byte aligned");
    if (a->n == 0) return EB_OK;
    if (!a->y) return fail(EB_EINVAL, "eb_ac_sample: null y");
    if (!a->actions && !a->logits_out && !a->values) return fail(EB_EINVAL, "eb_ac_sample: null actions, logits_out and values: nothing to write");
    eb::AcSampleArgs A;
    A.y = a->y; A.eps = a->eps; A.row_ids = a->row_ids; A.seed = a->seed; A.counter = a->counter;
    A.action_range = a->action_range;
    A.log_ar = a->action_range > 0.0f ? (float)std::log((double)a->action_range) : 0.0f;
    A.actions = a->actions; A.logits_out = a->logits_out; A.values = a->values; A.logp = a->logp; A.eps_out = a->eps_out;
    A.n = a->n; A.act_dim = a->act_dim;
    const hipError_t e = eb::launch_ac_sample(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_ac_sample: launch", e);
    return EB_OK;
}

}  // extern "C"
