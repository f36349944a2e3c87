// eb_collect.hip — the only translation unit of libenvbuild_collect.so (include/envbuild_collect.h), gfx950: the collection phase of a PPO
// iteration — the rollout buffer's first slot, one slot per env step, the bootstrap values of truncated episodes and the episode
// statistics.  None of the other three libraries holds this code, and it runs no network.
//
// collect_begin_kernel / collect_record_kernel: block k takes the 32 envs from 32 k.  Its first 32 lanes do the per-env scalars, one lane
// per env (record: reward, code, the two flags, the running return and length, the truncation mark), and leave "truncated" per env in
// LDS.  All 256 lanes then copy the block's 32 x D floats of the slot — one contiguous run of the source and of the destination,
// consecutive lanes on consecutive elements — as float4s when the launch's two base addresses are 16-byte aligned (a block's run starts
// 128 D bytes further, so the alignment of the bases is the alignment of every run) and as dwords otherwise; the n % 4 floats of a last,
// partial block go as dwords.  Last, the sparse part: each of the block's four waves walks the envs wave, wave + 4, ... of the block and,
// where LDS says truncated — a wave-uniform branch — its 64 lanes copy the env's final observation, consecutive lanes on consecutive floats
// of the row: the reads are coalesced within the row, and an env that is not truncated costs one LDS read.  Rows start at multiples of D
// floats, so that copy is dwords.  32 envs: 4 096 envs are 128 blocks, 65 536 envs 2 048 (8 blocks of 4 waves per CU), and a 137-float
// observation gives each lane four or five independent 16-byte loads.
// collect_next_values_kernel: a grid-stride select over the T x B elements.
// collect_episode_log_kernel: 64 blocks; lane t of block b walks the slots b * 256 + t + k * 16384 and the block folds its 16 doubles by
// halving, one after the other through one 2 KiB LDS array.
// Plain C++, __syncthreads only, plain vector stores, 256-thread blocks, rows indexed in 64 bits.
#include "eb_collect.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_collect_device.h"

namespace eb {

__global__ __launch_bounds__(collect::THREADS) void collect_begin_kernel(const CollectBeginArgs A) {
    const int t = threadIdx.x;
    const long long env0 = (long long)blockIdx.x * collect::ENVS;
    const int envs = A.n_env - env0 < collect::ENVS ? (int)(A.n_env - env0) : collect::ENVS;
    if (t < envs) A.trunc_t[env0 + t] = -1;
    const long long at = env0 * (long long)A.obs_dim;
    collect::copy_run(A.slot + at, A.obs + at, envs * A.obs_dim, A.wide != 0, t);
}

hipError_t launch_collect_begin(const CollectBeginArgs& A, hipStream_t s) {
    if (A.n_env <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.n_env + collect::ENVS - 1) / collect::ENVS);
    hipLaunchKernelGGL(collect_begin_kernel, dim3(blocks), dim3(collect::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(collect::THREADS) void collect_record_kernel(const CollectRecordArgs A) {
    __shared__ int truncated[collect::ENVS];
    const int t = threadIdx.x;
    const long long env0 = (long long)blockIdx.x * collect::ENVS;
    const int envs = A.n_env - env0 < collect::ENVS ? (int)(A.n_env - env0) : collect::ENVS;
    if (t < collect::ENVS) {
        int trunc = 0;
        if (t < envs) {
            const long long i = env0 + t;
            const unsigned char c = A.done_code[i];
            const float r = A.reward[i];
            const bool live = c == EB_DONE_NOT_YET;
            trunc = (c == EB_DONE_TIME_LIMIT && A.final_obs != nullptr) ? 1 : 0;
            const float R = A.ep_ret[i] + r;
            const int L = A.ep_len[i] + 1;
            A.rew[i] = r;
            A.nonterminal[i] = (live || trunc) ? 1.0f : 0.0f;
            A.carry[i] = live ? 1.0f : 0.0f;
            A.ret[i] = R;
            A.len[i] = L;
            A.code[i] = c;
            A.ep_ret[i] = c != 0 ? 0.0f : R;
            A.ep_len[i] = c != 0 ? 0 : L;
            if (trunc) A.trunc_t[i] = A.t;
        }
        truncated[t] = trunc;
    }
    const long long at = env0 * (long long)A.obs_dim;
    collect::copy_run(A.slot + at, A.obs + at, envs * A.obs_dim, A.wide != 0, t);
    if (A.final_obs == nullptr) return;                         // uniform over the launch
    __syncthreads();
    const int wave = t >> 6, lane = t & 63;
    for (int r = wave; r < envs; r += collect::THREADS / 64) {
        if (truncated[r]) {                                      // uniform over the wave
            const long long row = (env0 + r) * (long long)A.obs_dim;
            for (int c = lane; c < A.obs_dim; c += 64) A.trunc_obs[row + c] = A.final_obs[row + c];
        }
    }
}

hipError_t launch_collect_record(const CollectRecordArgs& A, hipStream_t s) {
    if (A.n_env <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.n_env + collect::ENVS - 1) / collect::ENVS);
    hipLaunchKernelGGL(collect_record_kernel, dim3(blocks), dim3(collect::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(collect::THREADS) void collect_next_values_kernel(const CollectNextValuesArgs A) {
    const long long stride = (long long)gridDim.x * collect::THREADS;
    for (long long e = (long long)blockIdx.x * collect::THREADS + threadIdx.x; e < A.n; e += stride) {
        const int step = (int)e / A.n_env;                       // n <= 2^31 - 1: a 32-bit division
        const int i = (int)e - step * A.n_env;
        const float next = A.values[e + A.n_env];              // values[step + 1, i]
        float v = next;
        if (A.trunc_t[i] == step) v = A.v_trunc[i];              // a select: an unused v_trunc row is not read into the result
        A.next_values[e] = v;
    }
}

hipError_t launch_collect_next_values(const CollectNextValuesArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    long long blocks = (A.n + collect::THREADS - 1) / collect::THREADS;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(collect_next_values_kernel, dim3((unsigned)blocks), dim3(collect::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(collect::THREADS) void collect_episode_log_kernel(const CollectEpisodeLogArgs A) {
    __shared__ double red[collect::THREADS];
    const int t = threadIdx.x;
    const double inf = (double)__int_as_float(0x7F800000);
    double episodes = 0.0, sum = 0.0, squares = 0.0, length = 0.0, top = -inf, low = inf, bad = 0.0, slots = 0.0;
    double codes[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) codes[k] = 0.0;
    for (long long i = (long long)blockIdx.x * collect::THREADS + t; i < A.n; i += (long long)EB_COLLECT_LOG_BLOCKS * collect::THREADS) {
        const unsigned char c = A.code[i];
#pragma unroll
        for (int k = 0; k < 8; ++k) codes[k] = codes[k] + (c == k ? 1.0 : 0.0);
        if (c != 0) {
            const float R = A.ret[i];
            episodes = episodes + 1.0;
            length = length + (double)A.len[i];
            if (R == R) {                                        // a NaN is passed over
                const double d = (double)R;
                sum = sum + d;
                squares = squares + d * d;
                top = d > top ? d : top;
                low = d < low ? d : low;
            }
            if (!collect::finite(R)) bad = bad + 1.0;
        }
        slots = slots + 1.0;
    }
    double out[EB_COLLECT_LOG_FIELDS];
    out[0] = collect::fold<0>(red, t, episodes);
    out[1] = collect::fold<0>(red, t, sum);
    out[2] = collect::fold<0>(red, t, squares);
    out[3] = collect::fold<0>(red, t, length);
    out[4] = collect::fold<1>(red, t, top);
    out[5] = collect::fold<2>(red, t, low);
    out[6] = collect::fold<0>(red, t, bad);
#pragma unroll
    for (int k = 0; k < 8; ++k) out[7 + k] = collect::fold<0>(red, t, codes[k]);
    out[15] = collect::fold<0>(red, t, slots);
    if (t < EB_COLLECT_LOG_FIELDS) {
        double mine = out[0];
#pragma unroll
        for (int k = 1; k < EB_COLLECT_LOG_FIELDS; ++k) mine = t == k ? out[k] : mine;
        A.out[blockIdx.x * EB_COLLECT_LOG_FIELDS + t] = mine;
    }
}

hipError_t launch_collect_episode_log(const CollectEpisodeLogArgs& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(collect_episode_log_kernel, dim3(EB_COLLECT_LOG_BLOCKS), dim3(collect::THREADS), 0, s, A);
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
constexpr long long MOST = 2147483647LL;

}  // namespace

extern "C" {

int eb_collect_abi_version(void) { return EB_COLLECT_ABI_VERSION; }
const char* eb_collect_last_error(void) { return g_err; }

int eb_collect_begin(const eb_collect_begin_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_collect_begin: null args");
    if (a->n_env < 0) return fail(EB_EINVAL, "eb_collect_begin: n_env must be in 0 .. 2^31 - 1");
    if (a->obs_dim < 1) return fail(EB_EINVAL, "eb_collect_begin: obs_dim must be in 1 .. 2^31 - 1");
    if ((long long)a->n_env * a->obs_dim > MOST) return fail(EB_EINVAL, "eb_collect_begin: n_env * obs_dim exceeds 2^31 - 1");
    if (a->n_env == 0) return EB_OK;
    if (!ok4(a->obs) || !ok4(a->obs_buf) || !ok4(a->trunc_t))
        return fail(EB_EINVAL, "eb_collect_begin: null or not 4-byte aligned obs, obs_buf or trunc_t");
    const eb::CollectBeginArgs A{a->obs, a->obs_buf, a->trunc_t, a->n_env, a->obs_dim, aligned(a->obs, 16) && aligned(a->obs_buf, 16) ? 1 : 0};
    const hipError_t e = eb::launch_collect_begin(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_collect_begin: launch", e);
    return EB_OK;
}

int eb_collect_record(const eb_collect_record_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_collect_record: null args");
    if (a->n_env < 0) return fail(EB_EINVAL, "eb_collect_record: n_env must be in 0 .. 2^31 - 1");
    if (a->obs_dim < 1 || a->steps < 1) return fail(EB_EINVAL, "eb_collect_record: obs_dim and steps must be in 1 .. 2^31 - 1");
    if ((long long)a->n_env * a->obs_dim > MOST) return fail(EB_EINVAL, "eb_collect_record: n_env * obs_dim exceeds 2^31 - 1");
    if (a->t < 0 || a->t >= a->steps) return fail(EB_EINVAL, "eb_collect_record: t must be in [0, steps)");
    if (a->n_env == 0) return EB_OK;
    if (!a->done_code || !a->code_buf) return fail(EB_EINVAL, "eb_collect_record: null done_code or code_buf");
    if (!ok4(a->obs) || !ok4(a->reward) || !ok4(a->ep_ret) || !ok4(a->ep_len) || !ok4(a->obs_buf) || !ok4(a->rew_buf) ||
        !ok4(a->nonterminal) || !ok4(a->carry) || !ok4(a->ret_buf) || !ok4(a->len_buf))
        return fail(EB_EINVAL, "eb_collect_record: null or not 4-byte aligned obs, reward, ep_ret, ep_len, obs_buf, rew_buf, nonterminal, "
                               "carry, ret_buf or len_buf");
    if (!aligned(a->final_obs, 4)) return fail(EB_EINVAL, "eb_collect_record: final_obs is not 4-byte aligned");
    if (a->final_obs && (!ok4(a->trunc_obs) || !ok4(a->trunc_t)))
        return fail(EB_EINVAL, "eb_collect_record: with final_obs, null or not 4-byte aligned trunc_obs or trunc_t");
    const size_t run = (size_t)a->n_env * (size_t)a->obs_dim, row = (size_t)a->t * (size_t)a->n_env;
    eb::CollectRecordArgs A;
    A.obs = a->obs;
    A.reward = a->reward;
    A.done_code = a->done_code;
    A.final_obs = a->final_obs;
    A.ep_ret = a->ep_ret;
    A.ep_len = a->ep_len;
    A.slot = a->obs_buf + ((size_t)a->t + 1) * run;
    A.rew = a->rew_buf + row;
    A.nonterminal = a->nonterminal + row;
    A.carry = a->carry + row;
    A.ret = a->ret_buf + row;
    A.len = a->len_buf + row;
    A.code = a->code_buf + row;
    A.trunc_obs = a->trunc_obs;
    A.trunc_t = a->trunc_t;
    A.n_env = a->n_env;
    A.obs_dim = a->obs_dim;
    A.t = a->t;
    A.wide = aligned(A.obs, 16) && aligned(A.slot, 16) ? 1 : 0;
    const hipError_t e = eb::launch_collect_record(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_collect_record: launch", e);
    return EB_OK;
}

int eb_collect_next_values(const eb_collect_next_values_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_collect_next_values: null args");
    if (a->n_env < 0 || a->steps < 0) return fail(EB_EINVAL, "eb_collect_next_values: n_env and steps must be in 0 .. 2^31 - 1");
    if (((long long)a->steps + 1) * a->n_env > MOST) return fail(EB_EINVAL, "eb_collect_next_values: (steps + 1) * n_env exceeds 2^31 - 1");
    if (a->n_env == 0 || a->steps == 0) return EB_OK;
    if (!ok4(a->values) || !ok4(a->v_trunc) || !ok4(a->trunc_t) || !ok4(a->next_values))
        return fail(EB_EINVAL, "eb_collect_next_values: null or not 4-byte aligned values, v_trunc, trunc_t or next_values");
    const eb::CollectNextValuesArgs A{a->values, a->v_trunc, a->trunc_t, a->next_values, a->n_env, (long long)a->steps * a->n_env};
    const hipError_t e = eb::launch_collect_next_values(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_collect_next_values: launch", e);
    return EB_OK;
}

int eb_collect_episode_log(const eb_collect_episode_log_args* a) {
    if (!a) return fail(EB_EINVAL, "eb_collect_episode_log: null args");
    if (a->n_slots < 0 || a->n_slots > MOST) return fail(EB_EINVAL, "eb_collect_episode_log: n_slots must be in 0 .. 2^31 - 1");
    if (a->n_slots == 0) return EB_OK;
    if (!a->code_buf) return fail(EB_EINVAL, "eb_collect_episode_log: null code_buf");
    if (!ok4(a->ret_buf) || !ok4(a->len_buf)) return fail(EB_EINVAL, "eb_collect_episode_log: null or not 4-byte aligned ret_buf or len_buf");
    if (!a->out || !aligned(a->out, 8)) return fail(EB_EINVAL, "eb_collect_episode_log: null or not 8-byte aligned out");
    const eb::CollectEpisodeLogArgs A{a->ret_buf, a->len_buf, a->code_buf, a->out, (long long)a->n_slots};
    const hipError_t e = eb::launch_collect_episode_log(A, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_collect_episode_log: launch", e);
    return EB_OK;
}

}  // extern "C"
