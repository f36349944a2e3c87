// eb_offpolicy.hip — the only translation unit of libenvbuild_offpolicy.so (include/envbuild_offpolicy.h), gfx950: the replay ring and
// the memory-bound and elementwise work of a SAC / TD3 / DDPG update between the network launches.  None of the other seven libraries
// holds this code, and it runs no network.
//
// replay_push_kernel: block k takes the rows 32 k .. 32 k + 31.  Their slots (start + i) mod C are one contiguous piece of the ring or
// two (n <= C: the piece crosses slot C - 1 at most once), and each piece of each array is ONE run of source and destination that all
// 256 lanes copy, consecutive lanes on consecutive floats, as float4s when both ends of the piece start 16-byte aligned and as dwords
// otherwise.  The first 32 lanes do the per-row scalars and leave "finished with a final observation" per row in LDS; behind the barrier
// that also orders the dense next_obs copy, each of the four waves walks the rows wave, wave + 4, ... and, where LDS says so — a
// wave-uniform branch — overwrites the row with final_obs.  One lane of block 0 stores fill_after.
// replay_sample_kernel: block k takes 32 destination rows.  Its first 32 lanes form the index once — mulhi64 of a keyed splitmix64 word
// and *fill, or the checked explicit index — and share it through LDS.  Then, output by output, the block's 32 x width destination
// floats are one contiguous run that consecutive lanes write as coalesced dwords; the reads are coalesced inside each source row.  The two
// width-1 outputs go one lane per row, each on another group of 32 lanes.
// q_pack_kernel / q_action_grad_kernel: block k takes 32 rows; consecutive lanes on consecutive floats of the dense side.
// sac_critic_kernel / sac_actor_kernel: one lane per row.  With the temperature gradient the actor kernel runs as 64 blocks striding over
// the rows, each lane summing (double)logp + target_entropy in ascending order; the block folds by halving and writes one partial;
// sac_alpha_fold_kernel, one block, adds the 64 in ascending order.
// polyak_kernel: blockIdx.y is the segment; a block walks chunks of 1024 elements of it, lane t on t, t + 256, t + 512, t + 768.
// Plain C++, __syncthreads only, plain vector stores, 256-thread blocks, rows indexed in 64 bits.
#include "eb_offpolicy.h"

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "eb_offpolicy_device.h"

namespace eb {

__global__ __launch_bounds__(offp::THREADS) void replay_push_kernel(const eb_replay_push_args A) {
    __shared__ int finished[offp::ROWS];
    const int t = threadIdx.x, C = A.capacity, D = A.obs_dim, Na = A.act_dim;
    const long long row0 = (long long)blockIdx.x * offp::ROWS;
    const int rows = A.n - row0 < offp::ROWS ? (int)(A.n - row0) : offp::ROWS;
    const long long slot0 = ((long long)A.start + row0) % C;
    const int len1 = C - slot0 < rows ? (int)(C - slot0) : rows;        // rows before the wrap
    const bool after = A.reward != nullptr;                             // uniform over the launch
    if (A.prev_obs != nullptr) {
        offp::copy_rows_to_ring(A.obs, A.prev_obs + row0 * D, slot0, len1, rows, D, t);
        offp::copy_rows_to_ring(A.act, A.action + row0 * Na, slot0, len1, rows, Na, t);
    }
    if (!after) return;
    if (t < offp::ROWS) {
        int fin = 0;
        if (t < rows) {
            const long long i = row0 + t;
            const long long slot = t < len1 ? slot0 + t : (long long)(t - len1);
            const unsigned char c = A.done_code[i];
            fin = (c != 0 && A.final_obs != nullptr) ? 1 : 0;
            A.rew[slot] = A.reward[i];
            A.nonterminal[slot] = (c == EB_DONE_NOT_YET || (c == EB_DONE_TIME_LIMIT && A.final_obs != nullptr)) ? 1.0f : 0.0f;
        }
        finished[t] = fin;
    }
    if (blockIdx.x == 0 && t == 0) *A.fill = (uint64_t)A.fill_after;
    offp::copy_rows_to_ring(A.next_obs, A.obs_after + row0 * D, slot0, len1, rows, D, t);
    if (A.final_obs == nullptr) return;                                 // uniform over the launch
    __syncthreads();                                                    // finished[] is there, and the dense copy is behind
    const int wave = t >> 6, lane = t & 63;
    for (int r = wave; r < rows; r += offp::THREADS / 64) {
        if (finished[r]) {                                              // uniform over the wave
            const long long slot = r < len1 ? slot0 + r : (long long)(r - len1);
            const float* src = A.final_obs + (row0 + r) * D;
            float* dst = A.next_obs + slot * D;
            for (int c = lane; c < D; c += 64) dst[c] = src[c];
        }
    }
}

hipError_t launch_replay_push(const eb_replay_push_args& A, hipStream_t s) {
    if (A.n <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.n + offp::ROWS - 1) / offp::ROWS);
    hipLaunchKernelGGL(replay_push_kernel, dim3(blocks), dim3(offp::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(offp::THREADS) void replay_sample_kernel(const eb_replay_sample_args A) {
    __shared__ int from_row[offp::ROWS];
    const int t = threadIdx.x, D = A.obs_dim, Na = A.act_dim;
    const long long row0 = (long long)blockIdx.x * offp::ROWS;
    const int rows = A.m - row0 < offp::ROWS ? (int)(A.m - row0) : offp::ROWS;
    if (t < rows) {
        uint64_t f = *A.fill;
        f = f > (uint64_t)A.capacity ? (uint64_t)A.capacity : f;
        const long long r = row0 + t;
        const uint64_t base = A.counter ? *A.counter : 0;
        const uint64_t word = offp::draw_word(offp::draw_key(A.seed, A.draw, base), (uint64_t)r);
        int from = -1;
        if (A.indices) {
            const long long v = A.index_bytes == 8 ? ((const long long*)A.indices)[r] : (long long)((const int*)A.indices)[r];
            from = v >= 0 && v < (long long)f ? (int)v : -1;
        } else if (f > 0) {
            from = (int)__umul64hi(word, f);
        }
        from_row[t] = from;
        if (A.index_out) A.index_out[r] = from;
        if (A.noise_id_out) A.noise_id_out[r] = (uint32_t)word;
    }
    __syncthreads();
    if (A.obs_out) offp::gather_rows<false>(A.obs_out + row0 * D, A.obs, D, nullptr, 0, from_row, rows, t);
    if (A.qin_out) offp::gather_rows<true>(A.qin_out + row0 * (D + Na), A.obs, D, A.act, Na, from_row, rows, t);
    if (A.next_obs_out) offp::gather_rows<false>(A.next_obs_out + row0 * D, A.next_obs, D, nullptr, 0, from_row, rows, t);
    const float quiet_nan = __int_as_float(0x7FC00000);
    if (A.rew_out && t < rows) {                                        // lanes 0 .. 31
        const int from = from_row[t];
        A.rew_out[row0 + t] = from >= 0 ? A.rew[from] : quiet_nan;
    }
    const int u = t - offp::ROWS;                                       // lanes 32 .. 63
    if (A.nonterminal_out && u >= 0 && u < rows) {
        const int from = from_row[u];
        A.nonterminal_out[row0 + u] = from >= 0 ? A.nonterminal[from] : quiet_nan;
    }
}

hipError_t launch_replay_sample(const eb_replay_sample_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.m + offp::ROWS - 1) / offp::ROWS);
    hipLaunchKernelGGL(replay_sample_kernel, dim3(blocks), dim3(offp::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(offp::THREADS) void q_pack_kernel(const eb_q_pack_args A) {
    const int t = threadIdx.x, D = A.obs_dim, Na = A.act_dim, W = D + Na;
    const long long row0 = (long long)blockIdx.x * offp::ROWS;
    const int rows = A.m - row0 < offp::ROWS ? (int)(A.m - row0) : offp::ROWS;
    float* dst = A.qin + row0 * W;
    if (A.obs != nullptr) {                                             // uniform over the launch
        const float* src = A.obs + row0 * D;
        const int total = rows * D, rp = offp::THREADS / D, cp = offp::THREADS - rp * D;
        int r = t / D, c = t - r * D;
        for (int e = t; e < total; e += offp::THREADS) {
            dst[r * W + c] = src[e];
            r += rp;
            c += cp;
            if (c >= D) {
                c -= D;
                ++r;
            }
        }
    }
    if (A.act != nullptr) {
        const float* src = A.act + row0 * Na;
        const int total = rows * Na;                                    // <= 512
        for (int e = t; e < total; e += offp::THREADS) {
            const int r = e / Na, c = e - r * Na;
            dst[r * W + D + c] = src[e];
        }
    }
}

hipError_t launch_q_pack(const eb_q_pack_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.m + offp::ROWS - 1) / offp::ROWS);
    hipLaunchKernelGGL(q_pack_kernel, dim3(blocks), dim3(offp::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(offp::THREADS) void sac_critic_kernel(const eb_sac_critic_args A) {
    const long long i = (long long)blockIdx.x * offp::THREADS + threadIdx.x;
    if (i >= A.m) return;
    const float alpha = offp::alpha_of(A.log_alpha, A.alpha);
    const float qm = offp::min_nan(A.q1t[i], A.q2t[i]);
    const float e = alpha * A.logp_next[i];
    const float v = qm - e;
    const float gn = A.gamma * A.nonterminal[i];
    const float rs = A.reward_scale * A.rew[i];
    const float y = __builtin_fmaf(gn, v, rs);
    if (A.y) A.y[i] = y;
    if (A.loss1 || A.g_q1) {
        const float d = A.q1[i] - y;
        if (A.loss1) A.loss1[i] = (0.5f * d) * d;
        if (A.g_q1) A.g_q1[i] = d * A.inv_m;
    }
    if (A.loss2 || A.g_q2) {
        const float d = A.q2[i] - y;
        if (A.loss2) A.loss2[i] = (0.5f * d) * d;
        if (A.g_q2) A.g_q2[i] = d * A.inv_m;
    }
}

hipError_t launch_sac_critic(const eb_sac_critic_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.m + offp::THREADS - 1) / offp::THREADS);
    hipLaunchKernelGGL(sac_critic_kernel, dim3(blocks), dim3(offp::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(offp::THREADS) void sac_actor_kernel(const eb_sac_actor_args A) {
    __shared__ double red[offp::THREADS];
    const int t = threadIdx.x;
    const long long stride = (long long)gridDim.x * offp::THREADS;
    const float alpha = offp::alpha_of(A.log_alpha, A.alpha);
    const float neg = -A.inv_m;
    const double te = (double)A.target_entropy;
    double sum = 0.0;
    for (long long i = (long long)blockIdx.x * offp::THREADS + t; i < A.m; i += stride) {
        const float q1 = A.q1[i], q2 = A.q2[i], lp = A.logp[i];
        const bool first = q1 <= q2;
        if (A.loss) {
            const float e = alpha * lp;
            A.loss[i] = e - offp::min_nan(q1, q2);
        }
        if (A.g_q1) A.g_q1[i] = first ? neg : 0.0f;
        if (A.g_q2) A.g_q2[i] = first ? 0.0f : neg;
        if (A.g_logp) A.g_logp[i] = alpha * A.inv_m;
        sum = sum + ((double)lp + te);
    }
    if (A.g_log_alpha == nullptr) return;                               // uniform over the launch
    const double total = offp::fold(red, t, sum);
    if (t == 0) A.partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(offp::THREADS) void sac_alpha_fold_kernel(const eb_sac_actor_args A) {
    if (threadIdx.x != 0) return;
    double S = 0.0;
    for (int b = 0; b < offp::ALPHA_BLOCKS; ++b) S = S + A.partials[b];
    A.g_log_alpha[0] = (float)(-(S / (double)A.m));
}

hipError_t launch_sac_actor(const eb_sac_actor_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    if (A.g_log_alpha == nullptr) {
        const unsigned blocks = (unsigned)(((long long)A.m + offp::THREADS - 1) / offp::THREADS);
        hipLaunchKernelGGL(sac_actor_kernel, dim3(blocks), dim3(offp::THREADS), 0, s, A);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(sac_actor_kernel, dim3(offp::ALPHA_BLOCKS), dim3(offp::THREADS), 0, s, A);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(sac_alpha_fold_kernel, dim3(1), dim3(offp::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(offp::THREADS) void q_action_grad_kernel(const eb_q_action_grad_args A) {
    const int t = threadIdx.x, D = A.obs_dim, Na = A.act_dim, W = D + Na;
    const long long row0 = (long long)blockIdx.x * offp::ROWS;
    const int rows = A.m - row0 < offp::ROWS ? (int)(A.m - row0) : offp::ROWS;
    const float* in1 = A.g_in1 + row0 * W;
    float* dst = A.g_a + row0 * Na;
    const int total = rows * Na;                                        // <= 512
    for (int e = t; e < total; e += offp::THREADS) {
        const int r = e / Na, c = e - r * Na;
        float g = in1[r * W + D + c];
        if (A.g_in2 != nullptr) g = g + (A.g_in2 + row0 * W)[r * W + D + c];
        dst[e] = g;
    }
}

hipError_t launch_q_action_grad(const eb_q_action_grad_args& A, hipStream_t s) {
    if (A.m <= 0) return hipSuccess;
    const unsigned blocks = (unsigned)(((long long)A.m + offp::ROWS - 1) / offp::ROWS);
    hipLaunchKernelGGL(q_action_grad_kernel, dim3(blocks), dim3(offp::THREADS), 0, s, A);
    return hipGetLastError();
}

__global__ __launch_bounds__(offp::THREADS) void polyak_kernel(const eb_polyak_args A) {
    const eb_polyak_segment S = A.segments[blockIdx.y];
    const long long stride = (long long)gridDim.x * offp::POLYAK_CHUNK;
    for (long long c0 = (long long)blockIdx.x * offp::POLYAK_CHUNK; c0 < S.count; c0 += stride) {
#pragma unroll
        for (int j = 0; j < offp::POLYAK_CHUNK / offp::THREADS; ++j) {
            const long long e = c0 + threadIdx.x + j * offp::THREADS;
            if (e < S.count) {
                const float tv = S.target[e];
                const float d = S.online[e] - tv;
                S.target[e] = __builtin_fmaf(A.tau, d, tv);
            }
        }
    }
}

hipError_t launch_polyak(const eb_polyak_args& A, long long most, hipStream_t s) {
    if (A.n_segments <= 0 || most <= 0) return hipSuccess;
    long long chunks = (most + offp::POLYAK_CHUNK - 1) / offp::POLYAK_CHUNK;
    if (chunks > 1024) chunks = 1024;
    hipLaunchKernelGGL(polyak_kernel, dim3((unsigned)chunks, (unsigned)A.n_segments), dim3(offp::THREADS), 0, s, A);
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
bool ok8(const void* p) { return p != nullptr && aligned(p, 8); }       // ... to 8-byte words
constexpr long long MOST = 2147483647LL;

// the sizes every row entry shares; NULL: fine
const char* bad_dims(int32_t obs_dim, int32_t act_dim, long long rows) {
    if (obs_dim < 1 || obs_dim > EB_OFFPOLICY_MAX_OBS) return "obs_dim must be in 1 .. 4096";
    if (act_dim < 1 || act_dim > EB_OFFPOLICY_MAX_ACT) return "act_dim must be in 1 .. 16";
    if (rows * ((long long)obs_dim + act_dim) > MOST) return "rows * (obs_dim + act_dim) exceeds 2^31 - 1";
    return nullptr;
}
int fail2(const char* entry, const char* msg) {
    std::snprintf(g_err, sizeof g_err, "%s: %s", entry, msg);
    return EB_EINVAL;
}

}  // namespace

extern "C" {

int eb_offpolicy_abi_version(void) { return EB_OFFPOLICY_ABI_VERSION; }
const char* eb_offpolicy_last_error(void) { return g_err; }

int eb_replay_push(const eb_replay_push_args* a) {
    const char* E = "eb_replay_push";
    if (!a) return fail2(E, "null args");
    if (a->capacity < 1) return fail2(E, "capacity must be in 1 .. 2^31 - 1");
    if (a->n < 0 || a->n > a->capacity) return fail2(E, "n must be in 0 .. capacity");
    if (a->start < 0 || a->start >= a->capacity) return fail2(E, "start must be in 0 .. capacity - 1");
    if (const char* m = bad_dims(a->obs_dim, a->act_dim, a->capacity)) return fail2(E, m);
    if (a->n == 0) return EB_OK;
    if (!a->prev_obs && !a->reward) return fail2(E, "neither prev_obs nor reward: nothing to push");
    if ((a->prev_obs != nullptr) != (a->action != nullptr)) return fail2(E, "prev_obs and action go together or not at all");
    if (a->prev_obs && (!ok4(a->obs) || !ok4(a->act) || !aligned(a->prev_obs, 4) || !aligned(a->action, 4)))
        return fail2(E, "with prev_obs, null or not 4-byte aligned obs, act, prev_obs or action");
    if ((a->reward != nullptr) != (a->obs_after != nullptr) || (a->reward != nullptr) != (a->done_code != nullptr))
        return fail2(E, "reward, obs_after and done_code go together or not at all");
    if (a->final_obs && !a->reward) return fail2(E, "final_obs belongs to the after part");
    if (a->reward) {
        if (a->fill_after < 0 || a->fill_after > a->capacity) return fail2(E, "fill_after must be in 0 .. capacity");
        if (!ok4(a->rew) || !ok4(a->next_obs) || !ok4(a->nonterminal) || !aligned(a->reward, 4) || !aligned(a->obs_after, 4) ||
            !aligned(a->final_obs, 4))
            return fail2(E, "with reward, null or not 4-byte aligned rew, next_obs, nonterminal, reward, obs_after or final_obs");
        if (!ok8(a->fill)) return fail2(E, "with reward, null or not 8-byte aligned fill");
    }
    const hipError_t e = eb::launch_replay_push(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_replay_push: launch", e);
    return EB_OK;
}

int eb_replay_sample(const eb_replay_sample_args* a) {
    const char* E = "eb_replay_sample";
    if (!a) return fail2(E, "null args");
    if (a->capacity < 1) return fail2(E, "capacity must be in 1 .. 2^31 - 1");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (const char* m = bad_dims(a->obs_dim, a->act_dim, a->capacity)) return fail2(E, m);
    if (const char* m = bad_dims(a->obs_dim, a->act_dim, a->m)) return fail2(E, m);
    if (a->m == 0) return EB_OK;
    if (!a->obs_out && !a->qin_out && !a->next_obs_out && !a->rew_out && !a->nonterminal_out && !a->index_out && !a->noise_id_out)
        return fail2(E, "no output: nothing to sample");
    if (!ok8(a->fill)) return fail2(E, "null or not 8-byte aligned fill");
    if (!aligned(a->counter, 8)) return fail2(E, "counter is not 8-byte aligned");
    if (a->indices && ((a->index_bytes != 4 && a->index_bytes != 8) || !aligned(a->indices, (uintptr_t)a->index_bytes)))
        return fail2(E, "with indices, index_bytes must be 4 or 8 and indices aligned to it");
    if (!aligned(a->obs_out, 4) || !aligned(a->qin_out, 4) || !aligned(a->next_obs_out, 4) || !aligned(a->rew_out, 4) ||
        !aligned(a->nonterminal_out, 4) || !aligned(a->index_out, 4) || !aligned(a->noise_id_out, 4))
        return fail2(E, "an output is not 4-byte aligned");
    if ((a->obs_out || a->qin_out) && !ok4(a->obs)) return fail2(E, "with obs_out or qin_out, null or not 4-byte aligned obs");
    if (a->qin_out && !ok4(a->act)) return fail2(E, "with qin_out, null or not 4-byte aligned act");
    if (a->next_obs_out && !ok4(a->next_obs)) return fail2(E, "with next_obs_out, null or not 4-byte aligned next_obs");
    if (a->rew_out && !ok4(a->rew)) return fail2(E, "with rew_out, null or not 4-byte aligned rew");
    if (a->nonterminal_out && !ok4(a->nonterminal)) return fail2(E, "with nonterminal_out, null or not 4-byte aligned nonterminal");
    const hipError_t e = eb::launch_replay_sample(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_replay_sample: launch", e);
    return EB_OK;
}

int eb_q_pack(const eb_q_pack_args* a) {
    const char* E = "eb_q_pack";
    if (!a) return fail2(E, "null args");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (const char* m = bad_dims(a->obs_dim, a->act_dim, a->m)) return fail2(E, m);
    if (a->m == 0) return EB_OK;
    if (!a->obs && !a->act) return fail2(E, "neither obs nor act: nothing to pack");
    if (!ok4(a->qin)) return fail2(E, "null or not 4-byte aligned qin");
    if (!aligned(a->obs, 4) || !aligned(a->act, 4)) return fail2(E, "obs or act is not 4-byte aligned");
    const hipError_t e = eb::launch_q_pack(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_q_pack: launch", e);
    return EB_OK;
}

int eb_sac_critic(const eb_sac_critic_args* a) {
    const char* E = "eb_sac_critic";
    if (!a) return fail2(E, "null args");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (std::isnan(a->gamma) || std::isnan(a->reward_scale) || std::isnan(a->inv_m)) return fail2(E, "gamma, reward_scale or inv_m is NaN");
    if (!a->log_alpha && std::isnan(a->alpha)) return fail2(E, "alpha is NaN and no log_alpha is given");
    if (a->m == 0) return EB_OK;
    if (!a->y && !a->loss1 && !a->loss2 && !a->g_q1 && !a->g_q2) return fail2(E, "no output: nothing to compute");
    if (!ok4(a->q1t) || !ok4(a->q2t) || !ok4(a->logp_next) || !ok4(a->rew) || !ok4(a->nonterminal))
        return fail2(E, "null or not 4-byte aligned q1t, q2t, logp_next, rew or nonterminal");
    if (!aligned(a->log_alpha, 4) || !aligned(a->y, 4) || !aligned(a->loss1, 4) || !aligned(a->loss2, 4) || !aligned(a->g_q1, 4) ||
        !aligned(a->g_q2, 4))
        return fail2(E, "log_alpha or an output is not 4-byte aligned");
    if ((a->loss1 || a->g_q1) && !ok4(a->q1)) return fail2(E, "with loss1 or g_q1, null or not 4-byte aligned q1");
    if ((a->loss2 || a->g_q2) && !ok4(a->q2)) return fail2(E, "with loss2 or g_q2, null or not 4-byte aligned q2");
    const hipError_t e = eb::launch_sac_critic(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_sac_critic: launch", e);
    return EB_OK;
}

int eb_sac_actor(const eb_sac_actor_args* a) {
    const char* E = "eb_sac_actor";
    if (!a) return fail2(E, "null args");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (std::isnan(a->inv_m)) return fail2(E, "inv_m is NaN");
    if (!a->log_alpha && std::isnan(a->alpha)) return fail2(E, "alpha is NaN and no log_alpha is given");
    if (a->g_log_alpha && std::isnan(a->target_entropy)) return fail2(E, "target_entropy is NaN");
    if (a->m == 0) return EB_OK;
    if (!a->loss && !a->g_q1 && !a->g_q2 && !a->g_logp && !a->g_log_alpha) return fail2(E, "no output: nothing to compute");
    if (!ok4(a->q1) || !ok4(a->q2) || !ok4(a->logp)) return fail2(E, "null or not 4-byte aligned q1, q2 or logp");
    if (!aligned(a->log_alpha, 4) || !aligned(a->loss, 4) || !aligned(a->g_q1, 4) || !aligned(a->g_q2, 4) || !aligned(a->g_logp, 4) ||
        !aligned(a->g_log_alpha, 4))
        return fail2(E, "log_alpha or an output is not 4-byte aligned");
    if (a->g_log_alpha && !ok8(a->partials)) return fail2(E, "with g_log_alpha, null or not 8-byte aligned partials");
    const hipError_t e = eb::launch_sac_actor(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_sac_actor: launch", e);
    return EB_OK;
}

int eb_q_action_grad(const eb_q_action_grad_args* a) {
    const char* E = "eb_q_action_grad";
    if (!a) return fail2(E, "null args");
    if (a->m < 0) return fail2(E, "m must be in 0 .. 2^31 - 1");
    if (const char* m = bad_dims(a->obs_dim, a->act_dim, a->m)) return fail2(E, m);
    if (a->m == 0) return EB_OK;
    if (!ok4(a->g_in1) || !ok4(a->g_a)) return fail2(E, "null or not 4-byte aligned g_in1 or g_a");
    if (!aligned(a->g_in2, 4)) return fail2(E, "g_in2 is not 4-byte aligned");
    const hipError_t e = eb::launch_q_action_grad(*a, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_q_action_grad: launch", e);
    return EB_OK;
}

int eb_polyak(const eb_polyak_args* a) {
    const char* E = "eb_polyak";
    if (!a) return fail2(E, "null args");
    if (a->n_segments < 0 || a->n_segments > EB_OFFPOLICY_MAX_SEGMENTS) return fail2(E, "n_segments must be in 0 .. 32");
    if (std::isnan(a->tau)) return fail2(E, "tau is NaN");
    long long total = 0, most = 0;
    for (int k = 0; k < a->n_segments; ++k) {
        const eb_polyak_segment& S = a->segments[k];
        if (S.count < 0 || S.count > MOST) return fail2(E, "a segment's count must be in 0 .. 2^31 - 1");
        total += S.count;
        if (total > MOST) return fail2(E, "the segments' total exceeds 2^31 - 1");
        if (S.count == 0) continue;
        if (!ok4(S.target) || !ok4(S.online)) return fail2(E, "a segment's target or online is null or not 4-byte aligned");
        if (S.target == S.online) return fail2(E, "a segment's target is its online");
        most = S.count > most ? S.count : most;
    }
    const hipError_t e = eb::launch_polyak(*a, most, (hipStream_t)a->stream);
    if (e != hipSuccess) return fail_hip("eb_polyak: launch", e);
    return EB_OK;
}

}  // extern "C"
