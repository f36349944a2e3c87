// eb_collect.h — host-visible launch interface of the collection kernels (eb_collect.hip), the only translation unit of
// libenvbuild_collect.so.  The contract is stated in include/envbuild_collect.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_collect.h"

namespace eb {

// obs_buf[0] = obs and trunc_t = -1; every pointer is a DEVICE pointer
struct CollectBeginArgs {
    const float* obs;
    float* slot;                           // obs_buf's slot 0
    int* trunc_t;
    int n_env, obs_dim;
    int wide;                              // obs and slot are both 16-byte aligned: the copy moves float4s
};
hipError_t launch_collect_begin(const CollectBeginArgs& A, hipStream_t s);

// slot t of the rollout buffer from one env step's outputs
struct CollectRecordArgs {
    const float* obs;
    const float* reward;
    const unsigned char* done_code;
    const float* final_obs;                // or NULL
    float* ep_ret;
    int* ep_len;
    float* slot;                           // obs_buf + (t + 1) * n_env * obs_dim
    float *rew, *nonterminal, *carry, *ret;   // the [T, B] arrays at row t
    int* len;
    unsigned char* code;
    float* trunc_obs;
    int* trunc_t;
    int n_env, obs_dim, t;
    int wide;
};
hipError_t launch_collect_record(const CollectRecordArgs& A, hipStream_t s);

struct CollectNextValuesArgs {
    const float* values;                   // [T + 1, B]
    const float* v_trunc;
    const int* trunc_t;
    float* next_values;                    // [T, B]
    int n_env;
    long long n;                           // T * B
};
hipError_t launch_collect_next_values(const CollectNextValuesArgs& A, hipStream_t s);

struct CollectEpisodeLogArgs {
    const float* ret;
    const int* len;
    const unsigned char* code;
    double* out;                           // [EB_COLLECT_LOG_BLOCKS][EB_COLLECT_LOG_FIELDS]
    long long n;
};
hipError_t launch_collect_episode_log(const CollectEpisodeLogArgs& A, hipStream_t s);

}  // namespace eb
