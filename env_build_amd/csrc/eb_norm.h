// eb_norm.h — host-visible launch interface of the normalisation kernels (eb_norm.hip), the only translation unit of
// libenvbuild_norm.so.  The contract is stated in include/envbuild_norm.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_norm.h"

namespace eb {

// a batch merged into the running statistics: norm_partial_kernel, then norm_fold_kernel; every pointer is a DEVICE pointer
struct NormUpdateArgs {
    const float* x;                        // [n, D] or NULL
    double* obs_stat;                      // [2 D + 1]
    float* obs_scale;                      // [2 D]
    const float* reward;                   // [n] or NULL
    float* ret_run;                        // [n]
    double* ret_stat;                      // [3]
    float* ret_scale;                      // [2]
    double* work;                          // [blocks][2][D + 1]: S1 and S2 per block and column, the return column last
    int n, D;
    int blocks;                            // of the partial kernel
    int wide;                              // x is 16-byte aligned: the runs are staged as float4s
    float gamma, eps;
};
hipError_t launch_norm_update(const NormUpdateArgs& A, hipStream_t s);

// the normalisation with a state that is only read: norm_apply_kernel
struct NormApplyArgs {
    const float* obs_scale;                // [2 D]
    const float* x;                        // [n, D] or NULL
    float* y;                              // [n, D]; may be x
    float* sel_x;                          // [n, D] or NULL
    const int* sel;                        // [n]
    const float* ret_scale;                // [2]
    const float* reward;                   // [n] or NULL
    float* reward_out;                     // [n]; may be reward
    const unsigned char* done_code;        // [n] or NULL
    float* ret_run;                        // [n] or NULL
    int n, D, sel_value;
    int wide;                              // x and y are both 16-byte aligned
    float clip_obs, clip_rew;
};
hipError_t launch_norm_apply(const NormApplyArgs& A, hipStream_t s);

}  // namespace eb
