// eb_ctl_device.h — what the kernels of eb_ctl.hip share.  The arithmetic of an Adam element, its uniforms, the block fold, THREADS and
// CHUNK are eb_train_device.h's and are used from there, not restated; the chunk walk's segment lookup lives in eb_train.hip (moving it
// would touch that unit), so its few lines are restated here.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_ctl.h"
#include "eb_train_device.h"

namespace eb {
namespace ctl {

constexpr int THREADS = train::THREADS;    // of all five kernels
constexpr int KL_BLOCKS = EB_CTL_KL_BLOCKS;

// the segment that holds chunk c (uniform over the block): the one with chunk0[s] <= c < chunk0[s + 1]; empty segments are passed over
__device__ __forceinline__ int segment_of(const CtlAdamArgs& A, int c) {
    int s = 0;
    while (s + 1 < A.n_seg && c >= A.chunk0[s + 1]) ++s;
    return s;
}

// one row of the approximate KL: the subtraction in fp32, the sum in double
__device__ __forceinline__ double kl_row(float logp_old, float logp) { return (double)(logp_old - logp); }

}  // namespace ctl
}  // namespace eb
