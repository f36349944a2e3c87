// eb_train.h — host-visible launch interface of the training kernels (eb_train.hip), the only translation unit of
// libenvbuild_train.so.  The arithmetic contract is stated in include/envbuild_train.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_train.h"

namespace eb {

// the value loss, one lane per row; every pointer is a DEVICE pointer
struct ValueLossArgs {
    const float* values;       // [n] at stride
    const float* ret;          // [n]
    const float* v_old;        // [n] or NULL
    float* loss;               // [n] or NULL
    float* g_values;           // [n] at stride, or NULL
    float clip_v, scale;
    int n, stride;
};
hipError_t launch_value_loss(const ValueLossArgs& A, hipStream_t s);

// one Adam step over the chunks of up to EB_TRAIN_MAX_SEGMENTS segments
struct AdamSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long count;
};
struct AdamArgs {
    AdamSeg seg[EB_TRAIN_MAX_SEGMENTS];
    int chunk0[EB_TRAIN_MAX_SEGMENTS + 1];   // the number of the first chunk of segment s; chunk0[n_seg] = chunks
    int n_seg, chunks, parts;                // parts = min(chunks, EB_TRAIN_ADAM_PARTIALS): blocks of launch 1, partials read by launch 2
    int clip;                                // clipping on
    float max_norm;                          // (float)max_grad_norm
    float b1, b2, o1, o2, eps, lwd;
    int decay;
    double lr, beta1, beta2;
    eb_adam_state* state;
    double* partials;
};
hipError_t launch_adam_step(const AdamArgs& A, hipStream_t s);   // two launches

}  // namespace eb
