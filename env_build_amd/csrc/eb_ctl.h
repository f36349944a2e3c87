// eb_ctl.h — host-visible launch interface of the update-control kernels (eb_ctl.hip), the only translation unit of
// libenvbuild_ctl.so.  The contract is stated in include/envbuild_ctl.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_ctl.h"

namespace eb {

// eb_ctl_begin; every pointer is a DEVICE pointer
struct CtlBeginArgs {
    eb_update_ctl* ctl;
    const float* table;        // [n_table] or NULL
    int n_table;
};
hipError_t launch_ctl_begin(const CtlBeginArgs& A, hipStream_t s);      // one launch

// eb_kl_stop
struct KlStopArgs {
    const float* logp;         // [n]
    const float* logp_old;     // [n]
    double* partials;          // [EB_CTL_KL_BLOCKS]
    double* log;               // [max_slots][2] or NULL
    eb_update_ctl* ctl;
    double limit;
    long long n;
    int max_slots;
};
hipError_t launch_kl_stop(const KlStopArgs& A, hipStream_t s);          // two launches

// eb_adam_step_ctl: eb_train.h's AdamArgs restated field for field (that header is the train library's launch interface, not ours to
// include), the step's lr * weight_decay left to the kernel, and the control block
struct CtlAdamSeg {
    float* p;
    const float* g;
    float* m;
    float* v;
    long long count;
};
struct CtlAdamArgs {
    CtlAdamSeg seg[EB_TRAIN_MAX_SEGMENTS];
    int chunk0[EB_TRAIN_MAX_SEGMENTS + 1];   // the number of the first chunk of segment s; chunk0[n_seg] = chunks
    int n_seg, chunks, parts;                // parts = min(chunks, EB_TRAIN_ADAM_PARTIALS)
    int clip;
    float max_norm;
    float b1, b2, o1, o2, eps;
    int decay;
    double lr, weight_decay, beta1, beta2;
    eb_adam_state* state;
    double* partials;
    const eb_update_ctl* ctl;
};
hipError_t launch_adam_step_ctl(const CtlAdamArgs& A, hipStream_t s);   // two launches

}  // namespace eb
