// eb_epoch.h — host-visible launch interface of the epoch kernels (eb_epoch.hip), the only translation unit of
// libenvbuild_epoch.so.  The contract is stated in include/envbuild_epoch.h.
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_epoch.h"

namespace eb {

// the minibatch gather; every pointer is a DEVICE pointer
struct GatherSource {
    const float* src;
    float* dst;
    int width;
    int rows_per_pass, rest_per_pass;      // THREADS / width and THREADS % width: how a lane's (row, column) moves from one pass to the next
};
struct GatherArgs {
    GatherSource s[EB_EPOCH_MAX_SOURCES];
    const void* perm;                      // NULL: the keyed route
    const unsigned long long* counter;     // NULL: base 0
    int* index_out;                        // or NULL
    unsigned long long seed, epoch;
    long long offset, count;
    unsigned n_total, mask;                // mask = 2^h - 1
    int h, n_sources, perm_bytes;
};
hipError_t launch_gather(const GatherArgs& A, hipStream_t s);

// mean and 1 / (std + eps)
struct AdvStatsArgs {
    const float* x;
    float* out;                            // [2]
    float* std_out;                        // or NULL
    double* partials;                      // [2 * EB_EPOCH_PARTIALS]
    long long n;
    int chunks, parts;                     // parts = min(chunks, EB_EPOCH_PARTIALS): blocks of launch 1, partials read by launch 2
    float eps;
};
hipError_t launch_adv_stats(const AdvStatsArgs& A, hipStream_t s);   // two launches

// the logging sums of one minibatch
struct PpoLogArgs {
    const float *logp, *logp_old, *ratio, *surr, *ent, *vloss;
    double* out;                           // [EB_EPOCH_LOG_BLOCKS][EB_EPOCH_LOG_FIELDS]
    long long n;
    float clip;
};
hipError_t launch_ppo_log(const PpoLogArgs& A, hipStream_t s);

hipError_t launch_epoch_advance(unsigned long long* counter, unsigned long long by, hipStream_t s);

}  // namespace eb
