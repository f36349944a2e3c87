// eb_per.h — host-visible launch interface of the prioritised-replay kernels (eb_per.hip), the only translation unit of
// libenvbuild_per.so.  The contract is stated in include/envbuild_per.h.  The kernels take the checked argument structs of that header
// by value (every pointer in them is a DEVICE pointer; `stream` is not read on the device).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_per.h"

namespace eb {

hipError_t launch_per_reset(const eb_per_reset_args& A, hipStream_t s);    // per_reset_kernel
hipError_t launch_per_set(const eb_per_set_args& A, hipStream_t s);        // per_set_range_kernel | per_stamp_kernel, per_write_kernel;
                                                                           // per_repair_range_kernel | per_repair_rows_kernel per big
                                                                           // level; per_repair_top_kernel
hipError_t launch_per_sample(const eb_per_sample_args& A, hipStream_t s);  // per_sample_kernel
hipError_t launch_per_weigh(const eb_per_weigh_args& A, hipStream_t s);    // per_weigh_kernel

}  // namespace eb
