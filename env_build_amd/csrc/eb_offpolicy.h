// eb_offpolicy.h — host-visible launch interface of the off-policy kernels (eb_offpolicy.hip), the only translation unit of
// libenvbuild_offpolicy.so.  The contract is stated in include/envbuild_offpolicy.h.  The kernels take the checked argument structs of
// that header by value (every pointer in them is a DEVICE pointer; `stream` is not read on the device).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/envbuild_offpolicy.h"

namespace eb {

hipError_t launch_replay_push(const eb_replay_push_args& A, hipStream_t s);        // replay_push_kernel
hipError_t launch_replay_sample(const eb_replay_sample_args& A, hipStream_t s);    // replay_sample_kernel
hipError_t launch_q_pack(const eb_q_pack_args& A, hipStream_t s);                  // q_pack_kernel
hipError_t launch_sac_critic(const eb_sac_critic_args& A, hipStream_t s);          // sac_critic_kernel
hipError_t launch_sac_actor(const eb_sac_actor_args& A, hipStream_t s);            // sac_actor_kernel (+ sac_alpha_fold_kernel)
hipError_t launch_q_action_grad(const eb_q_action_grad_args& A, hipStream_t s);    // q_action_grad_kernel
hipError_t launch_polyak(const eb_polyak_args& A, long long most, hipStream_t s);  // polyak_kernel; most: the largest count

}  // namespace eb
