// eb_cand_grad.h — host-visible launch interface of the candidate-tape value-and-gradient kernel (eb_rollout_tape_cand_vjp.hip), next to
// eb_cand.h and eb_grad.h.
#pragma once
#include <hip/hip_runtime.h>

#include "eb_cand.h"

namespace eb {

// value and gradient of n_cand open-loop tapes per env in one launch; see include/envbuild_cand_grad.h:eb_rollout_tape_cand_vjp
struct TapeCandVjpArgs {
    TapeCandArgs F;            // the forward's arguments, as eb_rollout_tape_cand takes them (w5 is also the cotangent of every out5 row)
    float* g_obs0;             // [n_cand, n_env, nd] or NULL
    float* g_tapes;            // [n_cand, horizon, n_env, 2]
};
// the most candidates a launch takes for this slot count and horizon (queue and LDS tape of every (env, candidate) must fit); may be 0
int rollout_tape_cand_vjp_max(int n_veh, int horizon);
// n_cu: compute units of the device (the tile is chosen so that a grid fills them)
hipError_t launch_rollout_tape_cand_vjp(int task, const TapeCandVjpArgs& A, int n_cu, hipStream_t s);

}  // namespace eb
