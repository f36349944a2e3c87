// eb_tape_device.h — what the tape family's translation units (eb_rollout_tape_vjp / _cand / _cand_vjp / _sample / _ilqr.hip) share on
// the device beyond eb_device.h: the unaligned float pair and the closest-point lookup over the handle's path tables.
//
// The lookup reads the tables through whichever argument struct the kernel was launched with (TapeVjpArgs, TapeCandArgs,
// TapeSampleArgs, TapeIlqrArgs name them alike: xy10, phi10, rad_all, cells, gx0, gy0, gnx, gny, red_len), so no struct changes
// its layout for it.  The env's own chain per step (action transform, rewards, bicycle step, tracking, walls) and the five-weight
// cost fold are NOT here: sharing them changes the schedule of the kernels that use them, and each file still restates them.
#pragma once
#include "eb_device.h"

#pragma clang fp contract(off)

namespace eb {

typedef float f2u __attribute__((ext_vector_type(2), aligned(4)));   // 8-byte access, 4-byte aligned: the caller's tape pointer

// closest point of (px, py) on path p: eb_rollout.hip:closest_cell_index<0, false>, restated (DAM:702-715); returns its index
template <class Args>
__device__ __forceinline__ int tape_closest(const Args& A, int p, int roff, float px, float py, float& rx, float& ry, float& rphi) {
    const float* xy = A.xy10 + 2 * roff;
    const float* ph = A.phi10 + roff;
    const float fx = (px - A.gx0) * CELL_INV, fy = (py - A.gy0) * CELL_INV;
    unsigned c = 0xffffffffu;
    if (fx >= 0.0f && fx < (float)A.gnx && fy >= 0.0f && fy < (float)A.gny) c = A.cells[(p * A.gny + (int)fy) * A.gnx + (int)fx];
    if (c == 0xffffffffu) {                                                    // off the corridor's grid: the pruned full search
        const int n = p == 0 ? A.red_len[0] : p == 1 ? A.red_len[1] : A.red_len[2];
        const int bi = closest_reduced_index(reinterpret_cast<const float2*>(xy), A.rad_all + 32 * p, n, px, py, 0, 1 << 30);
        rx = xy[2 * bi]; ry = xy[2 * bi + 1]; rphi = ph[bi];
        return bi;
    }
    return closest_in_range<0>(xy, ph, (int)(c & 0xffffu), (int)(c >> 16), px, py, rx, ry, rphi);
}

}  // namespace eb
