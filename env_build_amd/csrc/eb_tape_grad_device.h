// eb_tape_grad_device.h — the per-env reverse sweep of an open-loop rollout (eb_rollout_tape_vjp), on top of eb_grad_device.h.
//
// What the reverse of H chained model steps needs from the forward is local to an env (the vehicle columns carry no
// cotangent, the vehicles do not depend on the ego, the closest path point is a constant):
//   per step   the pre-step ego state (6), the tracking triple the reward reads (3), the raw action (2), the five out5 cotangents,
//              and the vehicles' part — the three ego partials (x, y, heading) of that step's near records, summed in slot order.
// The vehicles' part can be formed in the FORWARD direction, because the out5 cotangents that scale it are known at launch.
// tape_reverse then runs grad::env_vjp last step first — the very lines one eb_rollout_step_vjp launch per step runs, fed the same
// values, so the same bits.  __host__ __device__: the kernel (eb_rollout_tape_vjp.hip) and a CPU harness run this text.
#pragma once
#include "eb_grad_device.h"

namespace eb {
namespace grad {

// one near record (x, y, heading in degrees) against the ego pose (x, y, sin, cos): its three ego partials, as the step VJP's queue
// pass forms them (eb_rollout_vjp.hip, phase 1b).  vs / vc: sin / cos of the record's heading (the forward's penalty terms share them).
EB_HD void record_partials(float ex, float ey, float es, float ec, float vx, float vy, float vs, float vc, float w35, float w25,
                           float& px, float& py, float& pphi) {
    px = 0.0f; py = 0.0f; pphi = 0.0f;
    veh_pair_vjp(ex, ey, es, ec, vx, vy, vs, vc, w35, w25, px, py, pphi);
}

// is the record's centre close enough to the ego for any circle pair to be within 3.5 m (DAM:228)?
EB_HD bool record_near(float ex, float ey, float vx, float vy) {
    const float cx = ex - vx, cy = ey - vy;
    return cx * cx + cy * cy < NEAR_R * NEAR_R;
}

// what one step leaves for the reverse sweep
struct TapeStep {
    float st[6];          // pre-step v_x, v_y, r, x, y, phi (deg)
    float trk[3];         // pre-step tracking triple
    float a0, a1;         // raw action of the step
    float w[5];           // cotangents of the step's out5
    float px, py, pphi;   // the vehicles' part
};

// Reverse sweep over `horizon` steps of one env.
//   g_final[9], ffx / ffy / ffphi: cotangent of the final obs' columns 0..8 and the sums over its look-ahead columns (DAM:763-768);
//   load(t, TapeStep&): step t's record;  store(t, ga[2]): the cotangent of step t's raw action;
//   go[0..8]: cotangent of obs0's columns 0..8 (its look-ahead columns feed nothing: zero).
template <int TASK, class Load, class Store>
EB_HD void tape_reverse(int horizon, bool has_path, const float (&g_final)[9], float ffx, float ffy, float ffphi, Load&& load,
                        Store&& store, float (&go)[9]) {
    EnvIn I;
    I.has_path = has_path;
#pragma unroll
    for (int c = 0; c < 9; ++c) I.g[c] = g_final[c];
    I.fx = ffx; I.fy = ffy; I.fphi = ffphi;
    for (int t = horizon - 1; t >= 0; --t) {
        TapeStep T;
        load(t, T);
#pragma unroll
        for (int c = 0; c < 6; ++c) I.st[c] = T.st[c];
#pragma unroll
        for (int c = 0; c < 3; ++c) I.trk[c] = T.trk[c];
        I.a0 = T.a0; I.a1 = T.a1;
#pragma unroll
        for (int k = 0; k < 5; ++k) I.w[k] = T.w[k];
        I.px = T.px; I.py = T.py; I.pphi = T.pphi;
        sincos_hd(deg2rad_hd(I.st[5]), I.es, I.ec);                            // DAM:211
        float ga[2];
        env_vjp<TASK>(I, go, ga);
        store(t, ga);
#pragma unroll
        for (int c = 0; c < 9; ++c) I.g[c] = go[c];
        I.fx = I.fy = I.fphi = 0.0f;               // a pre-step obs' look-ahead columns feed nothing (DAM:189-207, 322-333)
    }
}

}  // namespace grad
}  // namespace eb
