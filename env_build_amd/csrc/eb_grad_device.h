// eb_grad_device.h — the reverse pass (vector-Jacobian product) of one model step, EnvironmentModel.rollout_out (DAM:118-126).
//
// Closed-form transposes of the expressions in eb_device.h, written against the reference's lines (DAM = dynamics_and_models.py).
// Every function is __host__ __device__: the kernel (eb_rollout_vjp.hip) and a CPU harness run the same text.  On the device the
// forward quantities that DECIDE a branch (the clipped action, the pre-clip v_x, the circle distances, the ego corner points) are
// recomputed with the forward kernel's own helpers and operation order, so the reverse pass takes the branch the forward took.
//
// Conventions (what TensorFlow's and PyTorch's autograd do):
//   tf.where      — the cotangent goes to the selected branch only;
//   clip_by_value — the cotangent passes where lo <= x <= hi and is blocked outside;
//   argmin/gather — integers: the closest point and the +80 look-ahead points (DAM:702-733) are CONSTANTS.  Their values drop
//                   out of every derivative below (two2one and the look-ahead columns are differences against them, and
//                   deal_with_phi_diff has slope 1 on every piece), so the reverse pass never searches the path tables.
// One documented divergence: d sqrt(s)/ds at s == 0 (a circle distance, or the distance to the junction corner in two2one, of
// exactly zero) is NaN in the reference; the term contributes 0 here.
#pragma once
#include <math.h>

#include "eb_device.h"

#define EB_HD __host__ __device__ __forceinline__

namespace eb {
namespace grad {

constexpr float DEG2RAD = (float)(3.14159265358979323846 / 180.0);
constexpr float RAD2DEG = (float)(180.0 / 3.14159265358979323846);
constexpr float NEAR_R = 6.31f;   // 3.5 + 2 * LWS + slack: circle pairs of centres farther apart are all beyond 3.5 m (DAM:228)

EB_HD float sqf(float x) { return x * x; }

EB_HD float deg2rad_hd(float d) {
#if defined(__HIP_DEVICE_COMPILE__)
    return deg2rad(d);
#else
    return (float)((double)(d * PI_F) * (1.0 / 180.0));
#endif
}
EB_HD void sincos_hd(float x, float& s, float& c) {
#if defined(__HIP_DEVICE_COMPILE__)
    sincos_det(x, s, c);
#else
    s = sinf(x); c = cosf(x);
#endif
}

// ---- ego <-> vehicle two-circle penalties, DAM:218-229 ------------------------------------------------
// One vehicle (x, y, sin, cos of its heading) against the ego (x, y, sin, cos): adds the cotangent of the ego's x, y and heading
// (in radians).  w35 / w25: cotangents of veh2veh4training / veh2veh4real.
EB_HD void veh_pair_vjp(float ex, float ey, float es, float ec, float vx, float vy, float vs, float vc, float w35, float w25,
                        float& gx, float& gy, float& gphi) {
    const float epx[2] = {ex + LWS * ec, ex - LWS * ec}, epy[2] = {ey + LWS * es, ey - LWS * es};   // DAM:211-214
    const float wx[2] = {vx + LWS * vc, vx - LWS * vc}, wy[2] = {vy + LWS * vs, vy - LWS * vs};     // DAM:221-224
    float gpx[2] = {0.0f, 0.0f}, gpy[2] = {0.0f, 0.0f};
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float dx = epx[p] - wx[q], dy = epy[p] - wy[q];
            const float d = sqrtf(sqf(dx) + sqf(dy));                    // DAM:227
            const float a = d - 3.5f, b = d - 2.5f;
            float c = 0.0f;
            if (a < 0.0f) c += w35 * (2.0f * a);                         // DAM:228
            if (b < 0.0f) c += w25 * (2.0f * b);                         // DAM:229
            c = d > 0.0f ? c / d : 0.0f;                                 // sqrt'(0): 0 here, NaN in the reference
            gpx[p] += c * dx;
            gpy[p] += c * dy;
        }
    gx += gpx[0] + gpx[1];
    gy += gpy[0] + gpy[1];
    gphi += LWS * ((gpy[0] - gpy[1]) * ec - (gpx[0] - gpx[1]) * es);
}

// ---- road walls, DAM:231-295: one ego point; wt / wr = cotangents of veh2road4training / veh2road4real ----
template <int TASK>
EB_HD void road_terms_vjp(float px, float py, float wt, float wr, float& gpx, float& gpy) {
    constexpr float LWN = 11.25f, LW2 = 7.5f;
    const float w = wt + wr;
    if (TASK == TASK_LEFT) {            // DAM:233-251
        if (py < -HALF_CROSS && px < 1.0f) gpx += w * (2.0f * (px - 1.0f));
        if (py < -HALF_CROSS && LANE_W - px < 1.0f) gpx -= w * (2.0f * (LANE_W - px - 1.0f));
        if (px < 0.0f && LWN - py < 1.0f) gpy -= wt * (2.0f * (LWN - py - 1.0f));
        if (px < -HALF_CROSS && LWN - py < 1.0f) gpy -= wr * (2.0f * (LWN - py - 1.0f));
        if (px < -HALF_CROSS && py - 0.0f < 1.0f) gpy += w * (2.0f * (py - 0.0f - 1.0f));
    } else if (TASK == TASK_STRAIGHT) { // DAM:252-272
        if (py < -HALF_CROSS && px - LANE_W < 1.0f) gpx += w * (2.0f * (px - LANE_W - 1.0f));
        if (py < -HALF_CROSS && LW2 - px < 1.0f) gpx -= w * (2.0f * (LW2 - px - 1.0f));
        if (py > HALF_CROSS && LWN - px < 1.0f) gpx -= w * (2.0f * (LWN - px - 1.0f));
        if (py > HALF_CROSS && px - 0.0f < 1.0f) gpx += w * (2.0f * (px - 0.0f - 1.0f));
    } else {                            // DAM:273-295
        if (py < -HALF_CROSS && px - LW2 < 1.0f) gpx += w * (2.0f * (px - LW2 - 1.0f));
        if (py < -HALF_CROSS && LWN - px < 1.0f) gpx -= w * (2.0f * (LWN - px - 1.0f));
        if (px > HALF_CROSS && 0.0f - py < 1.0f) gpy -= w * (2.0f * (0.0f - py - 1.0f));
        if (px > HALF_CROSS && py - (-LWN) < 1.0f) gpy += w * (2.0f * (py - (-LWN) - 1.0f));
    }
}

// d delta_ / d(ego_xs, ego_ys) of two2one (DAM:736-752); the tracking column is -delta_
template <int TASK>
EB_HD void two2one_slope(float ex, float ey, float& sx, float& sy) {
    if (TASK == TASK_STRAIGHT) { sx = 1.0f; sy = 0.0f; return; }
    const float cx = TASK == TASK_LEFT ? -HALF_CROSS : HALF_CROSS, sign = TASK == TASK_LEFT ? 1.0f : -1.0f;
    const float ux = ex - cx, uy = ey - (-HALF_CROSS);
    const float d = sqrtf(sqf(ux) + sqf(uy));
    const float inv = d > 0.0f ? sign / d : 0.0f;
    sx = ux * inv; sy = uy * inv;
    if (ey < -HALF_CROSS) { sx = 1.0f; sy = 0.0f; }
    if (TASK == TASK_LEFT) { if (ex < -HALF_CROSS) { sx = 0.0f; sy = 1.0f; } }
    else if (ex > HALF_CROSS) { sx = 0.0f; sy = -1.0f; }
}

struct EnvIn {
    float st[6];       // v_x, v_y, r, x, y, phi (deg) of the pre-step obs
    float trk[3];      // its first tracking triple (the reward reads it, DAM:205-207)
    float a0, a1;      // RAW actions
    float es, ec;      // sin / cos of deg2rad(phi)
    bool has_path;     // the row tracks a path (training mode: ref_idx in range, DAM:342, 352)
    float g[9];        // cotangent of next obs columns 0..8
    float fx, fy, fphi;   // sums over the look-ahead points k of the cotangents of columns 9+3k, 10+3k, 11+3k (DAM:763-768)
    float w[5];        // cotangents of rewards, punish_term_for_training, real_punish_term, veh2veh4real, veh2road4real
    float px, py, pphi;   // the vehicles' part (veh_pair_vjp summed over the slots): ego x, y, heading in radians
};

// The env's part: tracking of the next pose, v_x clip, f_xu transposed, rewards, walls, action transform.
// go[0..8]: cotangent of obs columns 0..8 (columns 9.. of the pre-step obs feed nothing: zero); ga: of the raw actions.
template <int TASK>
EB_HD void env_vjp(const EnvIn& I, float (&go)[9], float (&ga)[2]) {
    using P = VehParams;
    const float tau = TAU10;
    const float v_x = I.st[0], v_y = I.st[1], r = I.st[2], x = I.st[3], y = I.st[4];
    const float sn = I.es, cs = I.ec;
    // forward pieces that decide branches, in the forward's operation order
    const bool pass0 = I.a0 >= -1.05f && I.a0 <= 1.05f, pass1 = I.a1 >= -1.05f && I.a1 <= 1.05f;   // DAM:129
    const float c0 = fminf(fmaxf(I.a0, -1.05f), 1.05f), c1 = fminf(fmaxf(I.a1, -1.05f), 1.05f);
    const float steer = 0.4f * c0, a_x = 2.25f * c1 - 0.75f;                                        // DAM:131
    const float k1 = P::a * P::C_f - P::b * P::C_r;
    const float nx0 = v_x + tau * (a_x + v_y * r);                                                  // DAM:73
    const float D1 = P::mass * v_x - tau * (P::C_f + P::C_r);
    const float nx1 = (P::mass * v_y * v_x + tau * k1 * r - tau * P::C_f * steer * v_x - tau * P::mass * sqf(v_x) * r) / D1;   // DAM:74-76
    const float D2 = tau * (sqf(P::a) * P::C_f + sqf(P::b) * P::C_r) - P::I_z * v_x;
    const float nx2 = (-P::I_z * r * v_x - tau * k1 * v_y + tau * P::a * P::C_f * steer * v_x) / D2;                          // DAM:77-78
    const float nx3 = x + tau * (v_x * cs - v_y * sn);                                              // DAM:79
    const float nx4 = y + tau * (v_x * sn + v_y * cs);                                              // DAM:80
    const bool pass_v = nx0 >= 0.0f && nx0 <= 35.0f;                                                // DAM:390

    // cotangent of the next ego state
    float n0 = I.g[0], n1 = I.g[1], n2 = I.g[2], n3 = I.g[3], n4 = I.g[4], n5 = I.g[5];
    if (I.has_path) {                                                                               // DAM:754-768
        float sx, sy;
        two2one_slope<TASK>(nx3, nx4, sx, sy);
        n3 -= I.g[6] * sx + I.fx;
        n4 -= I.g[6] * sy + I.fy;
        n5 += I.g[7] + I.fphi;
        n0 += I.g[8];
    }
    if (!pass_v) n0 = 0.0f;
    // f_xu transposed (DAM:73-81), tau = 0.1
    const float i1 = 1.0f / D1, i2 = 1.0f / D2;
    const float d1_vx = (P::mass * v_y - tau * P::C_f * steer - 2.0f * tau * P::mass * v_x * r - nx1 * P::mass) * i1;
    const float d1_vy = P::mass * v_x * i1;
    const float d1_r = (tau * k1 - tau * P::mass * sqf(v_x)) * i1;
    const float d1_s = -tau * P::C_f * v_x * i1;
    const float d2_vx = (-P::I_z * r + tau * P::a * P::C_f * steer + nx2 * P::I_z) * i2;
    const float d2_vy = -tau * k1 * i2;
    const float d2_r = -P::I_z * v_x * i2;
    const float d2_s = tau * P::a * P::C_f * v_x * i2;
    float g_vx = n0 + n1 * d1_vx + n2 * d2_vx + tau * (n3 * cs + n4 * sn);
    float g_vy = n0 * (tau * r) + n1 * d1_vy + n2 * d2_vy + tau * (n4 * cs - n3 * sn);
    float g_r = n0 * (tau * v_y) + n1 * d1_r + n2 * d2_r + n5 * (tau * RAD2DEG);
    float g_x = n3, g_y = n4;
    float g_phi_rad = tau * (n4 * (v_x * cs - v_y * sn) - n3 * (v_x * sn + v_y * cs));
    float g_steer = n1 * d1_s + n2 * d2_s;
    float g_ax = n0 * tau;
    // rewards (DAM:198-207, 297-298)
    const float wR = I.w[0];
    g_steer -= wR * (10.0f * steer);
    g_ax -= wR * (0.1f * a_x);
    g_r -= wR * (0.04f * r);
    go[6] = -wR * (1.6f * I.trk[0]);
    go[7] = -wR * ((60.0f * DEG2RAD * DEG2RAD) * I.trk[1]);
    go[8] = -wR * (0.1f * I.trk[2]);
    // road walls (DAM:231-295) on the ego's two circle centres, and the vehicles' part
    const float wt = I.w[1], wr = I.w[2] + I.w[4];
    float fpx = 0.0f, fpy = 0.0f, rpx = 0.0f, rpy = 0.0f;
    road_terms_vjp<TASK>(x + LWS * cs, y + LWS * sn, wt, wr, fpx, fpy);
    road_terms_vjp<TASK>(x - LWS * cs, y - LWS * sn, wt, wr, rpx, rpy);
    g_x += (fpx + rpx) + I.px;
    g_y += (fpy + rpy) + I.py;
    g_phi_rad += LWS * ((fpy - rpy) * cs - (fpx - rpx) * sn) + I.pphi;
    go[0] = g_vx; go[1] = g_vy; go[2] = g_r; go[3] = g_x; go[4] = g_y;
    go[5] = n5 + g_phi_rad * DEG2RAD;                                                               // DAM:54, 81
    ga[0] = pass0 ? 0.4f * g_steer : 0.0f;                                                          // DAM:129-131
    ga[1] = pass1 ? 2.25f * g_ax : 0.0f;
}

}  // namespace grad
}  // namespace eb
