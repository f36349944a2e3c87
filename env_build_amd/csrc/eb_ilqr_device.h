// eb_ilqr_device.h — the pieces of one iLQR iteration on the model rollout (eb_rollout_tape_ilqr, include/envbuild_ilqr.h), on top of
// eb_tape_grad_device.h: the feedback law of a closed-loop candidate, the quadratic model of one step (the step VJP's own Jacobian
// rows and the Gauss-Newton Hessian of the step's cost), the two-dimensional box QP and one step of the backward (Riccati) sweep.
// Every function is __host__ __device__: the kernel (eb_rollout_tape_ilqr.hip) and a CPU harness run the same text.
//
// The model lives in the step VJP's space: z = obs columns 0..8, u = the raw action.  Columns 6..8 (the tracking triple) of a
// pre-step obs feed the step's reward only — never the next obs — so columns 6..8 of A are zero, Q_uz has no such columns, K has
// none, and V_zz keeps the block form  [V66 0; 0 diag(d)]  with d the reward's own curvature of the step.  The sweep therefore
// carries a symmetric 6 x 6 matrix, three diagonal entries and a 9-vector.
#pragma once
#include "eb_tape_grad_device.h"

namespace eb {
namespace ilqr {

constexpr int GAIN_ROWS = 14;      // k (2), K (2 x 6, row-major)
constexpr int LQ_ROWS = 157;       // A 81, B 18, l_z 9, l_u 2, l_zz 45 (upper triangle, row-major), l_uu 2
constexpr int TAPE_FLOATS = 20;    // what a step leaves for the sweep: st 6, trk 3, raw action 2, vehicles' partials 3, their GN block 6

EB_HD float clamp1(float x) { return x < -1.0f ? -1.0f : (x > 1.0f ? 1.0f : x); }   // two compares: a NaN stays a NaN

// index of (i, j), i <= j, in the row-major upper triangle of a symmetric N x N matrix
template <int N> EB_HD constexpr int tri(int i, int j) { return i * N - (i * (i - 1)) / 2 + (j - i); }

// ---- the feedback law (include/envbuild_ilqr.h: candidates) ----
// g: the step's 14 gain entries; x: the candidate's pre-step obs columns 0..5; xn: the nominal's.  One rounding per operation.
EB_HD void feedback_action(float alpha, const float (&g)[GAIN_ROWS], const float (&x)[6], const float (&xn)[6], float un0, float un1,
                           float& u0, float& u1) {
    float du0 = alpha * g[0], du1 = alpha * g[1];
#pragma unroll
    for (int c = 0; c < 6; ++c) du0 = du0 + g[2 + c] * (x[c] - xn[c]);
#pragma unroll
    for (int c = 0; c < 6; ++c) du1 = du1 + g[8 + c] * (x[c] - xn[c]);
    u0 = clamp1(un0 + du0);
    u1 = clamp1(un1 + du1);
}

// ---- Gauss-Newton pieces: 2 c grad(r) grad(r)^T over the residuals ACTIVE in the forward ----
// One vehicle against the ego, the four circle pairs of DAM:218-229 with veh_pair_vjp's own distances and branch decisions.
// h[6] += the (x, y, heading in radians) block, upper triangle: xx, xy, xp, yy, yp, pp.  A zero distance contributes zero.
EB_HD void veh_pair_gn(float ex, float ey, float es, float ec, float vx, float vy, float vs, float vc, float w35, float w25, float (&h)[6]) {
    const float epx[2] = {ex + LWS * ec, ex - LWS * ec}, epy[2] = {ey + LWS * es, ey - LWS * es};   // DAM:211-214
    const float wx[2] = {vx + LWS * vc, vx - LWS * vc}, wy[2] = {vy + LWS * vs, vy - LWS * vs};     // DAM:221-224
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float dx = epx[p] - wx[q], dy = epy[p] - wy[q];
            const float d = sqrtf(grad::sqf(dx) + grad::sqf(dy));        // DAM:227
            const float a = d - 3.5f, b = d - 2.5f;
            float c = 0.0f;
            if (a < 0.0f) c += w35;                                      // DAM:228
            if (b < 0.0f) c += w25;                                      // DAM:229
            if (d > 0.0f && c != 0.0f) {
                const float nx = dx / d, ny = dy / d;
                const float np = (p == 0 ? LWS : -LWS) * (ny * ec - nx * es);
                const float c2 = 2.0f * c;
                h[0] += c2 * (nx * nx); h[1] += c2 * (nx * ny); h[2] += c2 * (nx * np);
                h[3] += c2 * (ny * ny); h[4] += c2 * (ny * np); h[5] += c2 * (np * np);
            }
        }
}

// The walls of one ego point (DAM:231-295), road_terms_vjp's conditions: cx / cy += the cost weight of every active residual in the
// point's x / in its y (each wall's residual is +-(coordinate) + constant, so its gradient is a unit vector).
template <int TASK>
EB_HD void road_terms_gn(float px, float py, float wt, float wr, float& cx, float& cy) {
    constexpr float LWN = 11.25f, LW2 = 7.5f;
    const float w = wt + wr;
    if (TASK == TASK_LEFT) {            // DAM:233-251
        if (py < -HALF_CROSS && px < 1.0f) cx += w;
        if (py < -HALF_CROSS && LANE_W - px < 1.0f) cx += w;
        if (px < 0.0f && LWN - py < 1.0f) cy += wt;
        if (px < -HALF_CROSS && LWN - py < 1.0f) cy += wr;
        if (px < -HALF_CROSS && py - 0.0f < 1.0f) cy += w;
    } else if (TASK == TASK_STRAIGHT) { // DAM:252-272
        if (py < -HALF_CROSS && px - LANE_W < 1.0f) cx += w;
        if (py < -HALF_CROSS && LW2 - px < 1.0f) cx += w;
        if (py > HALF_CROSS && LWN - px < 1.0f) cx += w;
        if (py > HALF_CROSS && px - 0.0f < 1.0f) cx += w;
    } else {                            // DAM:273-295
        if (py < -HALF_CROSS && px - LW2 < 1.0f) cx += w;
        if (py < -HALF_CROSS && LWN - px < 1.0f) cx += w;
        if (px > HALF_CROSS && 0.0f - py < 1.0f) cy += w;
        if (px > HALF_CROSS && py - (-LWN) < 1.0f) cy += w;
    }
}

// ---- the quadratic model of one step ----
struct StepIn {
    float st[6], trk[3], a0, a1;   // pre-step obs columns 0..8 and the raw action
    float px, py, pphi;            // the vehicles' part of l_z (record_partials summed in slot order, cotangents w5[1], w5[2] + w5[3])
    float hv[6];                   // the vehicles' part of l_zz (veh_pair_gn summed in slot order), heading in radians
    bool has_path;
};
struct StepLQ {
    float F[9][8];     // row i: d z'_i / d (z_0..5, u_0, u_1) — rows of A (columns 0..5) and of B
    float lz[9], lu[2];
    float h22;         // l_zz: (2, 2); the block of columns 3..5 (upper triangle: 33 34 35 44 45 55); the diagonal of columns 6..8;
    float hp[6];       //       every other entry is zero
    float hd[3];
    float luu[2];      // l_uu (diagonal; l_uz = 0)
};

// tail(i, a6, a7, a8): columns 6..8 of row i of A as env_vjp returns them (zeros), i = 0..8, then i = 9 for l_z's own — for lq_out
template <int TASK, class Tail>
EB_HD void step_model(const StepIn& S, const float (&w5)[5], StepLQ& M, Tail&& tail) {
    grad::EnvIn I;
#pragma unroll
    for (int c = 0; c < 6; ++c) I.st[c] = S.st[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) I.trk[c] = S.trk[c];
    I.a0 = S.a0; I.a1 = S.a1;
    I.has_path = S.has_path;
    grad::sincos_hd(grad::deg2rad_hd(I.st[5]), I.es, I.ec);                    // DAM:211
    I.fx = I.fy = I.fphi = 0.0f;
    float go[9], ga[2];
    // rows of A and B: the step VJP with g_obs_out = e_i, g_out5 = 0 (the vehicles' part scales with g_out5: zero)
#pragma unroll
    for (int k = 0; k < 5; ++k) I.w[k] = 0.0f;
    I.px = I.py = I.pphi = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
#pragma unroll
        for (int c = 0; c < 9; ++c) I.g[c] = c == i ? 1.0f : 0.0f;
        grad::env_vjp<TASK>(I, go, ga);
#pragma unroll
        for (int c = 0; c < 6; ++c) M.F[i][c] = go[c];
        M.F[i][6] = ga[0]; M.F[i][7] = ga[1];
        tail(i, go[6], go[7], go[8]);
    }
    // l_z, l_u: g_obs_out = 0, g_out5 = w5
#pragma unroll
    for (int c = 0; c < 9; ++c) I.g[c] = 0.0f;
#pragma unroll
    for (int k = 0; k < 5; ++k) I.w[k] = w5[k];
    I.px = S.px; I.py = S.py; I.pphi = S.pphi;
    grad::env_vjp<TASK>(I, go, ga);
#pragma unroll
    for (int c = 0; c < 9; ++c) M.lz[c] = go[c];
    M.lu[0] = ga[0]; M.lu[1] = ga[1];
    tail(9, go[6], go[7], go[8]);
    // Gauss-Newton Hessian.  Rewards (DAM:198-207, 297-298): cost -w5[0] * (0.05 v^2 + 0.8 y^2 + 30 phi_rad^2 + 0.02 r^2 + 5 steer^2 +
    // 0.05 a_x^2), every residual linear in z or in the clipped action.
    const float cR = -w5[0];
    M.h22 = (2.0f * 0.02f) * cR;
    M.hd[0] = (2.0f * 0.8f) * cR;
    M.hd[1] = (2.0f * 30.0f * grad::DEG2RAD * grad::DEG2RAD) * cR;
    M.hd[2] = (2.0f * 0.05f) * cR;
    const bool pass0 = S.a0 >= -1.05f && S.a0 <= 1.05f, pass1 = S.a1 >= -1.05f && S.a1 <= 1.05f;   // DAM:129
    M.luu[0] = pass0 ? (2.0f * 5.0f * 0.4f * 0.4f) * cR : 0.0f;
    M.luu[1] = pass1 ? (2.0f * 0.05f * 2.25f * 2.25f) * cR : 0.0f;
    // walls on the ego's two circle centres (x +- LWS cos, y +- LWS sin): d px / d phi = -+LWS sin, d py / d phi = +-LWS cos
    const float wt = w5[1], wr = w5[2] + w5[4];
    const float x = S.st[3], y = S.st[4], sn = I.es, cs = I.ec;
    float fcx = 0.0f, fcy = 0.0f, rcx = 0.0f, rcy = 0.0f;
    road_terms_gn<TASK>(x + LWS * cs, y + LWS * sn, wt, wr, fcx, fcy);
    road_terms_gn<TASK>(x - LWS * cs, y - LWS * sn, wt, wr, rcx, rcy);
    const float ls = LWS * sn, lc = LWS * cs;
    float h[6];                                                                // x, y, heading in radians
    h[0] = 2.0f * (fcx + rcx);
    h[1] = 0.0f;
    h[2] = 2.0f * ((rcx - fcx) * ls);
    h[3] = 2.0f * (fcy + rcy);
    h[4] = 2.0f * ((fcy - rcy) * lc);
    h[5] = 2.0f * ((fcx + rcx) * (ls * ls) + (fcy + rcy) * (lc * lc));
#pragma unroll
    for (int k = 0; k < 6; ++k) h[k] += S.hv[k];
    M.hp[0] = h[0]; M.hp[1] = h[1]; M.hp[2] = h[2] * grad::DEG2RAD;             // obs column 5 is in degrees
    M.hp[3] = h[3]; M.hp[4] = h[4] * grad::DEG2RAD; M.hp[5] = h[5] * (grad::DEG2RAD * grad::DEG2RAD);
}

// ---- the box QP in two dimensions ----
// min 1/2 d^T Q d + q^T d  s.t.  lo <= d <= hi, by enumeration.  A component is free (F), at its lower (L) or at its upper (U) bound;
// the sets are tried in the order (u_0, u_1) = FF, LF, UF, FL, FU, LL, LU, UL, UU.  A set is taken when its free block is finite and
// positive definite, its free components lie in [lo, hi], and the gradient Q d + q is >= 0 on every L and <= 0 on every U component.
// -> the set's index, or -1 when none is taken (d = 0 then).
typedef double acc_t;   // the working type of the sweep (see riccati_step)
struct BoxSol { acc_t d0, d1; bool free0, free1; int set; };
EB_HD bool is_finite(acc_t x) { return x - x == 0.0; }
EB_HD BoxSol box_qp2(acc_t q00, acc_t q01, acc_t q11, acc_t g0, acc_t g1, acc_t lo0, acc_t hi0, acc_t lo1, acc_t hi1) {
    BoxSol R;
    R.d0 = 0.0; R.d1 = 0.0; R.free0 = false; R.free1 = false; R.set = -1;
#pragma unroll
    for (int s = 0; s < 9; ++s) {
        // component states: 0 free, 1 lower, 2 upper
        const int s0 = s == 0 || s == 3 || s == 4 ? 0 : (s == 1 || s == 5 || s == 6 ? 1 : 2);
        const int s1 = s == 0 || s == 1 || s == 2 ? 0 : (s == 3 || s == 5 || s == 7 ? 1 : 2);
        acc_t d0 = s0 == 1 ? lo0 : hi0, d1 = s1 == 1 ? lo1 : hi1;
        bool ok = true;
        if (s0 == 0 && s1 == 0) {
            const acc_t det = q00 * q11 - q01 * q01;
            ok = q00 > 0.0 && det > 0.0 && is_finite(q00) && is_finite(det);
            d0 = (q01 * g1 - q11 * g0) / det;
            d1 = (q01 * g0 - q00 * g1) / det;
        } else if (s0 == 0) {
            ok = q00 > 0.0 && is_finite(q00);
            d0 = -(g0 + q01 * d1) / q00;
        } else if (s1 == 0) {
            ok = q11 > 0.0 && is_finite(q11);
            d1 = -(g1 + q01 * d0) / q11;
        }
        if (s0 == 0) ok = ok && d0 >= lo0 && d0 <= hi0;
        if (s1 == 0) ok = ok && d1 >= lo1 && d1 <= hi1;
        const acc_t r0 = (q00 * d0 + q01 * d1) + g0, r1 = (q01 * d0 + q11 * d1) + g1;
        if (s0 == 1) ok = ok && r0 >= 0.0;
        if (s0 == 2) ok = ok && r0 <= 0.0;
        if (s1 == 1) ok = ok && r1 >= 0.0;
        if (s1 == 2) ok = ok && r1 <= 0.0;
        ok = ok && is_finite(d0) && is_finite(d1);
        if (ok && R.set < 0) { R.d0 = d0; R.d1 = d1; R.free0 = s0 == 0; R.free1 = s1 == 0; R.set = s; }
    }
    return R;
}

// ---- one step of the backward sweep ----
struct Value {
    acc_t vz[9];       // V_z
    acc_t v66[21];     // V_zz, columns 0..5, upper triangle
    acc_t vd[3];       // V_zz, the diagonal of columns 6..8
};
EB_HD void value_zero(Value& V) {
#pragma unroll
    for (int c = 0; c < 9; ++c) V.vz[c] = 0.0;
#pragma unroll
    for (int c = 0; c < 21; ++c) V.v66[c] = 0.0;
    V.vd[0] = V.vd[1] = V.vd[2] = 0.0;
}
EB_HD acc_t sym6(const acc_t (&v)[21], int i, int j) { return i <= j ? v[tri<6>(i, j)] : v[tri<6>(j, i)]; }

// V (of the step after) -> V (of this step), the step's gains g[14] and its two dv terms; u0 / u1: the step's (clamped) action.
// The sweep works in double (acc_t) on the fp32 model and rounds the gains to fp32 once, at the end: the order and rounding of its
// sums are the kernel's own (include/envbuild_ilqr.h).  In crowded scenes Q_uu = l_uu + B^T V' B is ill-conditioned (l_zz in the
// thousands against l_uu near one), and an fp32 sweep's rounding came out at up to ten times the distance between the restatement's
// own float32 and float64 runs; the sweep is a few hundred operations per step on one lane.
EB_HD int riccati_step(const StepLQ& M, float mu, float u0, float u1, Value& V, float (&g)[GAIN_ROWS], acc_t& dv1, acc_t& dv2) {
    // Q_x (8): (z_0..5, u); Q_xx (8 x 8, upper triangle) = L + F^T V' F
    acc_t qx[8], Q[36];
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        acc_t acc = b < 6 ? M.lz[b] : M.lu[b - 6];
#pragma unroll
        for (int i = 0; i < 9; ++i) acc = fma(M.F[i][b], V.vz[i], acc);
        qx[b] = acc;
        acc_t w[6];                                                            // V66 F[:, b]
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            acc_t s = 0.0;
#pragma unroll
            for (int j = 0; j < 6; ++j) s = fma(sym6(V.v66, i, j), M.F[j][b], s);
            w[i] = s;
        }
#pragma unroll
        for (int a = 0; a <= b; ++a) {
            acc_t s = 0.0;
#pragma unroll
            for (int i = 0; i < 6; ++i) s = fma(M.F[i][a], w[i], s);
#pragma unroll
            for (int i = 6; i < 9; ++i) s = fma(M.F[i][a] * V.vd[i - 6], M.F[i][b], s);
            Q[tri<8>(a, b)] = s;
        }
    }
    Q[tri<8>(2, 2)] += M.h22;
    Q[tri<8>(3, 3)] += M.hp[0]; Q[tri<8>(3, 4)] += M.hp[1]; Q[tri<8>(3, 5)] += M.hp[2];
    Q[tri<8>(4, 4)] += M.hp[3]; Q[tri<8>(4, 5)] += M.hp[4]; Q[tri<8>(5, 5)] += M.hp[5];
    Q[tri<8>(6, 6)] += M.luu[0]; Q[tri<8>(7, 7)] += M.luu[1];
    const acc_t quu00 = Q[tri<8>(6, 6)], quu01 = Q[tri<8>(6, 7)], quu11 = Q[tri<8>(7, 7)];
    const BoxSol B = box_qp2(quu00 + mu, quu01, quu11 + mu, qx[6], qx[7], -1.0 - u0, 1.0 - u0, -1.0 - u1, 1.0 - u1);
    acc_t K0[6], K1[6];
    const acc_t t00 = quu00 + mu, t11 = quu11 + mu;
    const acc_t det = t00 * t11 - quu01 * quu01;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
        const acc_t z0 = Q[tri<8>(c, 6)], z1 = Q[tri<8>(c, 7)];                // Q_uz[0][c], Q_uz[1][c]
        acc_t a = 0.0, b = 0.0;
        if (B.free0 && B.free1) { a = (quu01 * z1 - t11 * z0) / det; b = (quu01 * z0 - t00 * z1) / det; }
        else if (B.free0) a = -z0 / t00;
        else if (B.free1) b = -z1 / t11;
        K0[c] = a; K1[c] = b;
    }
    const acc_t k0 = B.d0, k1 = B.d1;
    g[0] = (float)k0; g[1] = (float)k1;
#pragma unroll
    for (int c = 0; c < 6; ++c) { g[2 + c] = (float)K0[c]; g[8 + c] = (float)K1[c]; }
    // Q_uu k, and the two dv terms
    const acc_t m0 = quu00 * k0 + quu01 * k1, m1 = quu01 * k0 + quu11 * k1;
    dv1 = k0 * qx[6] + k1 * qx[7];
    dv2 = k0 * m0 + k1 * m1;
    // V_z = Q_z + K^T (Q_uu k + Q_u) + Q_uz^T k;  V_zz = Q_zz + K^T Q_uu K + K^T Q_uz + Q_uz^T K (symmetric as written)
    acc_t n0[6], n1[6];                                                        // Q_uu K
#pragma unroll
    for (int c = 0; c < 6; ++c) { n0[c] = quu00 * K0[c] + quu01 * K1[c]; n1[c] = quu01 * K0[c] + quu11 * K1[c]; }
#pragma unroll
    for (int c = 0; c < 6; ++c)
        V.vz[c] = qx[c] + (K0[c] * (m0 + qx[6]) + K1[c] * (m1 + qx[7])) + (Q[tri<8>(c, 6)] * k0 + Q[tri<8>(c, 7)] * k1);
#pragma unroll
    for (int c = 6; c < 9; ++c) V.vz[c] = M.lz[c];
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j)
            V.v66[tri<6>(i, j)] = Q[tri<8>(i, j)] + (K0[i] * n0[j] + K1[i] * n1[j]) +
                                  ((K0[i] * Q[tri<8>(j, 6)] + K1[i] * Q[tri<8>(j, 7)]) + (Q[tri<8>(i, 6)] * K0[j] + Q[tri<8>(i, 7)] * K1[j]));
    V.vd[0] = M.hd[0]; V.vd[1] = M.hd[1]; V.vd[2] = M.hd[2];
    return B.set;
}

}  // namespace ilqr
}  // namespace eb
