// CPU harness of the iLQR iteration (tests/test_tape_ilqr_host.py): the __host__ __device__ functions of
// env_build_amd/csrc/eb_ilqr_device.h — the text the gfx950 kernel eb_rollout_tape_ilqr runs per env — evaluated row by row on the
// host.  The forward's pre-step obs of every step come from the caller (the CPU oracle's eb_rollout_step, bit-identical to the HIP
// forward); per step the near records' parts are formed and summed in slot order as the kernel's pass 2 does, then
// ilqr::step_model and ilqr::riccati_step run last step first.
#include <hip/hip_runtime.h>

#include "eb_ilqr_device.h"

using namespace eb;

static void step_in(const float* o, const float* a, int nd, int nv, bool has_path, const float* w5, ilqr::StepIn& S) {
    for (int c = 0; c < 6; ++c) S.st[c] = o[c];
    for (int c = 0; c < 3; ++c) S.trk[c] = o[6 + c];
    S.a0 = a[0]; S.a1 = a[1];
    S.has_path = has_path;
    float es, ec;
    grad::sincos_hd(grad::deg2rad_hd(S.st[5]), es, ec);
    S.px = S.py = S.pphi = 0.0f;
    for (int k = 0; k < 6; ++k) S.hv[k] = 0.0f;
    for (int j = 0; j < nv; ++j) {                           // slot order
        const float* v = o + nd + 4 * j;
        if (!grad::record_near(S.st[3], S.st[4], v[0], v[1])) continue;
        float vs, vc, px, py, pphi;
        grad::sincos_hd(grad::deg2rad_hd(v[3]), vs, vc);
        grad::record_partials(S.st[3], S.st[4], es, ec, v[0], v[1], vs, vc, w5[1], w5[2] + w5[3], px, py, pphi);
        S.px += px; S.py += py; S.pphi += pphi;
        ilqr::veh_pair_gn(S.st[3], S.st[4], es, ec, v[0], v[1], vs, vc, w5[1], w5[2] + w5[3], S.hv);
    }
}

template <int TASK>
static void rows(int n, int H, int D, int nd, int nv, const float* obs_steps, const float* tape, const int* has_path, const float* w5p,
                 const float* mu, float* lq, float* gains, float* dv, int* sets) {
    float w5[5];
    for (int k = 0; k < 5; ++k) w5[k] = w5p[k];
    for (int i = 0; i < n; ++i) {
        ilqr::Value V;
        ilqr::value_zero(V);
        ilqr::acc_t dv1 = 0.0, dv2 = 0.0;
        for (int t = H - 1; t >= 0; --t) {
            ilqr::StepIn S;
            step_in(obs_steps + ((size_t)t * n + i) * D, tape + 2 * ((size_t)t * n + i), nd, nv, has_path[i] != 0, w5, S);
            float* q = lq + (size_t)t * ilqr::LQ_ROWS * n + i;
            ilqr::StepLQ M;
            ilqr::step_model<TASK>(S, w5, M, [&](int r, float a6, float a7, float a8) {
                if (r < 9) { q[(size_t)(9 * r + 6) * n] = a6; q[(size_t)(9 * r + 7) * n] = a7; q[(size_t)(9 * r + 8) * n] = a8; }
            });
            for (int r = 0; r < 9; ++r) {
                for (int c = 0; c < 6; ++c) q[(size_t)(9 * r + c) * n] = M.F[r][c];
                q[(size_t)(81 + 2 * r) * n] = M.F[r][6];
                q[(size_t)(82 + 2 * r) * n] = M.F[r][7];
                q[(size_t)(99 + r) * n] = M.lz[r];
            }
            q[(size_t)108 * n] = M.lu[0]; q[(size_t)109 * n] = M.lu[1];
            for (int k = 0; k < 45; ++k) q[(size_t)(110 + k) * n] = 0.0f;
            q[(size_t)(110 + ilqr::tri<9>(2, 2)) * n] = M.h22;
            q[(size_t)(110 + ilqr::tri<9>(3, 3)) * n] = M.hp[0]; q[(size_t)(110 + ilqr::tri<9>(3, 4)) * n] = M.hp[1];
            q[(size_t)(110 + ilqr::tri<9>(3, 5)) * n] = M.hp[2]; q[(size_t)(110 + ilqr::tri<9>(4, 4)) * n] = M.hp[3];
            q[(size_t)(110 + ilqr::tri<9>(4, 5)) * n] = M.hp[4]; q[(size_t)(110 + ilqr::tri<9>(5, 5)) * n] = M.hp[5];
            for (int k = 0; k < 3; ++k) q[(size_t)(110 + ilqr::tri<9>(6 + k, 6 + k)) * n] = M.hd[k];
            q[(size_t)155 * n] = M.luu[0]; q[(size_t)156 * n] = M.luu[1];
            float g[ilqr::GAIN_ROWS];
            ilqr::acc_t d1, d2;
            sets[(size_t)t * n + i] = ilqr::riccati_step(M, mu ? mu[i] : 0.0f, S.a0, S.a1, V, g, d1, d2);
            dv1 += d1; dv2 += d2;
            for (int r = 0; r < ilqr::GAIN_ROWS; ++r) gains[((size_t)t * ilqr::GAIN_ROWS + r) * n + i] = g[r];
        }
        dv[i] = (float)dv1; dv[n + i] = (float)dv2;
    }
}

// obs_steps [H, n, D]: the pre-step obs of every step; tape [H, n, 2]: the (clamped) actions; -> lq [H, 157, n], gains [H, 14, n],
// dv [2, n], sets [H, n] (the box QP's active set per step, -1: the fallback)
extern "C" void host_ilqr(int task, int n, int H, int D, int nd, int nv, const float* obs_steps, const float* tape, const int* has_path,
                          const float* w5, const float* mu, float* lq, float* gains, float* dv, int* sets) {
    if (task == TASK_LEFT) rows<TASK_LEFT>(n, H, D, nd, nv, obs_steps, tape, has_path, w5, mu, lq, gains, dv, sets);
    else if (task == TASK_STRAIGHT) rows<TASK_STRAIGHT>(n, H, D, nd, nv, obs_steps, tape, has_path, w5, mu, lq, gains, dv, sets);
    else rows<TASK_RIGHT>(n, H, D, nd, nv, obs_steps, tape, has_path, w5, mu, lq, gains, dv, sets);
}

// The same rows of A / B / l_z / l_u straight from grad::env_vjp with unit cotangents (the step VJP's per-env text), one call per
// row: out [H, 10, 11, n] — row r < 9: go[0..8], ga[0..1] for g_obs_out = e_r, g_out5 = 0; row 9: for g_obs_out = 0, g_out5 = w5.
template <int TASK>
static void vjp_rows(int n, int H, int D, int nd, int nv, const float* obs_steps, const float* tape, const int* has_path, const float* w5,
                     float* out) {
    for (int i = 0; i < n; ++i)
        for (int t = 0; t < H; ++t) {
            ilqr::StepIn S;
            step_in(obs_steps + ((size_t)t * n + i) * D, tape + 2 * ((size_t)t * n + i), nd, nv, has_path[i] != 0, w5, S);
            for (int r = 0; r < 10; ++r) {
                grad::EnvIn I;
                for (int c = 0; c < 6; ++c) I.st[c] = S.st[c];
                for (int c = 0; c < 3; ++c) I.trk[c] = S.trk[c];
                I.a0 = S.a0; I.a1 = S.a1; I.has_path = S.has_path;
                grad::sincos_hd(grad::deg2rad_hd(I.st[5]), I.es, I.ec);
                for (int c = 0; c < 9; ++c) I.g[c] = c == r ? 1.0f : 0.0f;
                I.fx = I.fy = I.fphi = 0.0f;
                for (int k = 0; k < 5; ++k) I.w[k] = r == 9 ? w5[k] : 0.0f;
                I.px = r == 9 ? S.px : 0.0f; I.py = r == 9 ? S.py : 0.0f; I.pphi = r == 9 ? S.pphi : 0.0f;
                float go[9], ga[2];
                grad::env_vjp<TASK>(I, go, ga);
                float* o = out + (((size_t)t * 10 + r) * 11) * n + i;
                for (int c = 0; c < 9; ++c) o[(size_t)c * n] = go[c];
                o[(size_t)9 * n] = ga[0]; o[(size_t)10 * n] = ga[1];
            }
        }
}

extern "C" void host_vjp_rows(int task, int n, int H, int D, int nd, int nv, const float* obs_steps, const float* tape,
                              const int* has_path, const float* w5, float* out) {
    if (task == TASK_LEFT) vjp_rows<TASK_LEFT>(n, H, D, nd, nv, obs_steps, tape, has_path, w5, out);
    else if (task == TASK_STRAIGHT) vjp_rows<TASK_STRAIGHT>(n, H, D, nd, nv, obs_steps, tape, has_path, w5, out);
    else vjp_rows<TASK_RIGHT>(n, H, D, nd, nv, obs_steps, tape, has_path, w5, out);
}

// ilqr::feedback_action over a tape: u_nom [H, n, 2], x / x_nom [H, 6, n], gains [H, 14, n] -> u [H, n, 2]
extern "C" void host_feedback(int n, int H, float alpha, const float* u_nom, const float* x, const float* x_nom, const float* gains,
                              float* u) {
    for (int t = 0; t < H; ++t)
        for (int i = 0; i < n; ++i) {
            float g[ilqr::GAIN_ROWS], xs[6], xn[6];
            for (int r = 0; r < ilqr::GAIN_ROWS; ++r) g[r] = gains[((size_t)t * ilqr::GAIN_ROWS + r) * n + i];
            for (int c = 0; c < 6; ++c) { xs[c] = x[((size_t)t * 6 + c) * n + i]; xn[c] = x_nom[((size_t)t * 6 + c) * n + i]; }
            const size_t at = 2 * ((size_t)t * n + i);
            ilqr::feedback_action(alpha, g, xs, xn, u_nom[at], u_nom[at + 1], u[at], u[at + 1]);
        }
}

// ilqr::box_qp2 on n problems: Q [n, 3] (q00, q01, q11), g / lo / hi [n, 2] -> d [n, 2], set [n]
extern "C" void host_box_qp(int n, const float* Q, const float* g, const float* lo, const float* hi, float* d, int* set) {
    for (int i = 0; i < n; ++i) {
        const ilqr::BoxSol R = ilqr::box_qp2(Q[3 * i], Q[3 * i + 1], Q[3 * i + 2], g[2 * i], g[2 * i + 1], lo[2 * i], hi[2 * i], lo[2 * i + 1],
                                            hi[2 * i + 1]);
        d[2 * i] = (float)R.d0; d[2 * i + 1] = (float)R.d1; set[i] = R.set;
    }
}
