// CPU harness of the open-loop reverse sweep (tests/test_tape_grad_host.py): the __host__ __device__ functions of
// env_build_amd/csrc/eb_tape_grad_device.h — the text the gfx950 kernel eb_rollout_tape_vjp runs per env — evaluated row by row on
// the host.  The forward's pre-step obs of every step come from the caller (the CPU oracle's eb_rollout_step, bit-identical to the
// HIP forward); per step the near records' partials are formed and summed in slot order as the kernel's phases (C) and (D) do, then
// grad::tape_reverse runs last step first.
#include <hip/hip_runtime.h>

#include "eb_tape_grad_device.h"

using namespace eb;

template <int TASK>
static void rows(int n, int H, int D, int nd, int nv, int nf, const float* obs_steps, const float* tape, const int* has_path,
                 const float* g_final, const float* g5, const float* w5, float* go_out, float* ga_out) {
    for (int i = 0; i < n; ++i) {
        auto load = [&](int t, grad::TapeStep& T) {
            const float* o = obs_steps + ((size_t)t * n + i) * D;
            for (int c = 0; c < 6; ++c) T.st[c] = o[c];
            for (int c = 0; c < 3; ++c) T.trk[c] = o[6 + c];
            T.a0 = tape[2 * ((size_t)t * n + i)]; T.a1 = tape[2 * ((size_t)t * n + i) + 1];
            for (int k = 0; k < 5; ++k) T.w[k] = g5 ? g5[((size_t)t * 5 + k) * n + i] : w5[k];
            float es, ec;
            grad::sincos_hd(grad::deg2rad_hd(T.st[5]), es, ec);
            T.px = T.py = T.pphi = 0.0f;
            for (int j = 0; j < nv; ++j) {                       // slot order
                const float* v = o + nd + 4 * j;
                if (!grad::record_near(T.st[3], T.st[4], v[0], v[1])) continue;
                float vs, vc, px, py, pphi;
                grad::sincos_hd(grad::deg2rad_hd(v[3]), vs, vc);
                grad::record_partials(T.st[3], T.st[4], es, ec, v[0], v[1], vs, vc, T.w[1], T.w[2] + T.w[3], px, py, pphi);
                T.px += px; T.py += py; T.pphi += pphi;
            }
        };
        auto store = [&](int t, const float (&ga)[2]) {
            ga_out[2 * ((size_t)t * n + i)] = ga[0]; ga_out[2 * ((size_t)t * n + i) + 1] = ga[1];
        };
        const float* gf = g_final + (size_t)i * nd;
        float g9[9], ffx = 0.0f, ffy = 0.0f, ffphi = 0.0f, go[9];
        for (int c = 0; c < 9; ++c) g9[c] = gf[c];
        for (int k = 0; k < nf; ++k) { ffx += gf[9 + 3 * k]; ffy += gf[10 + 3 * k]; ffphi += gf[11 + 3 * k]; }
        grad::tape_reverse<TASK>(H, has_path[i] != 0, g9, ffx, ffy, ffphi, load, store, go);
        for (int c = 0; c < nd; ++c) go_out[(size_t)i * nd + c] = c < 9 ? go[c] : 0.0f;
    }
}

// obs_steps [H, n, D]: the pre-step obs of every step; g5 [H, 5, n] or NULL (then w5[5] at every step and env)
extern "C" void host_tape_vjp(int task, int n, int H, int D, int nd, int nv, int nf, const float* obs_steps, const float* tape,
                              const int* has_path, const float* g_final, const float* g5, const float* w5, float* go, float* ga) {
    if (task == TASK_LEFT) rows<TASK_LEFT>(n, H, D, nd, nv, nf, obs_steps, tape, has_path, g_final, g5, w5, go, ga);
    else if (task == TASK_STRAIGHT) rows<TASK_STRAIGHT>(n, H, D, nd, nv, nf, obs_steps, tape, has_path, g_final, g5, w5, go, ga);
    else rows<TASK_RIGHT>(n, H, D, nd, nv, nf, obs_steps, tape, has_path, g_final, g5, w5, go, ga);
}
