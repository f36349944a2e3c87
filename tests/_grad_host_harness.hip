// CPU harness of the reverse pass's arithmetic (tests/test_grad_host.py): the __host__ __device__ functions of
// env_build_amd/csrc/eb_grad_device.h — the text the gfx950 kernel runs — evaluated row by row on the host, the vehicles
// summed in slot order.  Lets the math be held against the gradient fixtures on a machine without a GPU.
#include <hip/hip_runtime.h>

#include "eb_grad_device.h"

using namespace eb;

template <int TASK>
static void rows(int n, int D, int nd, int nv, int nf, const float* obs, const float* act, const int* has_path, const float* g,
                 const float* g5, float* go_out, float* ga_out) {
    for (int i = 0; i < n; ++i) {
        const float* o = obs + (size_t)i * D;
        const float* gi = g + (size_t)i * nd;
        grad::EnvIn I;
        for (int c = 0; c < 6; ++c) I.st[c] = o[c];
        for (int c = 0; c < 3; ++c) I.trk[c] = o[6 + c];
        I.a0 = act[2 * i]; I.a1 = act[2 * i + 1];
        I.has_path = has_path[i] != 0;
        for (int c = 0; c < 9; ++c) I.g[c] = gi[c];
        I.fx = I.fy = I.fphi = 0.0f;
        for (int k = 0; k < nf; ++k) { I.fx += gi[9 + 3 * k]; I.fy += gi[10 + 3 * k]; I.fphi += gi[11 + 3 * k]; }
        for (int k = 0; k < 5; ++k) I.w[k] = g5[(size_t)k * n + i];
        grad::sincos_hd(grad::deg2rad_hd(I.st[5]), I.es, I.ec);
        I.px = I.py = I.pphi = 0.0f;
        for (int j = 0; j < nv; ++j) {
            const float* v = o + nd + 4 * j;
            const float cx = I.st[3] - v[0], cy = I.st[4] - v[1];
            if (cx * cx + cy * cy < grad::NEAR_R * grad::NEAR_R) {
                float vs, vc;
                grad::sincos_hd(grad::deg2rad_hd(v[3]), vs, vc);
                grad::veh_pair_vjp(I.st[3], I.st[4], I.es, I.ec, v[0], v[1], vs, vc, I.w[1], I.w[2] + I.w[3], I.px, I.py, I.pphi);
            }
        }
        float go[9], ga[2];
        grad::env_vjp<TASK>(I, go, ga);
        for (int c = 0; c < nd; ++c) go_out[(size_t)i * nd + c] = c < 9 ? go[c] : 0.0f;
        ga_out[2 * i] = ga[0]; ga_out[2 * i + 1] = ga[1];
    }
}

extern "C" void host_step_vjp(int task, int n, int D, int nd, int nv, int nf, const float* obs, const float* act, const int* has_path,
                              const float* g, const float* g5, float* go, float* ga) {
    if (task == TASK_LEFT) rows<TASK_LEFT>(n, D, nd, nv, nf, obs, act, has_path, g, g5, go, ga);
    else if (task == TASK_STRAIGHT) rows<TASK_STRAIGHT>(n, D, nd, nv, nf, obs, act, has_path, g, g5, go, ga);
    else rows<TASK_RIGHT>(n, D, nd, nv, nf, obs, act, has_path, g, g5, go, ga);
}
