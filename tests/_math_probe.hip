// _math_probe.hip — TEST ONLY.  One elementwise kernel that evaluates, on the device and with the product's compiler flags, the
// hand-written fp32 functions the numerics contract rests on and the IEEE operations they are built from, so
// that tests/test_gpu_math_probe.py can hold each of them to the CPU oracle, to its NumPy twin and to IEEE arithmetic bit for bit.
// It includes the product's device headers and calls their functions; it defines no arithmetic of its own.  It is part of no product
// library, of no source list and of no hash (tests/_math_probe.py compiles it into a temporary directory once per test session).
//
// Layout: every argument array holds n elements, every output array n 4-byte elements.  a / b / c are read as float, uint32, uint64 or
// int32 as the operation says; o1 is written only by the operations with two results.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "eb_policy_logp_device.h"   // -> eb_policy_sample_device.h -> eb_env_device.h (-> eb_device.h), eb_mlp_device.h

#pragma clang fp contract(off)

namespace {

enum Op {   // tests/_math_probe.py:OPS names them in this order
    OP_SINCOS = 0,    // a: float x                      -> o0 = sin, o1 = cos            sincos_det
    OP_SINCOS_K,      // the same through sincos_det_k with sincos_consts()
    OP_ATAN,          // a: float x                      -> o0                            atan_det
    OP_EXP,           //                                                                  mlp::exp_det
    OP_ELU,           //                                                                  mlp::elu_det
    OP_TANH,          //                                                                  mlp::tanh_det
    OP_LOG,           //                                                                  psample::log_det
    OP_ARTANH,        //                                                                  plogp::artanh_log
    OP_DIV_10,        // a: float x                      -> o0 = div_const<C>(x)
    OP_DIV_180,
    OP_DIV_PI,
    OP_DIV_26875,
    OP_DIV_15625,
    OP_DIV_BY,        // a: float x, rc (a launch argument) -> o0 = div_by(x, rc)
    OP_DEG2RAD,
    OP_RAD2DEG,
    OP_DIV,           // a: float x, b: float y          -> o0 = x / y
    OP_RCP,           // a: float x                      -> o0 = 1.0f / x
    OP_SQRT,          // a: float x                      -> o0 = __builtin_sqrtf(x)
    OP_U01,           // a: uint64 key, b: uint64 idx    -> o0 = u01(key, idx)
    OP_NORMAL,        // a: uint64 key, b: uint64 id, c: int32 p, P (a launch argument) -> o0 = e0, o1 = e1     psample::normal_pair
    OP_F32_TO_F16,    // a: float x                      -> o0 = (float)(_Float16)x, o1 = the half's bits (uint32)
    OP_F16_TO_F32,    // a: uint32 half bits (low 16)    -> o0 = (float)half
    OP_COUNT
};

__global__ __launch_bounds__(256) void math_probe_kernel(int op, size_t n, const void* __restrict__ a, const void* __restrict__ b,
                                                         const void* __restrict__ c, int P, double rc, uint32_t* __restrict__ o0,
                                                         uint32_t* __restrict__ o1) {
    using namespace eb;
    const float* af = static_cast<const float*>(a);
    const float* bf = static_cast<const float*>(b);
    const uint32_t* au = static_cast<const uint32_t*>(a);
    const uint64_t* aq = static_cast<const uint64_t*>(a);
    const uint64_t* bq = static_cast<const uint64_t*>(b);
    const int32_t* ci = static_cast<const int32_t*>(c);
    const SinCosK K = sincos_consts();
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        float r0 = 0.0f, r1 = 0.0f;
        bool two = false, raw1 = false;
        uint32_t u1 = 0u;
        switch (op) {   // a launch argument: uniform over the grid
            case OP_SINCOS: sincos_det(af[i], r0, r1); two = true; break;
            case OP_SINCOS_K: sincos_det_k(af[i], K, r0, r1); two = true; break;
            case OP_ATAN: r0 = atan_det(af[i]); break;
            case OP_EXP: r0 = mlp::exp_det(af[i]); break;
            case OP_ELU: r0 = mlp::elu_det(af[i]); break;
            case OP_TANH: r0 = mlp::tanh_det(af[i]); break;
            case OP_LOG: r0 = psample::log_det(af[i]); break;
            case OP_ARTANH: r0 = plogp::artanh_log(af[i]); break;
            case OP_DIV_10: r0 = div_const<C10>(af[i]); break;
            case OP_DIV_180: r0 = div_const<C180>(af[i]); break;
            case OP_DIV_PI: r0 = div_const<CPi>(af[i]); break;
            case OP_DIV_26875: r0 = div_const<C26875>(af[i]); break;
            case OP_DIV_15625: r0 = div_const<C15625>(af[i]); break;
            case OP_DIV_BY: r0 = div_by(af[i], rc); break;
            case OP_DEG2RAD: r0 = deg2rad(af[i]); break;
            case OP_RAD2DEG: r0 = rad2deg(af[i]); break;
            case OP_DIV: r0 = af[i] / bf[i]; break;
            case OP_RCP: r0 = 1.0f / af[i]; break;
            case OP_SQRT: r0 = __builtin_sqrtf(af[i]); break;
            case OP_U01: r0 = u01(aq[i], bq[i]); break;
            case OP_NORMAL: psample::normal_pair(aq[i], bq[i], ci[i], P, r0, r1); two = true; break;
            case OP_F32_TO_F16: {
                const _Float16 h = (_Float16)af[i];          // the rollout kernels' store (eb_rollout.hip:Stored<_Float16>)
                r0 = (float)h;
                u1 = (uint32_t)__builtin_bit_cast(unsigned short, h);
                two = true; raw1 = true;
                break;
            }
            case OP_F16_TO_F32: r0 = (float)__builtin_bit_cast(_Float16, (unsigned short)(au[i] & 0xffffu)); break;
            default: break;
        }
        o0[i] = __builtin_bit_cast(uint32_t, r0);
        if (two) o1[i] = raw1 ? u1 : __builtin_bit_cast(uint32_t, r1);
    }
}

thread_local char g_err[256] = "";

int fail(hipError_t e, const char* what) {
    snprintf(g_err, sizeof g_err, "%s: %s (hipError %d)", what, hipGetErrorString(e), (int)e);
    return (int)e;
}

}  // namespace

extern "C" {

const char* eb_math_probe_last_error() { return g_err; }
int eb_math_probe_op_count() { return (int)OP_COUNT; }

// Runs operation `op` over n elements.  a / b / c: HOST arrays of a_bytes / b_bytes / c_bytes (NULL, 0: not used); o0 / o1: HOST arrays of
// n 4-byte elements (o1 NULL: not wanted).  Copies in, launches once, copies out.  -> 0, or the hipError_t of the first call that failed
// (eb_math_probe_last_error names it).
int eb_math_probe_run(int op, size_t n, const void* a, size_t a_bytes, const void* b, size_t b_bytes, const void* c, size_t c_bytes, int P,
                      double rc, void* o0, void* o1) {
    g_err[0] = 0;
    if (op < 0 || op >= (int)OP_COUNT || !a || !o0) {
        snprintf(g_err, sizeof g_err, "eb_math_probe_run: bad argument");
        return -1;
    }
    if (n == 0) return 0;
    const void* host[3] = {a, b, c};
    const size_t bytes[3] = {a_bytes, b_bytes, c_bytes};
    void* dev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    hipError_t e = hipSuccess;
    const char* what = "";
    for (int k = 0; k < 3 && e == hipSuccess; ++k) {
        if (!host[k] || !bytes[k]) continue;
        what = "hipMalloc";
        e = hipMalloc(&dev[k], bytes[k]);
        if (e == hipSuccess) { what = "hipMemcpy (in)"; e = hipMemcpy(dev[k], host[k], bytes[k], hipMemcpyHostToDevice); }
    }
    for (int k = 3; k < 5 && e == hipSuccess; ++k) {
        what = "hipMalloc";
        e = hipMalloc(&dev[k], n * 4);
        if (e == hipSuccess) { what = "hipMemset"; e = hipMemset(dev[k], 0, n * 4); }
    }
    if (e == hipSuccess) {
        const size_t want = (n + 255) / 256;
        const unsigned blocks = (unsigned)(want < 4096 ? want : 4096);
        math_probe_kernel<<<dim3(blocks), dim3(256), 0, 0>>>(op, n, dev[0], dev[1], dev[2], P, rc, static_cast<uint32_t*>(dev[3]),
                                                            static_cast<uint32_t*>(dev[4]));
        what = "hipLaunchKernel";
        e = hipGetLastError();
    }
    if (e == hipSuccess) { what = "hipDeviceSynchronize"; e = hipDeviceSynchronize(); }
    if (e == hipSuccess) { what = "hipMemcpy (out)"; e = hipMemcpy(o0, dev[3], n * 4, hipMemcpyDeviceToHost); }
    if (e == hipSuccess && o1) { what = "hipMemcpy (out)"; e = hipMemcpy(o1, dev[4], n * 4, hipMemcpyDeviceToHost); }
    const int rcode = e == hipSuccess ? 0 : fail(e, what);
    for (int k = 0; k < 5; ++k)
        if (dev[k]) (void)hipFree(dev[k]);
    return rcode;
}

}  // extern "C"
