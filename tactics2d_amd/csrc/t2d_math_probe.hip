// t2d_math_probe.hip -- t2d_debug_math (include/t2d_debug.h): one function of t2d_math.h evaluated over arrays on the device, so
// that tests/test_gpu_math.py can hold the device code itself -- not a kernel built on it -- against the oracle's restatement.
// Compiled with the product's flags (-ffp-contract=off is the point).  Element i is computed by lane i % 64 of wave i / 64
// (workgroups of 256 = 4 waves), and lanes past n leave before anything wave-level happens: a test decides which inputs
// share a wave with which, which is what the __ballot shortcuts of sincos_det_steer / sincos_det_steer_and depend on.
//
// This file is compiled twice.  As itself it holds the literal variant -- what every translation unit but t2d_collide.hip
// compiles -- and the C entry point.  t2d_math_probe_table.hip defines T2D_TRIG_TABLE and T2D_MATH_PROBE_TABLE and includes
// it: t2d_math.h then goes inside a namespace of its own (its __constant__ tables have external linkage in namespace t2d,
// where t2d_collide.hip already defines them), and only the launcher of the table variant comes out.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#ifdef T2D_MATH_PROBE_TABLE
namespace t2d_math_probe_table {
#include "t2d_math.h"
}
#define T2D_PROBE_MATH t2d_math_probe_table::t2d
#define T2D_PROBE_LAUNCH math_probe_launch_table
#else
#include "t2d_math.h"
#define T2D_PROBE_MATH t2d
#define T2D_PROBE_LAUNCH math_probe_launch_literal
#endif

#include "../../include/t2d_debug.h"

namespace t2d {
namespace probe {
namespace {   // (the two compilations of this file define different kernels of the same name: internal linkage)

// out is planar: output j of element i at out[j * n + i]
template <int FN>
__global__ __launch_bounds__(256) void math_probe_kernel(long long n, const double* __restrict__ a, const double* __restrict__ b,
                                                         double* __restrict__ out) {
    namespace M = T2D_PROBE_MATH;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x = a[i];
    if constexpr (FN == T2D_MATH_SINCOS) {
        double s, c;
        M::sincos_det(x, s, c);
        out[i] = s; out[n + i] = c;
    } else if constexpr (FN == T2D_MATH_SINCOS_SMALL) {
        double s, c;
        M::sincos_det_small(x, s, c);
        out[i] = s; out[n + i] = c;
    } else if constexpr (FN == T2D_MATH_SINCOS_STEER) {
        double s, c;
        M::sincos_det_steer(x, s, c);
        out[i] = s; out[n + i] = c;
    } else if constexpr (FN == T2D_MATH_SINCOS_STEER_AND) {
        double sa, ca, sb, cb;
        M::sincos_det_steer_and(x, b[i], sa, ca, sb, cb);
        out[i] = sa; out[n + i] = ca; out[2 * n + i] = sb; out[3 * n + i] = cb;
    } else if constexpr (FN == T2D_MATH_TAN) {
        out[i] = M::tan_det(x);
    } else if constexpr (FN == T2D_MATH_ATAN) {
        out[i] = M::atan_det(x);
    } else if constexpr (FN == T2D_MATH_ATAN2) {
        out[i] = M::atan2_det(x, b[i]);
#ifndef T2D_MATH_PROBE_TABLE
    } else if constexpr (FN == T2D_MATH_MOD_TWO_PI) {
        out[i] = M::mod_two_pi(x);
    } else if constexpr (FN == T2D_MATH_LOG) {
        out[i] = M::log_det(x);
    } else if constexpr (FN == T2D_MATH_EXP) {
        out[i] = M::exp_det(x);
    } else if constexpr (FN == T2D_MATH_POW) {
        out[i] = M::pow_det(x, b[i]);
    } else if constexpr (FN == T2D_MATH_FRESNEL) {
        double S, C;
        M::fresnel_det(x, S, C);
        out[i] = S; out[n + i] = C;
#endif
    }
}

template <int FN>
static hipError_t launch_one(long long n, const double* a, const double* b, double* out) {
    hipLaunchKernelGGL(math_probe_kernel<FN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, a, b, out);
    return hipGetLastError();
}

}  // namespace

// device pointers; fn was validated by the caller (for the table variant: a function that has one)
hipError_t T2D_PROBE_LAUNCH(int fn, long long n, const double* a, const double* b, double* out) {
    switch (fn) {
        case T2D_MATH_SINCOS: return launch_one<T2D_MATH_SINCOS>(n, a, b, out);
        case T2D_MATH_SINCOS_SMALL: return launch_one<T2D_MATH_SINCOS_SMALL>(n, a, b, out);
        case T2D_MATH_SINCOS_STEER: return launch_one<T2D_MATH_SINCOS_STEER>(n, a, b, out);
        case T2D_MATH_SINCOS_STEER_AND: return launch_one<T2D_MATH_SINCOS_STEER_AND>(n, a, b, out);
        case T2D_MATH_TAN: return launch_one<T2D_MATH_TAN>(n, a, b, out);
        case T2D_MATH_ATAN: return launch_one<T2D_MATH_ATAN>(n, a, b, out);
        case T2D_MATH_ATAN2: return launch_one<T2D_MATH_ATAN2>(n, a, b, out);
#ifndef T2D_MATH_PROBE_TABLE
        case T2D_MATH_MOD_TWO_PI: return launch_one<T2D_MATH_MOD_TWO_PI>(n, a, b, out);
        case T2D_MATH_LOG: return launch_one<T2D_MATH_LOG>(n, a, b, out);
        case T2D_MATH_EXP: return launch_one<T2D_MATH_EXP>(n, a, b, out);
        case T2D_MATH_POW: return launch_one<T2D_MATH_POW>(n, a, b, out);
        case T2D_MATH_FRESNEL: return launch_one<T2D_MATH_FRESNEL>(n, a, b, out);
#endif
        default: return hipErrorInvalidValue;
    }
}

#ifndef T2D_MATH_PROBE_TABLE
hipError_t math_probe_launch_table(int fn, long long n, const double* a, const double* b, double* out);
#endif

}  // namespace probe
}  // namespace t2d

#ifndef T2D_MATH_PROBE_TABLE
#include "t2d_host.h"

namespace {

int n_outputs(int fn) {
    switch (fn) {
        case T2D_MATH_SINCOS: case T2D_MATH_SINCOS_SMALL: case T2D_MATH_SINCOS_STEER: case T2D_MATH_FRESNEL: return 2;
        case T2D_MATH_SINCOS_STEER_AND: return 4;
        case T2D_MATH_TAN: case T2D_MATH_ATAN: case T2D_MATH_ATAN2: case T2D_MATH_MOD_TWO_PI: case T2D_MATH_LOG:
        case T2D_MATH_EXP: case T2D_MATH_POW: return 1;
        default: return 0;
    }
}
bool two_inputs(int fn) { return fn == T2D_MATH_SINCOS_STEER_AND || fn == T2D_MATH_ATAN2 || fn == T2D_MATH_POW; }
bool has_table_variant(int fn) { return fn >= T2D_MATH_SINCOS && fn <= T2D_MATH_ATAN2; }

}  // namespace

extern "C" int t2d_debug_math(int32_t device_id, int32_t fn, int32_t table, int64_t n, const double* a_host, const double* b_host,
                              double* out_host) {
    using t2d::host::fail;
    const int nout = n_outputs(fn);
    if (!nout) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_math: fn is not one of T2D_MATH_*");
    if (table != 0 && table != 1) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_math: table must be 0 or 1");
    if (table && !has_table_variant(fn))
        return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_math: this function has no T2D_TRIG_TABLE variant");
    if (n < 1 || n > T2D_MATH_MAX_N) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_math: n must be in [1, T2D_MATH_MAX_N]");
    if (!a_host || !out_host || (two_inputs(fn) && !b_host))
        return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_math: a null array");
    int n_dev = 0;
    T2D_HIP(nullptr, hipGetDeviceCount(&n_dev));
    if (device_id < 0 || device_id >= n_dev) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_math: no such device");
    T2D_HIP(nullptr, hipSetDevice(device_id));
    const size_t bytes = (size_t)n * sizeof(double);
    t2d::DevBuf<double> a, b, out;   // (freed on every way out)
    T2D_HIP(nullptr, a.alloc((size_t)n));
    T2D_HIP(nullptr, hipMemcpy(a, a_host, bytes, hipMemcpyHostToDevice));
    if (two_inputs(fn)) {
        T2D_HIP(nullptr, b.alloc((size_t)n));
        T2D_HIP(nullptr, hipMemcpy(b, b_host, bytes, hipMemcpyHostToDevice));
    }
    T2D_HIP(nullptr, out.alloc((size_t)n * nout));
    T2D_HIP(nullptr, hipMemset(out, 0xff, bytes * nout));   // (a NaN with a payload no function returns: an unwritten element shows)
    T2D_HIP(nullptr, table ? t2d::probe::math_probe_launch_table(fn, n, a, b, out)
                           : t2d::probe::math_probe_launch_literal(fn, n, a, b, out));
    T2D_HIP(nullptr, hipDeviceSynchronize());
    T2D_HIP(nullptr, hipMemcpy(out_host, out, bytes * nout, hipMemcpyDeviceToHost));
    return T2D_OK;
}
#endif
