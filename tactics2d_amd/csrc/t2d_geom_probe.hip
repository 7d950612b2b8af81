// t2d_geom_probe.hip -- t2d_debug_geom (include/t2d_debug.h): one predicate of t2d_geom_dev.h evaluated over arrays on the device,
// so that tests/test_gpu_geom.py can hold the device code itself -- not a kernel built on it -- against the oracle's restatement
// at contact, where the event kernels' random scenes practically never look.  Compiled with the product's flags
// (-ffp-contract=off is the point: the filters say fma where they mean it and nowhere else).  Element i is computed by lane
// i % 64 of wave i / 64 (workgroups of 256 = 4 waves); no function here is wave-level, the layout only fixes which inputs
// share a wave.  Inputs are fp64 -- vertices closer to each other than fp32 poses allow -- and PLANAR like the outputs:
// component j of element i at a[j * n + i].
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <math.h>

#include "t2d_geom_dev.h"
#include "../../include/t2d_debug.h"

namespace t2d {
namespace probe {
namespace {

T2D_DEV geom::Quad load_quad_planar(const double* __restrict__ p, long long n, long long i) {
    geom::Quad r;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        r.x[k] = p[(2 * k) * n + i];
        r.y[k] = p[(2 * k + 1) * n + i];
    }
    return r;
}

template <int FN>
__global__ __launch_bounds__(256) void geom_probe_kernel(long long n, const double* __restrict__ a, const double* __restrict__ b,
                                                         double* __restrict__ out) {
    namespace G = geom;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    if constexpr (FN == T2D_GEOM_SEG_DIST2) {
        out[i] = G::seg_dist2(a[i], a[n + i], a[2 * n + i], a[3 * n + i], a[4 * n + i], a[5 * n + i]);
    } else {
        const G::Quad A = load_quad_planar(a, n, i);
        if constexpr (FN == T2D_GEOM_POINT_IN_QUAD) {
            out[i] = G::point_in_quad(A, b[i], b[n + i]) ? 1.0 : 0.0;
        } else if constexpr (FN == T2D_GEOM_PIECE_MEETS_QUAD_INTERIOR) {
            out[i] = G::piece_meets_quad_interior(A, b[i], b[n + i], b[2 * n + i], b[3 * n + i]) ? 1.0 : 0.0;
        } else {
            const G::Quad B = load_quad_planar(b, n, i);
            if constexpr (FN == T2D_GEOM_SAT_QUADS) {
                out[i] = G::sat_quads(A, B) ? 1.0 : 0.0;
            } else if constexpr (FN == T2D_GEOM_RECT_PAIR_FILTER) {
                out[i] = (double)G::rect_pair_filter(A, B);
            } else if constexpr (FN == T2D_GEOM_RECT_VS_CONVEX_FILTER) {
                out[i] = (double)G::rect_vs_convex_filter(A, B);
            } else if constexpr (FN == T2D_GEOM_IOU_TERMS) {
                // the terms of quad_iou (t2d_collide.hip) in its order: A's edges clipped to closed B, B's edges to A with the
                // coincident pieces dropped, origin A[0]
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int k = (e + 1) & 3;
                    out[e * n + i] = G::clipped_edge_term(A.x[e], A.y[e], A.x[k], A.y[k], B, false, A.x[0], A.y[0]);
                    out[(4 + e) * n + i] = G::clipped_edge_term(B.x[e], B.y[e], B.x[k], B.y[k], A, true, A.x[0], A.y[0]);
                }
                out[8 * n + i] = G::quad_area2(A);
                out[9 * n + i] = G::quad_area2(B);
            }
        }
    }
}

template <int FN>
hipError_t launch_one(long long n, const double* a, const double* b, double* out) {
    hipLaunchKernelGGL(geom_probe_kernel<FN>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, a, b, out);
    return hipGetLastError();
}

hipError_t launch(int fn, long long n, const double* a, const double* b, double* out) {
    switch (fn) {
        case T2D_GEOM_SAT_QUADS: return launch_one<T2D_GEOM_SAT_QUADS>(n, a, b, out);
        case T2D_GEOM_RECT_PAIR_FILTER: return launch_one<T2D_GEOM_RECT_PAIR_FILTER>(n, a, b, out);
        case T2D_GEOM_RECT_VS_CONVEX_FILTER: return launch_one<T2D_GEOM_RECT_VS_CONVEX_FILTER>(n, a, b, out);
        case T2D_GEOM_POINT_IN_QUAD: return launch_one<T2D_GEOM_POINT_IN_QUAD>(n, a, b, out);
        case T2D_GEOM_SEG_DIST2: return launch_one<T2D_GEOM_SEG_DIST2>(n, a, b, out);
        case T2D_GEOM_PIECE_MEETS_QUAD_INTERIOR: return launch_one<T2D_GEOM_PIECE_MEETS_QUAD_INTERIOR>(n, a, b, out);
        case T2D_GEOM_IOU_TERMS: return launch_one<T2D_GEOM_IOU_TERMS>(n, a, b, out);
        default: return hipErrorInvalidValue;
    }
}

// doubles per element of a_host / b_host / out_host; 0 outputs = not a function
void widths(int fn, int& na, int& nb, int& nout) {
    na = 8; nb = 8; nout = 1;
    switch (fn) {
        case T2D_GEOM_SAT_QUADS: case T2D_GEOM_RECT_PAIR_FILTER: case T2D_GEOM_RECT_VS_CONVEX_FILTER: break;
        case T2D_GEOM_POINT_IN_QUAD: nb = 2; break;
        case T2D_GEOM_SEG_DIST2: na = 6; nb = 0; break;
        case T2D_GEOM_PIECE_MEETS_QUAD_INTERIOR: nb = 4; break;
        case T2D_GEOM_IOU_TERMS: nout = 10; break;
        default: nout = 0; break;
    }
}

}  // namespace
}  // namespace probe
}  // namespace t2d

#include "t2d_host.h"

extern "C" int t2d_debug_geom(int32_t device_id, int32_t fn, int64_t n, const double* a_host, const double* b_host, double* out_host) {
    using t2d::host::fail;
    int na, nb, nout;
    t2d::probe::widths(fn, na, nb, nout);
    if (!nout) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_geom: fn is not one of T2D_GEOM_*");
    if (n < 1 || n > T2D_GEOM_MAX_N) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_geom: n must be in [1, T2D_GEOM_MAX_N]");
    if (!a_host || !out_host || (nb && !b_host)) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_geom: a null array");
    int n_dev = 0;
    T2D_HIP(nullptr, hipGetDeviceCount(&n_dev));
    if (device_id < 0 || device_id >= n_dev) return fail(nullptr, T2D_ERR_INVALID, "t2d_debug_geom: no such device");
    T2D_HIP(nullptr, hipSetDevice(device_id));
    const size_t bytes = (size_t)n * sizeof(double);
    t2d::DevBuf<double> a, b, out;   // (freed on every way out)
    T2D_HIP(nullptr, a.alloc((size_t)n * na));
    T2D_HIP(nullptr, hipMemcpy(a, a_host, bytes * na, hipMemcpyHostToDevice));
    if (nb) {
        T2D_HIP(nullptr, b.alloc((size_t)n * nb));
        T2D_HIP(nullptr, hipMemcpy(b, b_host, bytes * nb, hipMemcpyHostToDevice));
    }
    T2D_HIP(nullptr, out.alloc((size_t)n * nout));
    T2D_HIP(nullptr, hipMemset(out, 0xff, bytes * nout));   // (a NaN with a payload no function returns: an unwritten element shows)
    T2D_HIP(nullptr, t2d::probe::launch(fn, n, a, b, out));
    T2D_HIP(nullptr, hipDeviceSynchronize());
    T2D_HIP(nullptr, hipMemcpy(out_host, out, bytes * nout, hipMemcpyDeviceToHost));
    return T2D_OK;
}
