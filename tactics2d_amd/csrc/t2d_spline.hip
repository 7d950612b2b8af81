// t2d_spline.hip -- Bezier, B-spline and cubic spline curves for a batch of control polygons (spline_curves_kernel) and the same
// sampler writing fp32 vertices into the installed route sets (spline_routes_kernel); the two share their prologue
// (spline_prologue) and the kind -> instantiation choice (for_spline_kind), and the route form's slot and fill are
// t2d_route_write_dev.h.  The formulas are t2d_spline_dev.h; what they restate is
// interpolator/cpp_interpolator/src/{bezier,b_spline,cubic_spline}.cpp.  DESIGN.md 4.19, 4.18a.
#include <type_traits>

#include "t2d_pool.h"
#include "t2d_spline_dev.h"
#include "t2d_route_write_dev.h"

namespace t2d {

static_assert(SPLINE_BEZIER == T2D_SPLINE_BEZIER && SPLINE_BSPLINE == T2D_SPLINE_BSPLINE && SPLINE_CUBIC == T2D_SPLINE_CUBIC, "t2d.h");
static_assert(SPLINE_NATURAL == T2D_SPLINE_NATURAL && SPLINE_CLAMPED == T2D_SPLINE_CLAMPED && SPLINE_NOT_A_KNOT == T2D_SPLINE_NOT_A_KNOT, "t2d.h");
static_assert(kSplineMaxCtrl == T2D_SPLINE_MAX_CTRL && kSplineMaxDegree == T2D_SPLINE_MAX_DEGREE, "t2d.h");

namespace {

// One curve per wave, four curves per workgroup.  The wave's lanes load the row into its own SplineWork in LDS (10 KB for a cubic
// spline: the not-a-knot matrix is 33 x 33), lane 0 does the serial set-up, then point k belongs to lane k mod 64: consecutive
// lanes store consecutive 16-byte points, whole cache lines per wave.  A wave past the batch's end only keeps the barriers.
constexpr int kSplineWave = 64, kSplineCurvesPerBlock = T2D_SPLINE_CURVES_PER_BLOCK, kSplineBlock = kSplineWave * kSplineCurvesPerBlock;

// What both kernels start with: the wave's lanes load row e, lane 0 sets the curve up and reports its count (ROUTES: count may be
// null), then w.total is the number of points of the whole curve.  A wave past the batch's end passes both barriers and is told so.
template <bool ROUTES, int KIND>
T2D_DEV bool spline_prologue(SplineWork<KIND>& w, const SplineArgs& a, int n, int e, int lane, int32_t* count) {
    if (e < n) spline_load(w, a, e, lane);
    __syncthreads();
    if (e < n && lane == 0) {
        spline_setup(w, a, e);
        if (!ROUTES || count) count[e] = point_count(w.total);
    }
    __syncthreads();
    return e < n;
}

template <int KIND>
__global__ __launch_bounds__(kSplineBlock) void spline_curves_kernel(SplineArgs a, int n, int max_points, double2* __restrict__ xy,
                                                                     int32_t* __restrict__ count) {
    __shared__ SplineWork<KIND> s_work[kSplineCurvesPerBlock];
    const int wave = threadIdx.x / kSplineWave, lane = threadIdx.x % kSplineWave;
    const int e = blockIdx.x * kSplineCurvesPerBlock + wave;
    SplineWork<KIND>& w = s_work[wave];
    if (!spline_prologue<false>(w, a, n, e, lane, count)) return;
    const long long total = w.total;
    const int m = total < (long long)max_points ? (int)total : max_points;
    double2* out = xy + (size_t)e * max_points;
    for (int k = lane; k < m; k += kSplineWave) {
        double x, y;
        spline_point(w, a, k, x, y);
        out[k] = make_double2(x, y);
    }
}

// The same sampler, curve e into route `route` of env e's own set (t2d_route_write_dev.h): the tail is the curve's last point (for
// a B-spline its last SAMPLE), computed only where the route is longer than the curve; a row without a curve leaves the route as
// it is.
template <int KIND>
__global__ __launch_bounds__(kSplineBlock) void spline_routes_kernel(RouteView rv, SplineArgs a, int n, int route,
                                                                     int32_t* __restrict__ count) {
    __shared__ SplineWork<KIND> s_work[kSplineCurvesPerBlock];
    const int wave = threadIdx.x / kSplineWave, lane = threadIdx.x % kSplineWave;
    const int e = blockIdx.x * kSplineCurvesPerBlock + wave;
    SplineWork<KIND>& w = s_work[wave];
    if (!spline_prologue<true>(w, a, n, e, lane, count)) return;
    const long long total = w.total;
    if (total == 0) return;
    const RouteSlot slot = route_slot(rv, e, route);
    auto point = [&](long long k, double& x, double& y) { spline_point(w, a, k, x, y); };
    float2 tail = make_float2(0.f, 0.f);
    if (total < slot.cap) {
        double x, y;
        point(total - 1, x, y);
        tail = make_float2((float)x, (float)y);
    }
    route_fill(slot, lane, kSplineWave, total, tail, point);
}

// the kernel instantiation of a kind that spline_args_error has passed: f(std::integral_constant<int, KIND>)
template <class F>
void for_spline_kind(int kind, F f) {
    if (kind == SPLINE_BEZIER) f(std::integral_constant<int, SPLINE_BEZIER>{});
    else if (kind == SPLINE_BSPLINE) f(std::integral_constant<int, SPLINE_BSPLINE>{});
    else f(std::integral_constant<int, SPLINE_CUBIC>{});
}

SplineArgs spline_args(const double* ctrl, const int32_t* n_ctrl, int max_ctrl, int n_interp, int degree, const double* knots,
                       int boundary, const double* derivs) {
    return SplineArgs{reinterpret_cast<const double2*>(ctrl), n_ctrl, knots, derivs, max_ctrl, n_interp, degree, boundary};
}

unsigned spline_blocks(int n) { return (unsigned)(((long long)n + kSplineCurvesPerBlock - 1) / kSplineCurvesPerBlock); }

}  // namespace

const char* spline_args_error(int kind, const double* ctrl, const int32_t* n_ctrl, int max_ctrl, int n_interp, int degree,
                              const double* knots, int boundary, const double* derivs) {
    if (kind != SPLINE_BEZIER && kind != SPLINE_BSPLINE && kind != SPLINE_CUBIC)
        return "kind must be T2D_SPLINE_BEZIER, T2D_SPLINE_BSPLINE or T2D_SPLINE_CUBIC";
    if (!ctrl || !n_ctrl || (reinterpret_cast<uintptr_t>(ctrl) & 15u) || (reinterpret_cast<uintptr_t>(n_ctrl) & 3u))
        return "null or misaligned ctrl_dev (16 bytes) / n_ctrl_dev (4 bytes)";
    if (max_ctrl < 1 || max_ctrl > kSplineMaxCtrl) return "max_ctrl must be 1 .. T2D_SPLINE_MAX_CTRL";
    if (n_interp < (kind == SPLINE_BSPLINE ? 1 : 2))
        return "n_interpolation is below the family's minimum (Bezier 2, B-spline 1, cubic 2)";
    if (kind == SPLINE_BSPLINE) {
        if (degree < 0 || degree > kSplineMaxDegree) return "degree must be 0 .. T2D_SPLINE_MAX_DEGREE";
        if (reinterpret_cast<uintptr_t>(knots) & 7u) return "misaligned knots_dev (8 bytes)";
    }
    if (kind == SPLINE_CUBIC) {
        if (boundary != SPLINE_NATURAL && boundary != SPLINE_CLAMPED && boundary != SPLINE_NOT_A_KNOT)
            return "boundary_type must be T2D_SPLINE_NATURAL, T2D_SPLINE_CLAMPED or T2D_SPLINE_NOT_A_KNOT";
        if (reinterpret_cast<uintptr_t>(derivs) & 7u) return "misaligned derivs_dev (8 bytes)";
    }
    return nullptr;
}

hipError_t launch_spline_routes(const PoolView& v, const RouteView& rv, int kind, const double* ctrl, const int32_t* n_ctrl,
                                int max_ctrl, int n_interp, int degree, const double* knots, int boundary, const double* derivs,
                                int route, int32_t* count, hipStream_t s) {
    const SplineArgs a = spline_args(ctrl, n_ctrl, max_ctrl, n_interp, degree, knots, boundary, derivs);
    for_spline_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(spline_routes_kernel<decltype(k)::value>, dim3(spline_blocks(v.n_env)), dim3(kSplineBlock), 0, s, rv, a, v.n_env, route, count);
    });
    return hipGetLastError();
}

}  // namespace t2d

extern "C" int t2d_spline_curves(int32_t device_id, int32_t n, int32_t kind, const double* ctrl_dev, const int32_t* n_ctrl_dev,
                                 int32_t max_ctrl, int32_t n_interpolation, int32_t degree, const double* knots_dev,
                                 int32_t boundary_type, const double* derivs_dev, int32_t max_points, double* xy_dev,
                                 int32_t* count_dev, void* hip_stream) {
    using namespace t2d;
    if (n < 0 || max_points <= 0 || !xy_dev || !count_dev || (reinterpret_cast<uintptr_t>(xy_dev) & 15u) ||
        (reinterpret_cast<uintptr_t>(count_dev) & 3u) ||
        spline_args_error(kind, ctrl_dev, n_ctrl_dev, max_ctrl, n_interpolation, degree, knots_dev, boundary_type, derivs_dev))
        return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    const SplineArgs a = spline_args(ctrl_dev, n_ctrl_dev, max_ctrl, n_interpolation, degree, knots_dev, boundary_type, derivs_dev);
    for_spline_kind(kind, [&](auto k) {
        hipLaunchKernelGGL(spline_curves_kernel<decltype(k)::value>, dim3(spline_blocks(n)), dim3(kSplineBlock), 0, (hipStream_t)hip_stream, a, n,
                           max_points, reinterpret_cast<double2*>(xy_dev), count_dev);
    });
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}
