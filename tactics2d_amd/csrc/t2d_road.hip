// t2d_road.hip -- Spiral and ParamPoly3 curves for a batch of parameter rows (spiral_curves_kernel, param_poly3_curves_kernel), the
// reference line of a batch of OpenDRIVE plan views (planview_kernel<false>) and the same chain writing fp32 vertices into the
// installed route sets (planview_kernel<true>, whose slot is t2d_route_write_dev.h's).  The formulas are t2d_road_dev.h; what they
// restate is interpolator/spiral.py, interpolator/param_poly3.py and map/parser/parse_xodr.py:256-474, 773-809.  DESIGN.md 4.20, 4.18a.
#include "t2d_pool.h"
#include "t2d_road_dev.h"
#include "t2d_route_write_dev.h"

namespace t2d {

static_assert(GEOM_LINE == T2D_GEOM_LINE && GEOM_SPIRAL == T2D_GEOM_SPIRAL && GEOM_ARC == T2D_GEOM_ARC && GEOM_POLY3 == T2D_GEOM_POLY3 &&
              GEOM_PARAM_POLY3 == T2D_GEOM_PARAM_POLY3, "t2d.h");
static_assert(SPIRAL_REFERENCE == T2D_SPIRAL_REFERENCE && SPIRAL_STANDARD == T2D_SPIRAL_STANDARD, "t2d.h");
static_assert(sizeof(PlanviewRecord) == T2D_PLANVIEW_RECORD_BYTES && kPlanviewMaxGeom == T2D_PLANVIEW_MAX_GEOM &&
              kPlanviewMaxRaw == T2D_PLANVIEW_MAX_RAW && kRoadsPerBlock == T2D_ROAD_CURVES_PER_BLOCK, "t2d.h");

namespace {

unsigned road_blocks(int n) { return (unsigned)(((long long)n + kRoadsPerBlock - 1) / kRoadsPerBlock); }

// ---- Spiral.get_curve / ParamPoly3.get_curve --------------------------------------------------------------------------------------
// One curve per wave, four per workgroup; point k belongs to lane k mod 64, so consecutive lanes store consecutive 16-byte points.
// The row's few parameters come in by wave-uniform loads; nothing is shared, so there is no barrier.
__global__ __launch_bounds__(kRoadBlock) void spiral_curves_kernel(int n, const double* __restrict__ par, int n_interp, int rule,
                                                                   int max_points, double2* __restrict__ xy, int32_t* __restrict__ count) {
    const int lane = threadIdx.x % kRoadWave, e = blockIdx.x * kRoadsPerBlock + threadIdx.x / kRoadWave;
    if (e >= n) return;
    const double* p = par + (size_t)e * 6;
    const double length = p[0], x0 = p[1], y0 = p[2], h = p[3], k0 = p[4], gamma = p[5];
    bool ok = length >= 0.0;
    for (int i = 0; i < 6; ++i) ok = ok && __builtin_isfinite(p[i]);
    if (lane == 0) count[e] = ok ? n_interp : 0;
    if (!ok) return;
    const int m = n_interp < max_points ? n_interp : max_points;
    double2* out = xy + (size_t)e * max_points;
    for (int k = lane; k < m; k += kRoadWave) {
        double x, y;
        spiral_point(length, x0, y0, h, k0, gamma, n_interp, k, rule, x, y);
        out[k] = make_double2(x, y);
    }
}

__global__ __launch_bounds__(kRoadBlock) void param_poly3_curves_kernel(int n, const double* __restrict__ par,
                                                                        const int32_t* __restrict__ p_range, int max_points,
                                                                        double2* __restrict__ xy, int32_t* __restrict__ count) {
    const int lane = threadIdx.x % kRoadWave, e = blockIdx.x * kRoadsPerBlock + threadIdx.x / kRoadWave;
    if (e >= n) return;
    const double* p = par + (size_t)e * 12;
    const int range = p_range[e];
    bool ok = p[0] >= 0.0 && (range == P_RANGE_NORMALIZED || range == P_RANGE_ARC_LENGTH);
    for (int i = 0; i < 12; ++i) ok = ok && __builtin_isfinite(p[i]);
    const int total = ok ? (int)tenth_count(p[0], 0.0, 2147483647.0) : 0;   // max(2, int(length / 0.1)), saturating
    if (lane == 0) count[e] = total;
    const int m = total < max_points ? total : max_points;
    double2* out = xy + (size_t)e * max_points;
    for (int k = lane; k < m; k += kRoadWave) {
        double x, y, kappa;
        param_poly3_point(p[0], p[1], p[2], p[3], p + 4, range == P_RANGE_ARC_LENGTH, total, k, x, y, kappa);
        out[k] = make_double2(x, y);
    }
}

// ---- the plan view ------------------------------------------------------------------------------------------------------------
// One road per wave, four per workgroup.  Lane g plans geometry g into the wave's RoadWork in LDS (count, pop, prefix sum by
// shuffles); after the one barrier the wave walks its road's raw points 64 per pass (road_walk): a ballot of the keep decisions,
// the population count below the lane and the running count of the road give every kept point its place.
//   ROUTES = false: kept point q -> xy / s / kappa [e][q], q < max_points; count = kept points, 0 where fewer than 2.
//   ROUTES = true:  kept points 0, stride, 2 stride, ... and the last one -> the fp32 vertices of route `route` of env e's set;
//                   count = the number of such vertices V; V < capacity: the rest repeats the last kept point; V > capacity: the
//                   first `capacity`.  The slot is route_slot's (t2d_route_write_dev.h); the strided store pattern is this kernel's.
template <bool ROUTES>
__global__ __launch_bounds__(kRoadBlock) void planview_kernel(RouteView rv, int n, const PlanviewRecord* __restrict__ rec,
                                                              const int32_t* __restrict__ n_geom, int max_geom, int rule, int stride,
                                                              int route, int max_points, double2* __restrict__ xy,
                                                              double* __restrict__ s_out, double* __restrict__ kappa_out,
                                                              int32_t* __restrict__ count) {
    __shared__ RoadWork s_work[kRoadsPerBlock];
    const int wave = threadIdx.x / kRoadWave, lane = threadIdx.x % kRoadWave;
    const int e = blockIdx.x * kRoadsPerBlock + wave;
    RoadWork& w = s_work[wave];
    if (e < n) road_plan(w, rec, n_geom, max_geom, e, rule, lane);
    __syncthreads();
    if (e >= n) return;
    RoadPoint head, tail;
    int kept = 0;
    if constexpr (ROUTES) {
        const RouteSlot slot = route_slot(rv, e, route);
        kept = road_walk(w, rule, lane, head, tail, [&](int q, const RoadPoint& p) {
            if (q % stride == 0 && q / stride < slot.cap) slot.out[q / stride] = make_float2((float)p.x, (float)p.y);
        });
        if (kept < 2) {
            if (lane == 0 && count) count[e] = 0;
            return;
        }
        const bool extra = (kept - 1) % stride != 0;          // the last kept point is not on the stride
        const int V = (kept - 1) / stride + 1 + (extra ? 1 : 0);
        const float2 last = make_float2((float)tail.x, (float)tail.y);
        if (lane == 0) {
            if (count) count[e] = V;
            if (slot.cap > 0) slot.out[0] = make_float2((float)head.x, (float)head.y);
            if (extra && V - 1 < slot.cap) slot.out[V - 1] = last;
        }
        for (int k = V + lane; k < slot.cap; k += kRoadWave) slot.out[k] = last;
    } else {
        double2* oxy = xy + (size_t)e * max_points;
        double* os = s_out ? s_out + (size_t)e * max_points : nullptr;
        double* ok = kappa_out ? kappa_out + (size_t)e * max_points : nullptr;
        auto put = [&](int q, const RoadPoint& p) {
            if (q >= max_points) return;
            oxy[q] = make_double2(p.x, p.y);
            if (os) os[q] = p.s;
            if (ok) ok[q] = p.kappa;
        };
        kept = road_walk(w, rule, lane, head, tail, put);
        if (kept >= 2 && lane == 0) put(0, head);
        if (lane == 0) count[e] = kept >= 2 ? kept : 0;
    }
}

}  // namespace

const char* planview_args_error(const void* rec, const int32_t* n_geom, int max_geom, int rule) {
    if (!rec || !n_geom || (reinterpret_cast<uintptr_t>(rec) & 7u) || (reinterpret_cast<uintptr_t>(n_geom) & 3u))
        return "null or misaligned rec_dev (8 bytes) / n_geom_dev (4 bytes)";
    if (max_geom < 1 || max_geom > kPlanviewMaxGeom) return "max_geom must be 1 .. T2D_PLANVIEW_MAX_GEOM";
    if (rule != SPIRAL_REFERENCE && rule != SPIRAL_STANDARD) return "rule must be T2D_SPIRAL_REFERENCE or T2D_SPIRAL_STANDARD";
    return nullptr;
}

hipError_t launch_planview_routes(const PoolView& v, const RouteView& rv, const void* rec, const int32_t* n_geom, int max_geom, int rule,
                                  int stride, int route, int32_t* count, hipStream_t s) {
    hipLaunchKernelGGL(planview_kernel<true>, dim3(road_blocks(v.n_env)), dim3(kRoadBlock), 0, s, rv, v.n_env,
                       static_cast<const PlanviewRecord*>(rec), n_geom, max_geom, rule, stride, route, 0, (double2*)nullptr,
                       (double*)nullptr, (double*)nullptr, count);
    return hipGetLastError();
}

}  // namespace t2d

extern "C" int t2d_spiral_curves(int32_t device_id, int32_t n, const double* par_dev, int32_t n_interpolation, int32_t rule,
                                 int32_t max_points, double* xy_dev, int32_t* count_dev, void* hip_stream) {
    using namespace t2d;
    if (n < 0 || max_points <= 0 || n_interpolation < 1 || (rule != SPIRAL_REFERENCE && rule != SPIRAL_STANDARD) || !par_dev || !xy_dev ||
        !count_dev || (reinterpret_cast<uintptr_t>(par_dev) & 7u) || (reinterpret_cast<uintptr_t>(xy_dev) & 15u) ||
        (reinterpret_cast<uintptr_t>(count_dev) & 3u))
        return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    hipLaunchKernelGGL(spiral_curves_kernel, dim3(road_blocks(n)), dim3(kRoadBlock), 0, (hipStream_t)hip_stream, n, par_dev,
                       n_interpolation, rule, max_points, reinterpret_cast<double2*>(xy_dev), count_dev);
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}

extern "C" int t2d_param_poly3_curves(int32_t device_id, int32_t n, const double* par_dev, const int32_t* p_range_dev, int32_t max_points,
                                      double* xy_dev, int32_t* count_dev, void* hip_stream) {
    using namespace t2d;
    if (n < 0 || max_points <= 0 || !par_dev || !p_range_dev || !xy_dev || !count_dev || (reinterpret_cast<uintptr_t>(par_dev) & 7u) ||
        (reinterpret_cast<uintptr_t>(p_range_dev) & 3u) || (reinterpret_cast<uintptr_t>(xy_dev) & 15u) ||
        (reinterpret_cast<uintptr_t>(count_dev) & 3u))
        return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    hipLaunchKernelGGL(param_poly3_curves_kernel, dim3(road_blocks(n)), dim3(kRoadBlock), 0, (hipStream_t)hip_stream, n, par_dev,
                       p_range_dev, max_points, reinterpret_cast<double2*>(xy_dev), count_dev);
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}

extern "C" int t2d_planview_lines(int32_t device_id, int32_t n, const void* rec_dev, const int32_t* n_geom_dev, int32_t max_geom,
                                  int32_t rule, int32_t max_points, double* xy_dev, double* s_dev, double* kappa_dev, int32_t* count_dev,
                                  void* hip_stream) {
    using namespace t2d;
    if (n < 0 || max_points <= 0 || planview_args_error(rec_dev, n_geom_dev, max_geom, rule) || !xy_dev || !count_dev ||
        (reinterpret_cast<uintptr_t>(xy_dev) & 15u) || (reinterpret_cast<uintptr_t>(s_dev) & 7u) ||
        (reinterpret_cast<uintptr_t>(kappa_dev) & 7u) || (reinterpret_cast<uintptr_t>(count_dev) & 3u))
        return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    hipLaunchKernelGGL(planview_kernel<false>, dim3(road_blocks(n)), dim3(kRoadBlock), 0, (hipStream_t)hip_stream, RouteView{}, n,
                       static_cast<const PlanviewRecord*>(rec_dev), n_geom_dev, max_geom, rule, 1, 0, max_points,
                       reinterpret_cast<double2*>(xy_dev), s_dev, kappa_dev, count_dev);
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}
