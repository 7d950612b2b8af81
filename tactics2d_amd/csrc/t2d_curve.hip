// t2d_curve.hip -- Dubins candidates for a batch of queries (dubins_paths_kernel), the sampled curve line of one Dubins or
// Reeds-Shepp word per curve (curve_lines_kernel), and the same sampler writing fp32 vertices into the installed route sets
// (curve_routes_kernel), whose slot and fill are t2d_route_write_dev.h.  The formulas are t2d_curve_dev.h; what they restate is
// interpolator/dubins.py, interpolator/reeds_shepp.py:46-139 and geometry/circle.py:106-139.  DESIGN.md 4.18, 4.18a.
#include "t2d_pool.h"
#include "t2d_curve_dev.h"
#include "t2d_route_write_dev.h"

namespace t2d {
namespace {

const int8_t kDubinsLettersHost[kDubinsSlots][3] = {T2D_DUBINS_SLOT_ROWS};

// ---- get_all_path / get_path for n independent queries ------------------------------------------------------------------------
// lane = query, all six words per lane: a word is two atan2 and a few mod 2 pi, and the six share the query's five sincos.
constexpr int kPathBlock = 256;

__global__ __launch_bounds__(kPathBlock) void dubins_paths_kernel(int n, double radius, const double* __restrict__ start,
                                                                  const double* __restrict__ goal, int lrl_rule,
                                                                  uint8_t* __restrict__ valid, double* __restrict__ segments,
                                                                  double* __restrict__ length, int32_t* __restrict__ shortest) {
    const long long q = (long long)blockIdx.x * kPathBlock + threadIdx.x;
    if (q >= n) return;
    const DubinsGoal g = dubins_normalise(start[3 * q], start[3 * q + 1], start[3 * q + 2], goal[3 * q], goal[3 * q + 1],
                                          goal[3 * q + 2], radius);
    const double inf = __builtin_inf();
    uint32_t mask = 0;
    int last = -1, first = -1;
    double best = inf;
#pragma unroll
    for (int s = 0; s < kDubinsSlots; ++s) {
        double t, p, u;
        const bool ok = dubins_slot(s, g, lrl_rule, t, p, u);
        const double len = ok ? ((__builtin_fabs(t) + __builtin_fabs(p)) + __builtin_fabs(u)) * radius : inf;
        double* o = segments + ((size_t)q * kDubinsSlots + s) * 3;
        o[0] = t;
        o[1] = p;
        o[2] = u;
        length[(size_t)q * kDubinsSlots + s] = len;
        if (ok) {
            mask |= 1u << s;
            if (first < 0 || len < best) first = s;
            if (!(len > best)) { last = s; best = len; }   // get_path :297-302: an equal length replaces the choice
        }
    }
    valid[q] = (uint8_t)mask;
    shortest[2 * q] = last;
    shortest[2 * q + 1] = first;
}

// ---- curve lines --------------------------------------------------------------------------------------------------------------
// One curve per workgroup of four waves.  Lane 0 walks the word (at most five segment start poses, a dozen sincos) and leaves the
// plan in LDS; then point k belongs to lane k mod 256, so consecutive lanes store consecutive points: 16 B of xy and 8 B of yaw
// each, whole cache lines per wave.  A curve of a few hundred points is one or two rounds.
constexpr int kCurveBlock = 256;

__global__ __launch_bounds__(kCurveBlock) void curve_lines_kernel(const CurveWord* __restrict__ words, const double* __restrict__ start,
                                                                  double radius, double step, int rule, int max_points,
                                                                  double2* __restrict__ xy, double* __restrict__ yaw,
                                                                  int32_t* __restrict__ count, double* __restrict__ end) {
    __shared__ CurvePlan s_plan;
    __shared__ long long s_total;
    const int e = blockIdx.x, tid = threadIdx.x;
    if (tid == 0) {
        long long total;
        const bool ok = curve_plan(words[e], start[3 * (size_t)e], start[3 * (size_t)e + 1], start[3 * (size_t)e + 2], radius, step,
                                   rule, s_plan, total);
        s_total = total;
        count[e] = point_count(total);
        if (ok) {
            end[3 * (size_t)e] = s_plan.end[0];
            end[3 * (size_t)e + 1] = s_plan.end[1];
            end[3 * (size_t)e + 2] = s_plan.end[2];
        }
    }
    __syncthreads();
    const long long total = s_total;
    const int n = total < (long long)max_points ? (int)total : max_points;
    double2* oxy = xy + (size_t)e * max_points;
    double* oyaw = yaw + (size_t)e * max_points;
    for (long long k = tid; k < n; k += kCurveBlock) {   // (64-bit: max_points may lie within a block of INT32_MAX)
        double x, y, h;
        curve_point(s_plan, radius, k, x, y, h);
        oxy[k] = make_double2(x, y);
        oyaw[k] = h;
    }
}

// The same sampler, curve e into route `route` of env e's own set (t2d_route_write_dev.h): the tail is the curve's end point; a
// curve without points leaves the route as it is.  The plan stage is curve_lines_kernel's without `end`, and stays written out
// in both: moved into a function the two call, the lines kernel came out 0.33 us slower.
__global__ __launch_bounds__(kCurveBlock) void curve_routes_kernel(RouteView rv, const CurveWord* __restrict__ words,
                                                                   const double* __restrict__ start, double radius, double step,
                                                                   int rule, int route, int32_t* __restrict__ count) {
    __shared__ CurvePlan s_plan;
    __shared__ long long s_total;
    const int e = blockIdx.x;
    if (threadIdx.x == 0) {
        long long total;
        curve_plan(words[e], start[3 * (size_t)e], start[3 * (size_t)e + 1], start[3 * (size_t)e + 2], radius, step, rule, s_plan,
                   total);
        s_total = total;
        if (count) count[e] = point_count(total);
    }
    __syncthreads();
    const long long total = s_total;
    if (total == 0) return;
    route_fill(route_slot(rv, e, route), threadIdx.x, kCurveBlock, total, make_float2((float)s_plan.end[0], (float)s_plan.end[1]),
               [&](int k, double& x, double& y) { double h; curve_point(s_plan, radius, k, x, y, h); });
}

// A polyline the caller already has (a planner's path) into route `route` of env e's own set: point k of the first
// min(counts[e], max_pts) rounded to fp32, the tail is the last of them.  A row without points, or with a coordinate among the ones
// it would write that is not finite as fp32, leaves the route as it is (count 0).
__global__ __launch_bounds__(kCurveBlock) void polyline_routes_kernel(RouteView rv, const double* __restrict__ points,
                                                                      const int32_t* __restrict__ counts, int max_pts, int cols,
                                                                      int route, int32_t* __restrict__ count) {
    const int e = blockIdx.x;
    const RouteSlot slot = route_slot(rv, e, route);
    const double* p = points + (size_t)e * (size_t)max_pts * (size_t)cols;
    const int given = counts[e], used = given < max_pts ? given : max_pts;
    const int written = used < slot.cap ? used : slot.cap;
    bool bad = false;
    for (int k = threadIdx.x; k < written; k += kCurveBlock) {
        const float x = (float)p[(size_t)k * cols], y = (float)p[(size_t)k * cols + 1];
        bad = bad || !(__builtin_fabsf(x) < __builtin_huge_valf()) || !(__builtin_fabsf(y) < __builtin_huge_valf());
    }
    const bool leave = __syncthreads_or(bad) || used <= 0;
    if (threadIdx.x == 0 && count) count[e] = leave ? 0 : used;
    if (leave) return;
    const double* last = p + (size_t)(used - 1) * cols;
    route_fill(slot, threadIdx.x, kCurveBlock, used, make_float2((float)last[0], (float)last[1]),
               [&](int k, double& x, double& y) { x = p[(size_t)k * cols]; y = p[(size_t)k * cols + 1]; });
}

}  // namespace

hipError_t launch_polyline_routes(const PoolView& v, const RouteView& rv, const double* points, const int32_t* counts, int max_pts,
                                  int cols, int route, int32_t* count, hipStream_t s) {
    hipLaunchKernelGGL(polyline_routes_kernel, dim3(v.n_env), dim3(kCurveBlock), 0, s, rv, points, counts, max_pts, cols, route, count);
    return hipGetLastError();
}

hipError_t launch_curve_routes(const PoolView& v, const RouteView& rv, const void* words, const double* start, double radius,
                               double step, int rule, int route, int32_t* count, hipStream_t s) {
    hipLaunchKernelGGL(curve_routes_kernel, dim3(v.n_env), dim3(kCurveBlock), 0, s, rv, static_cast<const CurveWord*>(words), start,
                       radius, step, rule, route, count);
    return hipGetLastError();
}

}  // namespace t2d

extern "C" int t2d_dubins_slot_info(int32_t slot, int8_t* letters) {
    using namespace t2d;
    if (slot < 0 || slot >= kDubinsSlots || !letters) return T2D_ERR_INVALID;
    for (int i = 0; i < 3; ++i) letters[i] = kDubinsLettersHost[slot][i];
    return T2D_OK;
}

extern "C" int t2d_dubins_paths(int32_t device_id, int32_t n, double radius, const double* start_dev, const double* goal_dev,
                                int32_t lrl_rule, uint8_t* valid_dev, double* segments_dev, double* length_dev, int32_t* shortest_dev,
                                void* hip_stream) {
    using namespace t2d;
    if (n < 0 || !(radius > 0.0) || !__builtin_isfinite(radius) || (lrl_rule != 0 && lrl_rule != 1) || !start_dev || !goal_dev ||
        !valid_dev || !segments_dev || !length_dev || !shortest_dev)
        return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    hipLaunchKernelGGL(dubins_paths_kernel, dim3((unsigned)(((long long)n + kPathBlock - 1) / kPathBlock)), dim3(kPathBlock), 0, (hipStream_t)hip_stream, n,
                       radius, start_dev, goal_dev, lrl_rule, valid_dev, segments_dev, length_dev, shortest_dev);
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}

extern "C" int t2d_curve_lines(int32_t device_id, int32_t n, const void* words_dev, const double* start_dev, double radius,
                               double step_size, int32_t rule, int32_t max_points, double* xy_dev, double* yaw_dev, int32_t* count_dev,
                               double* end_dev, void* hip_stream) {
    using namespace t2d;
    if (n < 0 || !(radius > 0.0) || !__builtin_isfinite(radius) || !(step_size > 0.0) || !__builtin_isfinite(step_size) ||
        max_points <= 0 || (rule != CURVE_RULE_DUBINS && rule != CURVE_RULE_RS) || !words_dev || !start_dev || !xy_dev || !yaw_dev ||
        !count_dev || !end_dev)
        return T2D_ERR_INVALID;
    if ((reinterpret_cast<uintptr_t>(words_dev) & 7u) || (reinterpret_cast<uintptr_t>(xy_dev) & 15u)) return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    hipLaunchKernelGGL(curve_lines_kernel, dim3(n), dim3(kCurveBlock), 0, (hipStream_t)hip_stream,
                       static_cast<const CurveWord*>(words_dev), start_dev, radius, step_size, rule, max_points,
                       reinterpret_cast<double2*>(xy_dev), yaw_dev, count_dev, end_dev);
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}
