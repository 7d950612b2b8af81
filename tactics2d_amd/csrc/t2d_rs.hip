// t2d_rs.hip -- Reeds-Shepp candidates for a batch of queries (rs_paths_kernel) and the parking tutorial's collision-checked
// choice among them for every env of a pool (rs_plan_kernel).  The curve family is t2d_rs_dev.h; what the planner restates is
// docs/tutorial/train_parking_demo.ipynb cell 9 (RSPlanner.get_rs_path, construct_obstacles, is_traj_valid).  DESIGN.md 4.15.
#include "t2d_pool.h"
#include "t2d_rs_dev.h"

namespace t2d {
namespace {

__constant__ RsSlot kSlots[kRsSlots] = {T2D_RS_SLOT_ROWS};
const RsSlot kSlotsHost[kRsSlots] = {T2D_RS_SLOT_ROWS};

// ---- get_all_path / get_path for n independent queries ------------------------------------------------------------------------
// A workgroup of four waves takes 64 queries: lane = query, and every wave walks through twelve consecutive slots, so a wave
// is in ONE family's formula at a time (the five families share almost no code) and reads the slot's constants as scalars.
// The goal is normalised by each wave for itself (two sincos) rather than handed over through LDS.  Lengths meet in LDS,
// where wave 0 takes the two minima of each query in slot order.
constexpr int kPathQueries = 64, kPathWaves = 4, kSlotsPerWave = kRsSlots / kPathWaves;

__global__ __launch_bounds__(kPathQueries* kPathWaves) void rs_paths_kernel(int n, double radius, const double* __restrict__ start,
                                                                            const double* __restrict__ goal, uint64_t* __restrict__ valid,
                                                                            double* __restrict__ segments, double* __restrict__ length,
                                                                            int32_t* __restrict__ shortest) {
    __shared__ double s_len[kRsSlots][kPathQueries];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long q = (long long)blockIdx.x * kPathQueries + lane;
    const bool in = q < n;
    RsGoal g{};
    if (in) g = rs_normalise(start[3 * q], start[3 * q + 1], start[3 * q + 2], goal[3 * q], goal[3 * q + 1], goal[3 * q + 2], radius);
    const double inf = __builtin_inf();
    for (int k = 0; k < kSlotsPerWave; ++k) {
        const int s = wave * kSlotsPerWave + k;
        double seg[kRsMaxSeg], sum;
        const bool ok = in && rs_slot(kSlots[s], g, seg, sum);
        const double len = ok ? sum * radius : inf;
        s_len[s][lane] = len;
        if (in) {
            double* o = segments + ((size_t)q * kRsSlots + s) * kRsMaxSeg;
#pragma unroll
            for (int i = 0; i < kRsMaxSeg; ++i) o[i] = seg[i];
            length[(size_t)q * kRsSlots + s] = len;
        }
    }
    __syncthreads();
    if (wave == 0 && in) {
        uint64_t mask = 0;
        int last = -1, first = -1;
        double best = inf;
        for (int s = 0; s < kRsSlots; ++s) {
            const double len = s_len[s][lane];
            if (len == inf) continue;
            mask |= 1ull << s;
            if (first < 0 || len < best) first = s;        // RSPlanner's heap of (length, index): the lowest index of the shortest
            if (!(len > best)) { last = s; best = len; }   // get_path :551-556: an equal length replaces the choice
        }
        valid[q] = mask;
        shortest[2 * q] = last;
        shortest[2 * q + 1] = first;
    }
}

// ---- the planner --------------------------------------------------------------------------------------------------------------
// One env per workgroup of four waves.  The work of an env is one candidate set (48 lanes, once), one obstacle chain of
// n_beams edges that every later phase reads -- so it lives in LDS, 56 bytes an edge -- and then, per visited candidate, up
// to T2D_RS_MAX_POSES x 4 box edges against that chain: a few hundred thousand predicates that want all 256 lanes, with a
// workgroup-wide OR after every 256 (pose, box edge) pairs so that the first hit ends the candidate.  A wave per env would
// leave the chain in LDS four times per CU slot and the sweep a quarter of the lanes.
constexpr int kPlanBlock = 256;
struct RsEdge {
    double d, e, f;                 // the edge's line d x + e y + f = 0 (cell 9 :234-236)
    double xlo, xhi, ylo, yhi;      // its coordinate ranges widened by the edge tolerance (:249-252)
};
static_assert(sizeof(RsEdge) == 56, "LDS budget of the chain");

struct RsBoxEdge {
    double a, b, c, xlo, xhi, ylo, yhi;
};
// edge `k` of the vehicle box (rear-axle frame: x in center_shift -+ half_length, y in -+ half_width) at the pose
// (px, py, yaw given as sin / cos): cell 9 :199-230, 254-257
T2D_DEV RsBoxEdge rs_box_edge(const t2d_rs_params& c, double px, double py, double sy, double cy, int k) {
    const double x0 = (k == 0 || k == 3 ? c.half_length : -c.half_length) + c.center_shift;
    const double y0 = k < 2 ? -c.half_width : c.half_width;
    const int k1 = (k + 1) & 3;
    const double x1 = (k1 == 0 || k1 == 3 ? c.half_length : -c.half_length) + c.center_shift;
    const double y1 = k1 < 2 ? -c.half_width : c.half_width;
    const double vx1 = cy * x0 - sy * y0 + px, vy1 = sy * x0 + cy * y0 + py;
    const double vx2 = cy * x1 - sy * y1 + px, vy2 = sy * x1 + cy * y1 + py;
    RsBoxEdge r;
    r.a = vy2 - vy1;
    r.b = vx1 - vx2;
    r.c = vy1 * vx2 - vx1 * vy2;
    r.xlo = fmin(vx1, vx2) - c.edge_tolerance;
    r.xhi = fmax(vx1, vx2) + c.edge_tolerance;
    r.ylo = fmin(vy1, vy2) - c.edge_tolerance;
    r.yhi = fmax(vy1, vy2) + c.edge_tolerance;
    return r;
}
// is_traj_valid's verdict for one (box edge, obstacle edge) pair (:239-260).  An intersection point inside both edges' ranges
// needs the ranges to overlap: that test comes first and skips the two divisions, with the same verdict.
T2D_DEV bool rs_edges_hit(const RsBoxEdge& v, const RsEdge& o) {
    if (o.xlo > v.xhi || v.xlo > o.xhi || o.ylo > v.yhi || v.ylo > o.yhi) return false;
    const double det = v.a * o.e - v.b * o.d;
    if (det == 0.0) return false;
    const double rx = (v.b * o.f - v.c * o.e) / det, ry = (v.c * o.d - v.a * o.f) / det;
    return !(rx > o.xhi) && !(rx < o.xlo) && !(ry > o.yhi) && !(ry < o.ylo) && !(rx > v.xhi) && !(rx < v.xlo) && !(ry > v.yhi) &&
           !(ry < v.ylo);
}

// point k of the chain (construct_obstacles :160-168), all in fp64 from the fp32 scan value; nan = the value is a NaN
T2D_DEV void rs_chain_point(const RsPlanView& rv, const float* scan, int k, double& x, double& y, bool& nan) {
    double v = (double)scan[k];
    nan = v != v;
    v = v < 0.0 ? 0.0 : v;                         // np.clip(lidar_obs, 0.0, lidar_range): +inf becomes the range
    v = v > rv.lidar_range ? rv.lidar_range : v;
    const double base = rv.beam_tab[3 * k + 2], w = v - rv.cfg.distance_tolerance;
    const double dist = base > w ? base : w;       // np.maximum(vehicle_base, lidar_obs - distance_tolerance)
    x = rv.beam_tab[3 * k] * dist + rv.cfg.center_shift;
    y = rv.beam_tab[3 * k + 1] * dist;
}

T2D_DEV void rs_store_record(t2d_rs_plan_record* out, int status, int slot, int n_visited, double length, double shortest,
                             const RsSlot* sl, const double* seg, double radius) {
    t2d_rs_plan_record r;
    r.status = status;
    r.slot = slot;
    r.n_seg = sl ? sl->n_seg : 0;
    r.n_visited = n_visited;
    for (int i = 0; i < T2D_RS_MAX_SEGMENTS; ++i) {
        r.steer[i] = sl && i < sl->n_seg ? sl->letter[i] : 0;
        r.distance[i] = sl && i < sl->n_seg ? seg[i] * radius : 0.0;
    }
    r.reserved = 0;
    r.length = length;
    r.shortest = shortest;
    *out = r;
}

__global__ __launch_bounds__(kPlanBlock) void rs_plan_kernel(PoolView pv, RsPlanView rv, const float* __restrict__ scan_all,
                                                             t2d_rs_plan_record* __restrict__ out_all) {
    extern __shared__ double s_dyn[];
    RsEdge* s_edge = reinterpret_cast<RsEdge*>(s_dyn);
    __shared__ double s_seg[kRsSlots][kRsMaxSeg];
    __shared__ double s_len[kRsSlots];
    __shared__ int s_order[kRsSlots];
    __shared__ double s_start[kRsMaxSeg][3];
    __shared__ int s_first[kRsMaxSeg + 1];
    __shared__ int s_n_edge;
    const int e = blockIdx.x, tid = threadIdx.x;
    const t2d_rs_params& c = rv.cfg;
    t2d_rs_plan_record* out = out_all + e;
    const double nan_v = __builtin_nan(""), inf = __builtin_inf();

    // 1. the ego's pose and the target: centre of the four vertices (get_rs_path :54-58), everything wave-uniform
    const int ie = e * pv.A + rv.ego_index;
    const double ex0 = (double)pv.x[ie], ey0 = (double)pv.y[ie], eh = (double)pv.heading[ie];
    const bool active = ((pv.ids[ie] >> kIdsActiveShift) & 0xffu) != 0;
    double q[8];
    for (int k = 0; k < 8; ++k) q[k] = rv.target_quads ? (double)rv.target_quads[8 * (size_t)e + k] : rv.target_xy[8 * (size_t)e + k];
    double tx = (((q[0] + q[2]) + q[4]) + q[6]) / 4.0, ty = (((q[1] + q[3]) + q[5]) + q[7]) / 4.0;
    const double th = rv.target_heading[e];
    if (!(active && __builtin_isfinite(ex0) && __builtin_isfinite(ey0) && __builtin_isfinite(eh) && __builtin_isfinite(tx) &&
          __builtin_isfinite(ty) && __builtin_isfinite(th))) {
        if (tid == 0) rs_store_record(out, T2D_RS_NO_TARGET, -1, 0, nan_v, nan_v, nullptr, nullptr, c.radius);
        return;
    }
    // 2. both poses to the rear axle (:61-65), the far cut (:70-72), the goal in the ego's frame (:74-80)
    double se, ce, st, ct;
    sincos_det(eh, se, ce);
    sincos_det(th, st, ct);
    tx -= c.center_shift * ct;
    ty -= c.center_shift * st;
    const double ex = ex0 - c.center_shift * ce, ey = ey0 - c.center_shift * se;
    const double ddx = tx - ex, ddy = ty - ey;
    const double rel = __builtin_sqrt(ddx * ddx + ddy * ddy);
    if (rel > c.threshold_distance) {
        if (tid == 0) rs_store_record(out, T2D_RS_FAR, -1, 0, nan_v, nan_v, nullptr, nullptr, c.radius);
        return;
    }
    const double rel_angle = atan2_det(ddy, ddx) - eh;
    double sa, ca;
    sincos_det(rel_angle, sa, ca);
    const double gx = rel * ca, gy = rel * sa, gyaw = th - eh;
    RsGoal g;
    g.x = gx / c.radius;
    g.y = gy / c.radius;
    g.phi = gyaw;
    sincos_det(gyaw, g.s, g.c);
    g.finite = true;
    if (tid == 0) s_n_edge = 0;
    bool valid = false;
    if (tid < kRsSlots) {
        double seg[kRsMaxSeg], sum;
        valid = rs_slot(kSlots[tid], g, seg, sum);
        for (int i = 0; i < kRsMaxSeg; ++i) s_seg[tid][i] = seg[i];
        s_len[tid] = valid ? sum * c.radius : inf;
    }
    const int n_valid = __syncthreads_count(valid);
    if (valid) {   // rank by (length, slot): what popping RSPlanner's heap gives (:96-108)
        const double mine = s_len[tid];
        int rank = 0;
        for (int j = 0; j < kRsSlots; ++j) {
            const double l = s_len[j];
            rank += (l < mine || (l == mine && j < tid)) ? 1 : 0;
        }
        s_order[rank] = tid;
    }
    // 3. the obstacle chain (construct_obstacles :155-193): edge k joins points k and k + 1 (the last one closes the chain);
    // an edge that touches the box at the goal pose is left out
    const float* scan = scan_all + (size_t)e * rv.n_beams;
    bool any_nan = false;
    for (int k = tid; k < rv.n_beams; k += kPlanBlock) {
        double x1, y1, x2, y2;
        bool n1, n2;
        rs_chain_point(rv, scan, k, x1, y1, n1);
        rs_chain_point(rv, scan, k + 1 == rv.n_beams ? 0 : k + 1, x2, y2, n2);
        any_nan |= n1 | n2;
        RsEdge o;
        o.d = y2 - y1;
        o.e = x1 - x2;
        o.f = y1 * x2 - x1 * y2;
        o.xlo = fmin(x1, x2) - c.edge_tolerance;
        o.xhi = fmax(x1, x2) + c.edge_tolerance;
        o.ylo = fmin(y1, y2) - c.edge_tolerance;
        o.yhi = fmax(y1, y2) + c.edge_tolerance;
        bool touch = false;
        for (int b = 0; b < 4; ++b) touch |= rs_edges_hit(rs_box_edge(c, gx, gy, g.s, g.c, b), o);
        if (!touch && !(n1 | n2)) s_edge[atomicAdd(&s_n_edge, 1)] = o;   // (any order: the sweep asks whether ANY edge is hit)
    }
    any_nan = __syncthreads_or(any_nan) != 0;
    if (n_valid == 0) {   // (never seen: some CSC slot always exists)
        if (tid == 0) rs_store_record(out, T2D_RS_NONE_FREE, -1, 0, nan_v, nan_v, nullptr, nullptr, c.radius);
        return;
    }
    const double shortest = s_len[s_order[0]];
    if (any_nan) {
        if (tid == 0) rs_store_record(out, T2D_RS_UNCHECKED, -1, 0, nan_v, shortest, nullptr, nullptr, c.radius);
        return;
    }
    const int n_edge = s_n_edge;
    // 4. candidates in rank order up to length_ratio x the shortest (:105-119); the first without a hit is the plan
    int visited = 0;
    for (int r = 0; r < n_valid; ++r) {
        const int slot = s_order[r];
        const double len = s_len[slot];
        if (len > c.length_ratio * shortest) break;
        const RsSlot& sl = kSlots[slot];
        // poses of segment i: arc length k * sample_step, k = 0 .. ceil(|d_i| / sample_step), the last one at the segment's end
        int total = 0;
        for (int i = 0; i < sl.n_seg; ++i) {
            const double d = __builtin_fabs(s_seg[slot][i]) * c.radius;
            const double cnt = __builtin_ceil(d / c.sample_step) + 1.0;
            total = cnt > (double)(T2D_RS_MAX_POSES + 1) || total > T2D_RS_MAX_POSES ? T2D_RS_MAX_POSES + 1 : total + (int)cnt;
        }
        if (total > T2D_RS_MAX_POSES) {
            if (tid == 0) rs_store_record(out, T2D_RS_UNCHECKED, slot, r + 1, len, shortest, &sl, s_seg[slot], c.radius);
            return;
        }
        if (tid == 0) {
            double x = 0.0, y = 0.0, yaw = 0.0;
            int first = 0;
            for (int i = 0; i < sl.n_seg; ++i) {
                s_start[i][0] = x; s_start[i][1] = y; s_start[i][2] = yaw;
                s_first[i] = first;
                const double d = s_seg[slot][i] * c.radius;
                first += (int)__builtin_ceil(__builtin_fabs(d) / c.sample_step) + 1;
                rs_advance(x, y, yaw, sl.letter[i], d, c.radius);
            }
            s_first[sl.n_seg] = first;
        }
        __syncthreads();
        bool hit_any = false;
        for (int base = 0; base < 4 * total; base += kPlanBlock) {
            const int item = base + tid;
            bool hit = false;
            if (item < 4 * total) {
                const int p = item >> 2;
                int i = 0;
                while (i + 1 < sl.n_seg && p >= s_first[i + 1]) ++i;
                const double d = s_seg[slot][i] * c.radius, ad = __builtin_fabs(d);
                double arc = (double)(p - s_first[i]) * c.sample_step;
                arc = arc > ad ? ad : arc;
                double x = s_start[i][0], y = s_start[i][1], yaw = s_start[i][2];
                rs_advance(x, y, yaw, sl.letter[i], d < 0.0 ? -arc : arc, c.radius);
                double sy, cy;
                sincos_det(yaw, sy, cy);
                const RsBoxEdge v = rs_box_edge(c, x, y, sy, cy, item & 3);
                for (int j = 0; j < n_edge && !hit; ++j) hit = rs_edges_hit(v, s_edge[j]);
            }
            if (__syncthreads_or(hit)) {
                hit_any = true;
                break;
            }
        }
        if (!hit_any) {
            if (tid == 0) rs_store_record(out, T2D_RS_FOUND, slot, r + 1, len, shortest, &sl, s_seg[slot], c.radius);
            return;
        }
        visited = r + 1;
    }
    if (tid == 0) rs_store_record(out, T2D_RS_NONE_FREE, -1, visited, nan_v, shortest, nullptr, nullptr, c.radius);
}

}  // namespace

hipError_t launch_rs_plan(const PoolView& v, const RsPlanView& rv, const float* scan, t2d_rs_plan_record* out, hipStream_t s) {
    hipLaunchKernelGGL(rs_plan_kernel, dim3(v.n_env), dim3(kPlanBlock), (size_t)rv.n_beams * sizeof(RsEdge), s, v, rv, scan, out);
    return hipGetLastError();
}

}  // namespace t2d

extern "C" int t2d_rs_slot_info(int32_t slot, int8_t* letters, int8_t* signs, int32_t* n_seg, int32_t* curve_type) {
    using namespace t2d;
    if (slot < 0 || slot >= kRsSlots || !letters || !signs || !n_seg || !curve_type) return T2D_ERR_INVALID;
    const RsSlot& sl = kSlotsHost[slot];
    for (int i = 0; i < kRsMaxSeg; ++i) {
        letters[i] = sl.letter[i];
        signs[i] = sl.col[i] > 0 ? 1 : sl.col[i] < 0 ? -1 : 0;
    }
    *n_seg = sl.n_seg;
    *curve_type = sl.curve_type;
    return T2D_OK;
}

extern "C" int t2d_rs_paths(int32_t device_id, int32_t n, double radius, const double* start_dev, const double* goal_dev,
                            uint64_t* valid_dev, double* segments_dev, double* length_dev, int32_t* shortest_dev, void* hip_stream) {
    using namespace t2d;
    if (n < 0 || !(radius > 0.0) || !__builtin_isfinite(radius) || !start_dev || !goal_dev || !valid_dev || !segments_dev ||
        !length_dev || !shortest_dev)
        return T2D_ERR_INVALID;
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return T2D_ERR_HIP;
    hipLaunchKernelGGL(rs_paths_kernel, dim3((n + kPathQueries - 1) / kPathQueries), dim3(kPathQueries * kPathWaves), 0,
                       (hipStream_t)hip_stream, n, radius, start_dev, goal_dev, valid_dev, segments_dev, length_dev, shortest_dev);
    return hipGetLastError() == hipSuccess ? T2D_OK : T2D_ERR_HIP;
}
