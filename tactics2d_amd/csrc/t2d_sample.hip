// t2d_sample.hip -- the reference's sampling planners for n independent queries in one launch (sample_plan_kernel): RRT, RRT* and
// RRT-Connect.  The formulas are t2d_sample_dev.h; what they restate is search/rrt.py, search/rrt_star.py and
// search/rrt_connect.py with the grid collision checker the reference's tests pair with them.  DESIGN.md 4.23.
#include <string>

#include "t2d_plan_host.h"
#include "t2d_sample_dev.h"

namespace t2d {

static_assert(SAMPLE_RRT == T2D_SAMPLE_RRT && SAMPLE_RRT_STAR == T2D_SAMPLE_RRT_STAR && SAMPLE_RRT_CONNECT == T2D_SAMPLE_RRT_CONNECT,
              "t2d.h");
static_assert(SAMPLE_FOUND == T2D_SAMPLE_FOUND && SAMPLE_MAX_ITER == T2D_SAMPLE_MAX_ITER && SAMPLE_TRUNCATED == T2D_SAMPLE_TRUNCATED &&
              SAMPLE_OVERFLOW == T2D_SAMPLE_OVERFLOW && SAMPLE_INVALID == T2D_SAMPLE_INVALID, "t2d.h");
static_assert(kSampleLdsNodes == T2D_SAMPLE_LDS_NODES, "t2d.h");

namespace {

// One query per wave, one wave per workgroup.  The loop is serial in its iterations; an iteration's nearest node is the wave's
// argmin of (d, index) over the tree -- numpy's argmin returns the first minimum, which is the minimum of that total order --, a
// segment's collision test spreads the cells near it over the 64 lanes, and RRT*'s two passes over the neighbourhood scan one node
// per lane and test only the segments that can matter, each with the whole wave.  Every branch around a barrier is taken by the
// whole wave: the counters live in every lane with the same value.
// Tree slot s holds a node's x, y (LDS for the first kSampleLdsNodes slots a query uses at each end of its buffer, and always
// the workspace), cost and parent.  Tree a grows from slot 0 upwards, RRT-Connect's tree b from slot max_nodes - 1 downwards.
__global__ __launch_bounds__(64) void sample_plan_kernel(SampleArgs a) {
    __shared__ double2 s_xy[kSampleLdsNodes];
    const int e = blockIdx.x, lane = threadIdx.x;
    const double nan = __builtin_nan(""), inf = __builtin_huge_val();

    const int H = a.hw[2 * e], W = a.hw[2 * e + 1];
    const double sx = a.start[2 * e], sy = a.start[2 * e + 1], tx = a.target[2 * e], ty = a.target[2 * e + 1];
    const double x_min = a.boundary[4 * e], x_max = a.boundary[4 * e + 1], y_min = a.boundary[4 * e + 2], y_max = a.boundary[4 * e + 3];
    const Stream stream{a.seed[e]};
    const double step = a.step, r2 = a.radius * a.radius;
    const int kind = a.kind, max_nodes = a.max_nodes;
    const bool connect = kind == SAMPLE_RRT_CONNECT;

    unsigned char* row = a.ws + (long long)e * a.ws_row;
    double2* g_xy = reinterpret_cast<double2*>(row);
    double* g_cost = reinterpret_cast<double*>(row + sample_cost_offset(max_nodes));
    int* g_parent = reinterpret_cast<int*>(row + sample_parent_offset(max_nodes));
    const ObstacleGrid obstacles{a.weight + (size_t)e * (size_t)a.stride, H, W, a.ox, a.oy, a.cell};

    // the LDS copy of slot s, or -1: the front lds_front slots and the back kSampleLdsNodes - lds_front ones
    const int lds_front = connect ? kSampleLdsNodes / 2 : kSampleLdsNodes;
    const auto lds_of = [&](int s) {
        if (s < lds_front) return s;
        const int back = max_nodes - s;   // 1 for the last slot
        return back <= kSampleLdsNodes - lds_front ? kSampleLdsNodes - back : -1;
    };
    const auto load_xy = [&](int s) {
        const int l = lds_of(s);
        return l >= 0 ? s_xy[l] : g_xy[s];
    };
    // node i of a tree -> its slot
    const auto slot_of = [&](bool back, int i) { return back ? max_nodes - 1 - i : i; };
    // the whole wave appends ONE node: lane 0 writes it
    const auto put = [&](int s, double x, double y, int parent, double cost) {
        if (lane == 0) {
            const int l = lds_of(s);
            if (l >= 0) s_xy[l] = make_double2(x, y);
            g_xy[s] = make_double2(x, y);
            g_parent[s] = parent;
            if (kind == SAMPLE_RRT_STAR) g_cost[s] = cost;
        }
    };
    // the segment p1 -> p2 against the obstacle cells near it, 64 at a time; the same answer in every lane
    const auto seg_hit = [&](double x1, double y1, double x2, double y2) { return obstacles.wave_seg_hit(x1, y1, x2, y2, lane); };
    // the node of a tree nearest to (px, py): the first minimum of dx * dx + dy * dy
    const auto nearest = [&](bool back, int count, double px, double py) {
        double bd = inf;
        int bi = 0x7fffffff, bp = 0;
        for (int i = lane; i < count; i += 64) {
            const double2 v = load_xy(slot_of(back, i));
            const double dx = v.x - px, dy = v.y - py, d = dx * dx + dy * dy;
            if (d < bd) {   // (a lane's indices ascend: its first minimum stays)
                bd = d;
                bi = i;
            }
        }
        wave_argmin(bd, bi, bp);
        return bi;
    };

    int status = -1, iterations = 0, na = 0, nb = 0, end_a = -1, end_b = -1;
    {
        // plan_row_bad's condition, written out: through the function this kernel compiles to another instruction stream, which
        // measured 1 to 4 % slower on some shapes
        const auto bad = [](double v) { return !(__builtin_fabs(v) <= kPlanXYLimit); };
        if (bad(sx) || bad(sy) || bad(tx) || bad(ty) || bad(x_min) || bad(x_max) || bad(y_min) || bad(y_max) || H < 1 || W < 1 ||
            (long long)H * (long long)W > (long long)a.stride)
            status = SAMPLE_INVALID;
    }
    if (status < 0) {
        put(0, sx, sy, -1, 0.0);
        na = 1;
        if (connect) {
            if (max_nodes < 2) status = SAMPLE_OVERFLOW;
            else {
                put(max_nodes - 1, tx, ty, -1, 0.0);
                nb = 1;
            }
        }
        __syncthreads();
    }

    for (int it = 0; status < 0 && it < a.max_iter; ++it) {
        iterations = it + 1;
        const double rx = x_min + (x_max - x_min) * stream.peek(2ull * (uint64_t)it);
        const double ry = y_min + (y_max - y_min) * stream.peek(2ull * (uint64_t)it + 1ull);
        const bool from_b = connect && (it & 1);
        const int from_n = from_b ? nb : na;
        // ---- nearest, steer, bounds, collision ----
        const int ni = nearest(from_b, from_n, rx, ry);
        const double2 nn = load_xy(slot_of(from_b, ni));
        const double dx = rx - nn.x, dy = ry - nn.y;
        const double dist = __builtin_sqrt(dx * dx + dy * dy);
        double nx = rx, ny = ry;
        if (!(dist < step)) {
            nx = nn.x + step * dx / dist;
            ny = nn.y + step * dy / dist;
        }
        if (!(x_min <= nx && nx <= x_max && y_min <= ny && ny <= y_max)) continue;
        if (seg_hit(nn.x, nn.y, nx, ny)) continue;
        if (na + nb + 1 > max_nodes) {
            status = SAMPLE_OVERFLOW;
            break;
        }
        int parent = ni;
        double cost = 0.0;
        const int new_idx = from_n;
        if (kind == SAMPLE_RRT_STAR) {
            // ---- _choose_parent: the smallest (cost, index) among the neighbours whose segment is free, if its cost is STRICTLY
            // below the nearest node's.  The candidates are tried in increasing (cost, index), so the first free one is it; each
            // round is one scan and one wave-wide segment test, and in open space the first round ends it.
            const double ex = nx - nn.x, ey = ny - nn.y;
            cost = g_cost[ni] + __builtin_sqrt(ex * ex + ey * ey);
            double tried_c = -inf;
            int tried_i = -1;
            for (;;) {
                double bc = inf;
                int bi = 0x7fffffff, bp = 0;
                for (int i = lane; i < na; i += 64) {
                    const double2 v = load_xy(i);
                    const double fx = v.x - nx, fy = v.y - ny, d2 = fx * fx + fy * fy;
                    if (d2 <= r2) {
                        const double c = g_cost[i] + __builtin_sqrt(d2);
                        if (c < cost && (c > tried_c || (c == tried_c && i > tried_i)) && c < bc) {
                            bc = c;
                            bi = i;
                        }
                    }
                }
                wave_argmin(bc, bi, bp);
                if (bi == 0x7fffffff) break;
                const double2 v = load_xy(bi);
                if (!seg_hit(v.x, v.y, nx, ny)) {
                    parent = bi;
                    cost = bc;
                    break;
                }
                tried_c = bc;
                tried_i = bi;
            }
        }
        put(slot_of(from_b, new_idx), nx, ny, parent, cost);
        if (from_b) ++nb;
        else ++na;
        if (kind == SAMPLE_RRT_STAR) {
            // ---- the rewire: every other node within the radius, each on its own, against the new node's cost.  A node that
            // would not get cheaper is not tested; the others' segments are tested by the whole wave, one node after another.
            for (int base = 0; base < new_idx; base += 64) {
                const int i = base + lane;
                double2 v = make_double2(0.0, 0.0);
                double alt = 0.0;
                bool cheaper = false;
                if (i < new_idx) {
                    v = load_xy(i);
                    const double fx = v.x - nx, fy = v.y - ny, d2 = fx * fx + fy * fy;
                    if (d2 <= r2) {
                        alt = cost + __builtin_sqrt(d2);
                        cheaper = alt < g_cost[i];
                    }
                }
                for (unsigned long long m = __ballot(cheaper); m; m &= m - 1) {
                    const int src = __builtin_ctzll(m);
                    const bool hit = seg_hit(wave_bcast(v.x, src), wave_bcast(v.y, src), nx, ny);
                    if (lane == src && !hit) {
                        g_parent[i] = new_idx;
                        g_cost[i] = alt;
                    }
                }
            }
        }
        __syncthreads();   // the node (LDS and workspace) and the rewired costs -> the lanes that read them next
        if (connect) {
            // ---- ONE segment to the nearest node of the other tree ----
            const int j = nearest(!from_b, from_b ? na : nb, nx, ny);
            const double2 q = load_xy(slot_of(!from_b, j));
            if (!seg_hit(nx, ny, q.x, q.y)) {
                end_a = from_b ? j : new_idx;
                end_b = from_b ? new_idx : j;
                status = SAMPLE_FOUND;
            }
        } else {
            const double gx = nx - tx, gy = ny - ty;
            const double gd = __builtin_sqrt(gx * gx + gy * gy);
            if (gd < step && !seg_hit(nx, ny, tx, ty)) {
                if (na + 1 > max_nodes) {
                    status = SAMPLE_OVERFLOW;
                    break;
                }
                put(na, tx, ty, new_idx, cost + gd);
                ++na;
                status = SAMPLE_FOUND;
                __syncthreads();
            }
        }
    }
    if (status < 0) status = SAMPLE_MAX_ITER;

    // ---- the path, start first.  RRT and RRT*: the walk from the last node appended, found or not (rrt.py:147).  RRT-Connect:
    // a's walk, then b's towards the target.  A walk is bounded by its tree's node count.
    int len = 0;
    if (status == SAMPLE_FOUND || (status == SAMPLE_MAX_ITER && !connect)) {
        if (!connect) end_a = na - 1;
        int la = 0, lb = 0;
        for (int i = end_a; i != -1 && la < na; i = g_parent[i]) ++la;
        for (int i = end_b; i != -1 && lb < nb; i = g_parent[slot_of(true, i)]) ++lb;
        len = la + lb;
        if (lane == 0) {
            double* out = a.path + (size_t)e * (size_t)a.max_path * 2;
            int k = la - 1;
            for (int i = end_a; k >= 0; i = g_parent[i], --k) {
                if (k < a.max_path) {
                    const double2 v = g_xy[i];
                    out[2 * k] = v.x;
                    out[2 * k + 1] = v.y;
                }
            }
            k = la;
            for (int i = end_b; k < len; i = g_parent[slot_of(true, i)], ++k) {
                if (k < a.max_path) {
                    const double2 v = g_xy[slot_of(true, i)];
                    out[2 * k] = v.x;
                    out[2 * k + 1] = v.y;
                }
            }
        }
        if (status == SAMPLE_FOUND && len > a.max_path) status = SAMPLE_TRUNCATED;
    }
    {   // (plan_path_tail<2, 64>, written out for the same reason)
        double* out = a.path + (size_t)e * (size_t)a.max_path * 2;
        const int from = (len < a.max_path ? len : a.max_path) * 2;
        for (int i = from + lane; i < a.max_path * 2; i += 64) out[i] = nan;
    }
    if (lane == 0) {
        a.path_len[e] = len;
        a.status[e] = status;
        a.iterations[e] = iterations;
        a.nodes[2 * e] = na;
        a.nodes[2 * e + 1] = nb;
    }
}

}  // namespace
}  // namespace t2d

extern "C" int64_t t2d_sample_plan_workspace_bytes(int32_t n, int32_t max_nodes) {
    if (n < 0 || max_nodes < 1) return -1;
    return (int64_t)n * (int64_t)t2d::sample_row_bytes(max_nodes);
}

extern "C" int t2d_sample_plan(int32_t device_id, int32_t n, int32_t kind, const double* weight_dev, const int32_t* hw_dev,
                               int32_t max_cells, const double* start_dev, const double* target_dev, const double* boundary_dev,
                               const uint64_t* seed_dev, double extension_step, double radius, double cell_size, double origin_x,
                               double origin_y, int32_t max_iter, int32_t max_nodes, int32_t max_path, void* workspace_dev,
                               int64_t workspace_bytes, double* path_dev, int32_t* path_len_dev, int32_t* status_dev,
                               int32_t* iterations_dev, int32_t* nodes_dev, void* hip_stream) {
    using namespace t2d;
    host::PlanEntry entry("t2d_sample_plan");
    if (kind != T2D_SAMPLE_RRT && kind != T2D_SAMPLE_RRT_STAR && kind != T2D_SAMPLE_RRT_CONNECT)
        return entry.invalid("kind must be T2D_SAMPLE_RRT, _RRT_STAR or _RRT_CONNECT");
    if (n < 0 || max_cells < 1 || max_path < 0 || max_nodes < 1 || max_iter < 0)
        return entry.invalid("n >= 0, max_cells >= 1, max_path >= 0, max_nodes >= 1 and max_iter >= 0");
    if (!(extension_step >= kPlanStepMin && extension_step <= kPlanStepMax)) return entry.invalid("extension_step must be positive (1e-150 .. 1e150)");
    if (!(radius >= 0.0)) return entry.invalid("radius must not be negative or NaN");
    if (int rc = entry.cell_origin(cell_size, origin_x, origin_y)) return rc;
    entry.required(7u, weight_dev, start_dev, target_dev, boundary_dev, seed_dev);
    entry.required(3u, hw_dev, path_len_dev, status_dev, iterations_dev, nodes_dev);
    if (max_path > 0) entry.required(7u, path_dev);
    if (int rc = entry.workspace(workspace_dev).pointers()) return rc;
    if (int rc = entry.workspace_bytes(workspace_bytes, t2d_sample_plan_workspace_bytes(n, max_nodes))) return rc;
    const SampleArgs a{weight_dev, hw_dev, start_dev, target_dev, boundary_dev, seed_dev,
                       kind, max_cells, max_iter, max_nodes, max_path, extension_step, radius, cell_size, origin_x, origin_y,
                       static_cast<unsigned char*>(workspace_dev), sample_row_bytes(max_nodes),
                       path_dev, path_len_dev, status_dev, iterations_dev, nodes_dev};
    return entry.launch(device_id, n, [&] { hipLaunchKernelGGL(sample_plan_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)hip_stream, a); });
}
