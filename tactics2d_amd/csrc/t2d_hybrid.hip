// t2d_hybrid.hip -- the reference's hybrid A* for n independent queries in one launch (hybrid_astar_kernel).  The formulas are
// t2d_hybrid_dev.h; what they restate is search/hybrid_a_star.py: HybridAStar.plan with the grid collision checker its tests pair
// with it.  DESIGN.md 4.22.
#include <string>

#include "t2d_hybrid_dev.h"
#include "t2d_plan_host.h"

namespace t2d {

static_assert(HYBRID_FOUND == T2D_HYBRID_FOUND && HYBRID_NO_PATH == T2D_HYBRID_NO_PATH && HYBRID_MAX_ITER == T2D_HYBRID_MAX_ITER &&
              HYBRID_TRUNCATED == T2D_HYBRID_TRUNCATED && HYBRID_OVERFLOW == T2D_HYBRID_OVERFLOW &&
              HYBRID_INVALID == T2D_HYBRID_INVALID, "t2d.h");
static_assert(kHybridMaxOpen == T2D_HYBRID_MAX_OPEN && kHybridMaxXYCells == T2D_HYBRID_MAX_XY_CELLS &&
              kHybridMaxSteer == T2D_HYBRID_MAX_STEER, "t2d.h");

namespace {

// One query per wave, one wave per workgroup.  The search is serial in its pops; a pop is the wave's argmin of (f, node) over the
// open entries in LDS -- the reference's heap of (f, node) tuples yields the minimum of the same total order, so the sequence of
// pops is the reference's whatever the order of the entries --, the popped entry is overwritten with the last one.  Lane s
// evaluates primitive s; the slab tests of a primitive's candidate cells are spread over the 64 lanes; the sequential prune
// (an earlier primitive of the same expansion that took the cell wins) and the append order come from one ballot.  Every
// branch around a barrier is taken by the whole wave: the counters live in every lane with the same value.
__global__ __launch_bounds__(64) void hybrid_astar_kernel(HybridArgs a) {
    __shared__ double s_f[kHybridMaxOpen];
    __shared__ int s_i[kHybridMaxOpen];
    const int e = blockIdx.x, lane = threadIdx.x;
    const int H = a.hw[2 * e], W = a.hw[2 * e + 1];
    const double sx = a.start[3 * e], sy = a.start[3 * e + 1], sh = a.start[3 * e + 2];
    const double tx = a.target[3 * e], ty = a.target[3 * e + 1], th = a.target[3 * e + 2];
    const double x_min = a.boundary[4 * e], x_max = a.boundary[4 * e + 1], y_min = a.boundary[4 * e + 2], y_max = a.boundary[4 * e + 3];
    const double step = a.step, xy_res = step * 0.5;
    const double my_delta = lane < a.n_steer ? a.delta[lane] : 0.0;

    int status = -1, iterations = 0, n_nodes = 0, goal = -1, x_cells = 0, y_cells = 0;
    {
        bool bad = plan_row_bad(sx, sy, tx, ty, x_min, x_max, y_min, y_max, H, W, a.stride) || hybrid_bad_angle(sh) || hybrid_bad_angle(th);
        bad = bad || __ballot(hybrid_bad_angle(my_delta)) != 0ull;
        bad = bad || x_min >= x_max || y_min >= y_max;
        const double inf = __builtin_huge_val();
        const double qx = (sx - x_min) / xy_res, qy = (sy - y_min) / xy_res;
        const double cxd = __builtin_trunc((x_max - x_min) / xy_res) + 1.0, cyd = __builtin_trunc((y_max - y_min) / xy_res) + 1.0;
        bad = bad || __builtin_fabs(qx) == inf || __builtin_fabs(qy) == inf;
        bad = bad || !(0.0 <= __builtin_trunc(qx) && __builtin_trunc(qx) < cxd && 0.0 <= __builtin_trunc(qy) && __builtin_trunc(qy) < cyd);
        if (bad) status = HYBRID_INVALID;
        else if (!(cxd * cyd <= (double)kHybridMaxXYCells)) status = HYBRID_OVERFLOW;
        else {
            x_cells = (int)cxd;
            y_cells = (int)cyd;
        }
    }

    unsigned char* row = a.ws + (long long)e * a.ws_row;
    double4* node_xyhg = reinterpret_cast<double4*>(row);
    int2* node_pd = reinterpret_cast<int2*>(row + hybrid_pd_offset(a.max_nodes));
    uint16_t* grid = reinterpret_cast<uint16_t*>(row + hybrid_grid_offset(a.max_nodes));
    const ObstacleGrid obstacles{a.weight + (size_t)e * (size_t)a.stride, H, W, a.ox, a.oy, a.cell};

    const auto cell_of = [&](double x, double y, double h) {
        int xi = (int)((x - x_min) / xy_res), yi = (int)((y - y_min) / xy_res);
        // (a point inside the boundary is inside the grid, the quotient being monotone; the clamp is the kernel's own bound check)
        xi = xi < 0 ? 0 : (xi >= x_cells ? x_cells - 1 : xi);
        yi = yi < 0 ? 0 : (yi >= y_cells ? y_cells - 1 : yi);
        return (xi * y_cells + yi) * kHybridHeadingCells + hybrid_heading_cell(h);
    };

    int open_n = 0;
    if (status < 0) {
        // the cost grid: 32 bytes per (x, y) cell, all ones = kHybridEmpty in each of its 16 headings
        uint4* g4 = reinterpret_cast<uint4*>(grid);
        const int words = x_cells * y_cells * 2;
        for (int i = lane; i < words; i += 64) g4[i] = make_uint4(~0u, ~0u, ~0u, ~0u);
        __syncthreads();   // (different lanes write the same 32 bytes next)
        if (lane == 0) {
            node_xyhg[0] = make_double4(sx, sy, sh, 0.0);
            node_pd[0] = make_int2(-1, 0);
            grid[cell_of(sx, sy, sh)] = 0;
            s_f[0] = 0.0 + hybrid_heuristic(sx, sy, sh, tx, ty, th);
            s_i[0] = 0;
        }
        open_n = n_nodes = 1;
        __syncthreads();
    }

    while (status < 0) {
        if (open_n == 0) {
            status = HYBRID_NO_PATH;
            break;
        }
        if (iterations >= a.max_iter) {
            status = HYBRID_MAX_ITER;
            break;
        }
        // ---- pop: the smallest (f, node) ----
        double bf = __builtin_huge_val();
        int bi = 0x7fffffff, bp = 0;
        for (int i = lane; i < open_n; i += 64) {
            const double f = s_f[i];
            const int idx = s_i[i];
            if (f < bf || (f == bf && idx < bi)) {
                bf = f;
                bi = idx;
                bp = i;
            }
        }
        wave_argmin(bf, bi, bp);
        const int idx = bi;
        ++iterations;
        --open_n;
        if (lane == 0 && bp != open_n) {
            s_f[bp] = s_f[open_n];
            s_i[bp] = s_i[open_n];
        }
        const double4 cur = node_xyhg[idx];
        const int depth = node_pd[idx].y;
        const double x = cur.x, y = cur.y, h = cur.z, g = cur.w;
        if (__builtin_fabs(x - tx) < xy_res && __builtin_fabs(y - ty) < xy_res && __builtin_fabs(h - th) < kHybridHeadingRes) {
            goal = idx;
            break;
        }
        // ---- lane s: primitive s ----
        const double new_g = g + step;
        const int new_depth = depth + 1;
        const double new_h = h + my_delta, avg = h + my_delta / 2;
        double sn, cs;
        sincos_det(avg, sn, cs);
        const double nx = x + cs * step, ny = y + sn * step;
        bool alive = lane < a.n_steer && x_min <= nx && nx <= x_max && y_min <= ny && ny <= y_max;
        // ---- the slab tests of primitive s over the obstacle cells near its segment, 64 at a time ----
        unsigned long long todo = __ballot(alive), hit_mask = 0ull;
        while (todo) {
            const int s = __builtin_ctzll(todo);
            todo &= todo - 1;
            if (obstacles.wave_seg_hit(x, y, wave_bcast(nx, s), wave_bcast(ny, s), lane)) hit_mask |= 1ull << s;
        }
        alive = alive && !(hit_mask >> lane & 1ull);
        // ---- the prune against the cost grid, in the order of the primitives ----
        const int cell = alive ? cell_of(nx, ny, new_h) : -1;
        bool keep = alive && new_depth < (int)grid[cell < 0 ? 0 : cell];
        const unsigned long long first = __ballot(keep);
        for (unsigned long long m = first; m; m &= m - 1) {
            const int s = __builtin_ctzll(m);
            const int other = __builtin_amdgcn_readlane(cell, s);
            if (s < lane && other == cell) keep = false;   // (both have new_depth: the later one is not cheaper)
        }
        const unsigned long long kept = __ballot(keep);
        const int count = __builtin_popcountll(kept);
        if (count && (new_depth >= kHybridEmpty || n_nodes + count > a.max_nodes || open_n + count > kHybridMaxOpen)) {
            status = HYBRID_OVERFLOW;
            break;
        }
        if (keep) {
            const int rank = __builtin_popcountll(kept & ((1ull << lane) - 1ull));
            const int ni = n_nodes + rank;
            node_xyhg[ni] = make_double4(nx, ny, new_h, new_g);
            node_pd[ni] = make_int2(idx, new_depth);
            grid[cell] = (uint16_t)new_depth;
            s_f[open_n + rank] = new_g + hybrid_heuristic(nx, ny, new_h, tx, ty, th);
            s_i[open_n + rank] = ni;
        }
        n_nodes += count;
        open_n += count;
        __syncthreads();   // nodes, grid and open entries of this expansion -> the lanes that read them next
    }

    // ---- the path, start first: a node's depth is its place ----
    int len = 0;
    if (goal >= 0) {
        len = node_pd[goal].y + 1;
        status = len <= a.max_path ? HYBRID_FOUND : HYBRID_TRUNCATED;
        if (lane == 0) {
            double* out = a.path + (size_t)e * (size_t)a.max_path * 3;
            for (int i = goal; i != -1;) {
                const double4 v = node_xyhg[i];
                const int2 pd = node_pd[i];
                if (pd.y < a.max_path) {
                    out[3 * pd.y] = v.x;
                    out[3 * pd.y + 1] = v.y;
                    out[3 * pd.y + 2] = v.z;
                }
                i = pd.x;
            }
        }
    }
    plan_path_tail<3, 64>(a.path + (size_t)e * (size_t)a.max_path * 3, len, a.max_path, lane);
    if (lane == 0) {
        a.path_len[e] = len;
        a.status[e] = status;
        a.iterations[e] = iterations;
        a.nodes[e] = n_nodes;
    }
}

}  // namespace
}  // namespace t2d

extern "C" int64_t t2d_hybrid_astar_workspace_bytes(int32_t n, int32_t max_nodes) {
    if (n < 0 || max_nodes < 1) return -1;
    return (int64_t)n * (int64_t)t2d::hybrid_row_bytes(max_nodes);
}

extern "C" int t2d_hybrid_astar(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, int32_t max_cells,
                                const double* start_dev, const double* target_dev, const double* boundary_dev, const double* delta_dev,
                                int32_t n_steer, double step_size, double cell_size, double origin_x, double origin_y, int32_t max_iter,
                                int32_t max_nodes, int32_t max_path, void* workspace_dev, int64_t workspace_bytes, double* path_dev,
                                int32_t* path_len_dev, int32_t* status_dev, int32_t* iterations_dev, int32_t* nodes_dev,
                                void* hip_stream) {
    using namespace t2d;
    host::PlanEntry entry("t2d_hybrid_astar");
    if (n < 0 || max_cells < 1 || max_path < 0 || max_nodes < 1) return entry.invalid("n >= 0, max_cells >= 1, max_path >= 0 and max_nodes >= 1");
    if (n_steer < 1 || n_steer > T2D_HYBRID_MAX_STEER) return entry.invalid("n_steer must be 1 .. " + std::to_string(T2D_HYBRID_MAX_STEER));
    if (!(step_size >= kPlanStepMin && step_size <= kPlanStepMax)) return entry.invalid("step_size must be positive (1e-150 .. 1e150)");
    if (int rc = entry.cell_origin(cell_size, origin_x, origin_y)) return rc;
    entry.required(7u, weight_dev, start_dev, target_dev, boundary_dev, delta_dev);
    entry.required(3u, hw_dev, path_len_dev, status_dev, iterations_dev, nodes_dev);
    if (max_path > 0) entry.required(7u, path_dev);
    if (int rc = entry.workspace(workspace_dev).pointers()) return rc;
    if (int rc = entry.workspace_bytes(workspace_bytes, t2d_hybrid_astar_workspace_bytes(n, max_nodes))) return rc;
    const HybridArgs a{weight_dev, hw_dev, start_dev, target_dev, boundary_dev, delta_dev,
                       n_steer, max_cells, max_iter, max_nodes, max_path, step_size, cell_size, origin_x, origin_y,
                       static_cast<unsigned char*>(workspace_dev), hybrid_row_bytes(max_nodes),
                       path_dev, path_len_dev, status_dev, iterations_dev, nodes_dev};
    return entry.launch(device_id, n, [&] { hipLaunchKernelGGL(hybrid_astar_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)hip_stream, a); });
}
