// t2d_astar.hip -- the reference's grid A* for n independent queries in one launch (grid_astar_kernel).  The formulas are
// t2d_astar_dev.h; what they restate is search/a_star.py: AStar.plan_graph / AStar.plan over the graph of
// search/graph_utils.py: grid_to_csr.  DESIGN.md 4.26.
#include <cmath>
#include <string>

#include "t2d_astar_dev.h"
#include "t2d_plan_host.h"

namespace t2d {

static_assert(GRID_MAX_ITER == T2D_GRID_MAX_ITER, "t2d.h");
static_assert(ASTAR_H_ZERO == T2D_ASTAR_H_ZERO && ASTAR_H_EUCLIDEAN == T2D_ASTAR_H_EUCLIDEAN && ASTAR_H_MANHATTAN == T2D_ASTAR_H_MANHATTAN &&
              ASTAR_H_OCTILE == T2D_ASTAR_H_OCTILE && ASTAR_H_TABLE == T2D_ASTAR_H_TABLE, "t2d.h");

namespace {

// One query per wave, one wave per workgroup.  The reference's heap holds (f, cell) tuples; here the entries of a cell are the f
// values it was pushed with (workspace: at most one per neighbour, because a neighbour pushes when it closes and closes once), the
// smallest of them is the cell's key in LDS, and lane b keeps the smallest (key, cell) of the 64 cells of block b in registers.
// A pop is the wave's argmin over those 64 registers -- the minimum of the same total order the heap yields, equal entries being
// identical --; it removes that f from the cell's entries, and a popped cell that is closed already is the reference's stale
// pop.  Lane d relaxes neighbour d.  Every branch around a barrier is taken by the whole wave: the counters live in every lane
// with the same value.
__global__ __launch_bounds__(64) void grid_astar_kernel(AStarArgs a) {
    extern __shared__ double s_key[];
    const int e = blockIdx.x, lane = threadIdx.x;
    const int cells64 = astar_cells64(a.stride);
    unsigned* s_closed = reinterpret_cast<unsigned*>(s_key + cells64);
    unsigned char* s_cnt = reinterpret_cast<unsigned char*>(s_closed + cells64 / 32);
    const double nan = __builtin_nan(""), inf = grid_inf();

    const int H = a.hw[2 * e], W = a.hw[2 * e + 1], src = a.source[e], tgt = a.target[e];
    const long long cells = (long long)H * (long long)W;
    const bool shape_ok = H > 0 && W > 0 && cells <= (long long)a.stride;
    const int n = shape_ok ? (int)cells : 0;
    bool ok = shape_ok && src >= 0 && src < n && tgt >= 0 && tgt < n;

    const double* w_in = a.weight + (size_t)e * (size_t)a.stride;
    const double* tab = a.kind == ASTAR_H_TABLE ? a.table + (size_t)e * (size_t)a.stride : nullptr;
    unsigned char* row = a.ws + (long long)e * a.ws_row;
    double* slots = reinterpret_cast<double*>(row);
    double* sh = reinterpret_cast<double*>(row + astar_sh_offset(a.stride, a.conn));
    double* g = a.g ? a.g + (size_t)e * (size_t)a.stride : reinterpret_cast<double*>(row + astar_g_offset(a.stride, a.conn));
    int32_t* parent = a.parent ? a.parent + (size_t)e * (size_t)a.stride
                               : reinterpret_cast<int32_t*>(row + astar_parent_offset(a.stride, a.conn));
    const auto weight_of = [&](int v) {
        const double x = w_in[v];
        return x != x ? inf : x;   // NaN is an obstacle, as in grid_to_csr
    };

    // ---- the row's checks; scale * h of every cell, g = +inf, no parent, no entry, nothing closed ----
    double hx = 0.0, hy = 0.0;
    bool bad = !(a.scale >= 0.0 && a.scale < inf);
    if (a.kind == ASTAR_H_EUCLIDEAN || a.kind == ASTAR_H_MANHATTAN || a.kind == ASTAR_H_OCTILE) {
        hx = a.htarget[2 * e];
        hy = a.htarget[2 * e + 1];
        bad = bad || !(__builtin_fabs(hx) < inf) || !(__builtin_fabs(hy) < inf);
    }
    for (int v = lane; v < cells64; v += 64) {
        s_key[v] = nan;
        s_cnt[v] = 0;
    }
    for (int v = lane; v < cells64 / 32; v += 64) s_closed[v] = 0u;
    for (int v = lane; v < n; v += 64) {
        const double h = astar_h(a.kind, v % W, v / W, hx, hy, a.mult, tab ? tab[v] : 0.0);
        const double s = a.scale * h;
        bad = bad || weight_of(v) < 0.0 || h != h || h == -inf || s != s;
        sh[v] = s;
        g[v] = inf;
        parent[v] = -1;
    }
    if (__ballot(bad) != 0ull) ok = false;
    if (ok && (!(weight_of(src) < inf) || !(weight_of(tgt) < inf))) ok = false;
    __syncthreads();

    int status = ok ? -1 : GRID_INVALID, iterations = 0, expanded = 0;
    double bf = inf;          // lane b: the smallest (key, cell) of the cells 64 b .. 64 b + 63
    int bc = kAStarNoCell;
    if (ok) {
        const double f0 = 0.0 + sh[src];
        if (lane == 0) {
            g[src] = 0.0;
            slots[(size_t)src * a.conn] = f0;
            s_key[src] = f0;
            s_cnt[src] = 0x11;
        }
        if (lane == (src >> 6)) {
            bf = f0;
            bc = src;
        }
        __syncthreads();
    }

    while (status < 0) {
        // ---- pop: the smallest (f, cell) ----
        double f = bf;
        int c = bc, unused = 0;
        wave_argmin(f, c, unused);
        if (c == kAStarNoCell) {
            status = GRID_NO_PATH;
            break;
        }
        if (iterations >= a.max_iter) {
            status = GRID_MAX_ITER;
            break;
        }
        const int cnt = s_cnt[c], total = cnt & 15, live = (cnt >> 4) - 1;
        double key = nan;   // the cell's smallest f once this one is gone
        if (live > 0) {
            double sv = lane < total ? slots[(size_t)c * a.conn + lane] : nan;
            const unsigned long long same = __ballot(sv == f);
            if (lane == __builtin_ctzll(same)) {
                slots[(size_t)c * a.conn + lane] = nan;
                sv = nan;
            }
            for (int k = 0; k < total; ++k) {
                const double v = wave_bcast(sv, k);
                if (v == v && !(key <= v)) key = v;
            }
        }
        const bool stale = (s_closed[c >> 5] >> (c & 31) & 1u) != 0u;
        if (lane == 0) {
            s_key[c] = key;
            s_cnt[c] = (unsigned char)(live > 0 ? total | live << 4 : 0);   // (no entry left: its slots start over)
            if (!stale) s_closed[c >> 5] |= 1u << (c & 31);
        }
        bool pushed = false;
        double pf = 0.0;
        int nb = 0;
        if (!stale) {
            ++expanded;
            if (c == tgt) {
                status = GRID_FOUND;
                break;
            }
            // ---- lane d: neighbour d ----
            const int r = c / W, col = c % W, rr = r + grid_dr(lane & 7), cc = col + grid_dc(lane & 7);
            if (lane < a.conn && rr >= 0 && rr < H && cc >= 0 && cc < W) {
                nb = rr * W + cc;
                if (!(s_closed[nb >> 5] >> (nb & 31) & 1u)) {
                    const double edge = grid_edge(weight_of(c), weight_of(nb), lane >= 4, a.mult);
                    const int cn = s_cnt[nb], tot = cn & 15;
                    if (edge != 0.0 && tot < a.conn) {   // (tot < conn always: one push per neighbour)
                        const double t = g[c] + edge;
                        if (t < g[nb]) {
                            parent[nb] = c;
                            g[nb] = t;
                            pf = t + sh[nb];
                            pushed = true;
                            slots[(size_t)nb * a.conn + tot] = pf;
                            s_cnt[nb] = (unsigned char)(cn + 0x11);
                            if (!(s_key[nb] <= pf)) s_key[nb] = pf;
                        }
                    }
                }
            }
        }
        __syncthreads();   // keys, counters, closed bits, g, parents and entries of this pop -> the lanes that read them next
        // ---- the block minima: the pushes into their blocks, then the popped cell's block from its keys ----
        for (unsigned long long m = __ballot(pushed); m; m &= m - 1) {
            const int d = __builtin_ctzll(m);
            const double df = wave_bcast(pf, d);
            const int dn = __builtin_amdgcn_readlane(nb, d);
            if (lane == (dn >> 6) && (df < bf || (df == bf && dn < bc))) {
                bf = df;
                bc = dn;
            }
        }
        {
            const int v = (c & ~63) + lane;
            double kv = s_key[v];
            int kc = kv == kv ? v : kAStarNoCell;
            if (kv != kv) kv = inf;
            wave_argmin(kv, kc, unused);
            if (lane == (c >> 6)) {
                bf = kv;
                bc = kc;
            }
        }
        ++iterations;
    }

    // ---- the path: came_from walked back from the target into LDS (the keys are dead), written out source first ----
    __syncthreads();
    int* s_chain = reinterpret_cast<int*>(s_key);
    int len = 0;
    if (status == GRID_FOUND) {
        int m = 0;
        if (lane == 0) {
            for (int cur = tgt;;) {
                s_chain[m++] = cur;
                const int p = parent[cur];
                if (p < 0 || m >= n) break;
                cur = p;
            }
        }
        len = __builtin_amdgcn_readfirstlane(m);
        if (len > a.max_path) status = GRID_TRUNCATED;
        __syncthreads();
    }
    {
        int32_t* path_out = a.path + (size_t)e * (size_t)a.max_path;
        double* xy_out = a.path_xy ? a.path_xy + (size_t)e * (size_t)a.max_path * 2 : nullptr;
        for (int i = lane; i < a.max_path; i += 64) {
            const int cell = i < len ? s_chain[len - 1 - i] : -1;
            path_out[i] = cell;
            if (xy_out) {
                xy_out[2 * i] = cell < 0 ? nan : a.ox + (double)(cell % W) * a.cell;
                xy_out[2 * i + 1] = cell < 0 ? nan : a.oy + (double)(cell / W) * a.cell;
            }
        }
    }
    if (a.closed) {
        uint8_t* closed_out = a.closed + (size_t)e * (size_t)a.stride;
        for (int v = lane; v < n; v += 64) closed_out[v] = (uint8_t)(s_closed[v >> 5] >> (v & 31) & 1u);
    }
    if (lane == 0) {
        a.path_len[e] = len;
        a.status[e] = status;
        a.iterations[e] = iterations;
        a.expanded[e] = expanded;
    }
}

}  // namespace
}  // namespace t2d

extern "C" int64_t t2d_grid_astar_workspace_bytes(int32_t n, int32_t max_cells, int32_t connectivity) {
    if (n < 0 || max_cells < 1 || max_cells > T2D_GRID_MAX_CELLS || (connectivity != 4 && connectivity != 8)) return -1;
    return (int64_t)n * (int64_t)t2d::astar_row_bytes(max_cells, connectivity);
}

extern "C" int t2d_grid_astar(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, const int32_t* source_dev,
                              const int32_t* target_dev, int32_t max_cells, int32_t connectivity, double diagonal_cost_multiplier,
                              int32_t heuristic_kind, const double* htarget_dev, const double* h_dev, double heuristic_scale,
                              int32_t max_iter, int32_t max_path, double cell_size, double origin_x, double origin_y, void* workspace_dev,
                              int64_t workspace_bytes, int32_t* path_dev, int32_t* path_len_dev, double* path_xy_dev, int32_t* status_dev,
                              int32_t* iterations_dev, int32_t* expanded_dev, double* g_dev, uint8_t* closed_dev, int32_t* parent_dev,
                              void* hip_stream) {
    using namespace t2d;
    host::PlanEntry entry("t2d_grid_astar");
    if (n < 0 || max_cells < 1 || max_path < 0 || (connectivity != 4 && connectivity != 8))
        return entry.invalid("n >= 0, max_cells >= 1, max_path >= 0 and connectivity 4 or 8");
    if (!std::isfinite(diagonal_cost_multiplier) || diagonal_cost_multiplier < 0.0)
        return entry.invalid("diagonal_cost_multiplier must be finite and not negative");
    if (heuristic_kind < T2D_ASTAR_H_ZERO || heuristic_kind > T2D_ASTAR_H_TABLE) return entry.invalid("heuristic_kind must be one of T2D_ASTAR_H_*");
    if (int rc = entry.cell_origin(cell_size, origin_x, origin_y)) return rc;
    const bool table = heuristic_kind == T2D_ASTAR_H_TABLE, point = !table && heuristic_kind != T2D_ASTAR_H_ZERO;
    entry.required(7u, weight_dev).required(3u, hw_dev, source_dev, target_dev, path_len_dev, status_dev, iterations_dev, expanded_dev);
    entry.optional(7u, path_xy_dev, g_dev).optional(3u, parent_dev);
    if (max_path > 0) entry.required(3u, path_dev);
    if (point) entry.required(7u, htarget_dev);
    if (table) entry.required(7u, h_dev);
    if (int rc = entry.workspace(workspace_dev).pointers()) return rc;
    if (int rc = entry.grid_cap(max_cells, "one fp64 key per cell in LDS")) return rc;
    if (int rc = entry.workspace_bytes(workspace_bytes, t2d_grid_astar_workspace_bytes(n, max_cells, connectivity))) return rc;
    const AStarArgs a{weight_dev, hw_dev, source_dev, target_dev, point ? htarget_dev : nullptr, table ? h_dev : nullptr,
                      diagonal_cost_multiplier, heuristic_scale, cell_size, origin_x, origin_y,
                      max_cells, connectivity, heuristic_kind, max_iter, max_path,
                      static_cast<unsigned char*>(workspace_dev), astar_row_bytes(max_cells, connectivity),
                      path_dev, path_len_dev, max_path > 0 ? path_xy_dev : nullptr, status_dev, iterations_dev, expanded_dev,
                      g_dev, closed_dev, parent_dev};
    return entry.launch(device_id, n, [&] {
        hipLaunchKernelGGL(grid_astar_kernel, dim3((unsigned)n), dim3(64), (size_t)astar_lds_bytes(max_cells), (hipStream_t)hip_stream, a);
    });
}
