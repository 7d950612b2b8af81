// t2d_astar.hip -- the reference's grid A* for n independent queries in one launch (grid_astar_kernel).  The formulas are
// t2d_astar_dev.h; what they restate is search/a_star.py: AStar.plan_graph / AStar.plan over the graph of
// search/graph_utils.py: grid_to_csr.  DESIGN.md 4.26.
#include <cmath>
#include <string>

#include "t2d_astar_dev.h"
#include "t2d_hybrid_dev.h"
#include "t2d_host.h"

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
        hybrid_wave_argmin(f, c, unused);
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
                const double v = hybrid_bcast(sv, k);
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
            const double df = hybrid_bcast(pf, d);
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
            hybrid_wave_argmin(kv, kc, unused);
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
    const auto misaligned = [](const void* p, uintptr_t mask) { return !p || (reinterpret_cast<uintptr_t>(p) & mask); };
    const auto odd = [](const void* p, uintptr_t mask) { return p && (reinterpret_cast<uintptr_t>(p) & mask); };
    if (n < 0 || max_cells < 1 || max_path < 0 || (connectivity != 4 && connectivity != 8))
        return host::fail(nullptr, T2D_ERR_INVALID, "t2d_grid_astar: n >= 0, max_cells >= 1, max_path >= 0 and connectivity 4 or 8");
    if (!std::isfinite(diagonal_cost_multiplier) || diagonal_cost_multiplier < 0.0)
        return host::fail(nullptr, T2D_ERR_INVALID, "t2d_grid_astar: diagonal_cost_multiplier must be finite and not negative");
    if (heuristic_kind < T2D_ASTAR_H_ZERO || heuristic_kind > T2D_ASTAR_H_TABLE)
        return host::fail(nullptr, T2D_ERR_INVALID, "t2d_grid_astar: heuristic_kind must be one of T2D_ASTAR_H_*");
    if (!(cell_size >= kHybridStepMin && cell_size <= kHybridStepMax) || !(std::fabs(origin_x) <= kHybridXYLimit) ||
        !(std::fabs(origin_y) <= kHybridXYLimit))
        return host::fail(nullptr, T2D_ERR_INVALID, "t2d_grid_astar: cell_size must be positive (1e-150 .. 1e150), the origin finite");
    const bool table = heuristic_kind == T2D_ASTAR_H_TABLE, point = !table && heuristic_kind != T2D_ASTAR_H_ZERO;
    if (misaligned(weight_dev, 7u) || misaligned(hw_dev, 3u) || misaligned(source_dev, 3u) || misaligned(target_dev, 3u) ||
        misaligned(path_len_dev, 3u) || misaligned(status_dev, 3u) || misaligned(iterations_dev, 3u) || misaligned(expanded_dev, 3u) ||
        (max_path > 0 && misaligned(path_dev, 3u)) || odd(path_xy_dev, 7u) || odd(g_dev, 7u) || odd(parent_dev, 3u) ||
        (point && misaligned(htarget_dev, 7u)) || (table && misaligned(h_dev, 7u)) || misaligned(workspace_dev, 15u))
        return host::fail(nullptr, T2D_ERR_INVALID, "t2d_grid_astar: null or misaligned device pointer (the workspace: 16 bytes)");
    if (max_cells > T2D_GRID_MAX_CELLS)
        return host::fail(nullptr, T2D_ERR_GEOMETRY, "t2d_grid_astar: a grid of " + std::to_string(max_cells) +
                                                         " cells is above T2D_GRID_MAX_CELLS = " + std::to_string(T2D_GRID_MAX_CELLS) +
                                                         " (one fp64 key per cell in LDS)");
    const int64_t need = t2d_grid_astar_workspace_bytes(n, max_cells, connectivity);
    if (workspace_bytes < need)
        return host::fail(nullptr, T2D_ERR_INVALID, "t2d_grid_astar: the workspace has " + std::to_string(workspace_bytes) +
                                                        " bytes, t2d_grid_astar_workspace_bytes asks for " + std::to_string(need));
    if (n == 0) return T2D_OK;
    if (hipSetDevice(device_id) != hipSuccess) return host::fail(nullptr, T2D_ERR_HIP, "t2d_grid_astar: hipSetDevice failed");
    AStarArgs a;
    a.weight = weight_dev;
    a.hw = hw_dev;
    a.source = source_dev;
    a.target = target_dev;
    a.htarget = point ? htarget_dev : nullptr;
    a.table = table ? h_dev : nullptr;
    a.mult = diagonal_cost_multiplier;
    a.scale = heuristic_scale;
    a.cell = cell_size;
    a.ox = origin_x;
    a.oy = origin_y;
    a.stride = max_cells;
    a.conn = connectivity;
    a.kind = heuristic_kind;
    a.max_iter = max_iter;
    a.max_path = max_path;
    a.ws = static_cast<unsigned char*>(workspace_dev);
    a.ws_row = astar_row_bytes(max_cells, connectivity);
    a.path = path_dev;
    a.path_len = path_len_dev;
    a.path_xy = max_path > 0 ? path_xy_dev : nullptr;
    a.status = status_dev;
    a.iterations = iterations_dev;
    a.expanded = expanded_dev;
    a.g = g_dev;
    a.closed = closed_dev;
    a.parent = parent_dev;
    hipLaunchKernelGGL(grid_astar_kernel, dim3((unsigned)n), dim3(64), (size_t)astar_lds_bytes(max_cells), (hipStream_t)hip_stream, a);
    const hipError_t err = hipGetLastError();
    if (err != hipSuccess) return host::fail(nullptr, T2D_ERR_HIP, std::string("t2d_grid_astar: ") + hipGetErrorString(err));
    return T2D_OK;
}
