// t2d_gridsearch_dev.h -- shortest paths over a weighted obstacle grid (search/dijkstra.py over the graph of search/graph_utils.py:
// grid_to_csr) as device functions.  fp64 throughout, one rounding per operation; tests/grid_search_ref.py states the same
// operations in numpy.  DESIGN.md 4.21.
//
// A grid is worked on by one workgroup with its weights and its field g in LDS.  The edges are never stored: grid_edge evaluates
// grid_to_csr's expression where it is needed.  grid_relax is one cell's side of a relaxation round (read only: the round's
// writes follow a barrier), grid_pred one cell's predecessor once the field stands.
#pragma once
#include "t2d_math.h"

namespace t2d {

enum { GRID_FOUND = 0, GRID_NO_PATH = 1, GRID_TRUNCATED = 2, GRID_INVALID = 3, GRID_FIELD_ONLY = 4 };
constexpr int kGridMaxCells = 4096;   // two fp64 planes of 32 KiB: two workgroups share a CU's 160 KiB
constexpr int kGridSmallCells = 1024; // the small form: two planes of 8 KiB, eight workgroups of four waves per CU

// The arguments of one launch (t2d_grid_dijkstra), checked by the entry point.
struct GridArgs {
    const double* weight;     // [n][stride]
    const int32_t* hw;        // [n][2]
    const int32_t* source;    // [n]
    const int32_t* target;    // [n]
    double mult;              // diagonal_cost_multiplier
    int stride, diagonals, max_path;
    double* g;                // [n][stride]
    int32_t* path;            // [n][max_path]
    int32_t* path_len;        // [n]
    int32_t* status;          // [n]
    int32_t* sweeps;          // [n]
};

T2D_DEV double grid_inf() { return __builtin_huge_val(); }

// the neighbours of a cell, orthogonal ones first (bits 0 .. 3 of a neighbour mask), then the diagonal ones (bits 4 .. 7)
T2D_DEV int grid_dr(int d) { return d == 1 || d == 4 || d == 5 ? 1 : (d == 3 || d == 6 || d == 7 ? -1 : 0); }
T2D_DEV int grid_dc(int d) { return d == 0 || d == 4 || d == 6 ? 1 : (d == 2 || d == 5 || d == 7 ? -1 : 0); }

// bit d: neighbour d of (r, c) lies inside the H x W grid (and diagonals are edges at all)
T2D_DEV int grid_neighbour_mask(int r, int c, int H, int W, int diagonals) {
    int m = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        const int rr = r + grid_dr(d), cc = c + grid_dc(d);
        if (rr >= 0 && rr < H && cc >= 0 && cc < W && (d < 4 || diagonals)) m |= 1 << d;
    }
    return m;
}

// grid_to_csr's edge weight, operation by operation (the sum of two doubles does not depend on their order).  An obstacle is
// +inf here, so its edges are +inf and never improve anything.
T2D_DEV double grid_edge(double wa, double wb, bool diagonal, double mult) {
    double e = (wa + wb) / 2.0;
    if (diagonal) e = e * mult;
    return e;
}

// min over the neighbours u of fl(g[u] + e(u, v)), and g[v] itself.  An edge of weight exactly 0 is no edge (the reference walks
// graph[i].nonzero()); a NaN edge (inf * 0) compares false and improves nothing.
T2D_DEV double grid_relax(const double* s_g, const double* s_w, int v, int W, int mask, double wv, double mult) {
    double best = s_g[v];
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        if (!(mask >> d & 1)) continue;
        const int u = v + grid_dr(d) * W + grid_dc(d);
        const double e = grid_edge(wv, s_w[u], d >= 4, mult);
        if (e != 0.0) {
            const double cand = s_g[u] + e;
            if (cand < best) best = cand;
        }
    }
    return best;
}

// The predecessor of v: among the neighbours u with fl(g[u] + e(u, v)) == g[v] that precede v in the order of (g, index), the
// one with the smallest (g[u], u); -1 where there is none (the source, an unreached cell).
T2D_DEV int grid_pred(const double* s_g, const double* s_w, int v, int W, int mask, double wv, double mult) {
    const double gv = s_g[v];
    if (!(gv < grid_inf())) return -1;
    double bg = grid_inf();
    int bu = -1;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        if (!(mask >> d & 1)) continue;
        const int u = v + grid_dr(d) * W + grid_dc(d);
        const double e = grid_edge(wv, s_w[u], d >= 4, mult), gu = s_g[u];
        if (e != 0.0 && gu + e == gv && (gu < gv || (gu == gv && u < v)) && (bu < 0 || gu < bg || (gu == bg && u < bu))) {
            bg = gu;
            bu = u;
        }
    }
    return bu;
}

}  // namespace t2d
