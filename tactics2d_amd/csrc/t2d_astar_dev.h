// t2d_astar_dev.h -- the pieces of the grid A* (search/a_star.py: AStar.plan_graph / AStar.plan over the graph of
// search/graph_utils.py: grid_to_csr) as device functions.  fp64 throughout, one rounding per operation; tests/astar_ref.py states
// the same operations in Python.  The edge expression and the neighbour order are t2d_gridsearch_dev.h's.  DESIGN.md 4.26.
#pragma once
#include "t2d_gridsearch_dev.h"

namespace t2d {

enum { GRID_MAX_ITER = 5 };   // beside GRID_FOUND .. GRID_FIELD_ONLY
enum { ASTAR_H_ZERO = 0, ASTAR_H_EUCLIDEAN = 1, ASTAR_H_MANHATTAN = 2, ASTAR_H_OCTILE = 3, ASTAR_H_TABLE = 4 };
constexpr int kAStarNoCell = 0x7fffffff;   // the cell of "no entry": it loses against every cell at equal f, +inf included

// The arguments of one launch (t2d_grid_astar), checked by the entry point.
struct AStarArgs {
    const double* weight;      // [n][stride]
    const int32_t* hw;         // [n][2]
    const int32_t* source;     // [n]
    const int32_t* target;     // [n]
    const double* htarget;     // [n][2] (NULL: ZERO and TABLE)
    const double* table;       // [n][stride] (TABLE only)
    double mult, scale, cell, ox, oy;
    int stride, conn, kind, max_iter, max_path;
    unsigned char* ws;         // the caller's workspace: ws_row bytes per query
    long long ws_row;
    int32_t* path;             // [n][max_path]
    int32_t* path_len;         // [n]
    double* path_xy;           // [n][max_path][2] or NULL
    int32_t* status;           // [n]
    int32_t* iterations;       // [n]
    int32_t* expanded;         // [n]
    double* g;                 // [n][stride] or NULL
    uint8_t* closed;           // [n][stride] or NULL
    int32_t* parent;           // [n][stride] or NULL
};

// One query's share of the workspace: per cell the f of every push it can ever receive (one per neighbour, each neighbour closing
// once), heuristic_scale * h, g and came_from (the last two are used only where the caller passes no output for them).
__host__ __device__ inline long long astar_sh_offset(int stride, int conn) { return (long long)stride * conn * 8; }
__host__ __device__ inline long long astar_g_offset(int stride, int conn) { return astar_sh_offset(stride, conn) + (long long)stride * 8; }
__host__ __device__ inline long long astar_parent_offset(int stride, int conn) { return astar_g_offset(stride, conn) + (long long)stride * 8; }
__host__ __device__ inline long long astar_row_bytes(int stride, int conn) {
    return (astar_parent_offset(stride, conn) + (long long)stride * 4 + 255) & ~255ll;
}

// LDS of one query: per cell the smallest f it still has in the open set (NaN: none), one closed bit and one byte of counters
// (low nibble: the pushes so far, high nibble: those not popped yet), for the row width rounded up to whole blocks of 64 cells
__host__ __device__ inline int astar_cells64(int stride) { return (stride + 63) & ~63; }
__host__ __device__ inline int astar_lds_bytes(int stride) { return astar_cells64(stride) * 8 + astar_cells64(stride) / 8 + astar_cells64(stride); }

// h of the cell (x, y) = (col, row) against the point (hx, hy); `tab` is the cell's table entry
T2D_DEV double astar_h(int kind, int col, int row, double hx, double hy, double mult, double tab) {
    const double dx = (double)col - hx, dy = (double)row - hy;
    if (kind == ASTAR_H_EUCLIDEAN) return __builtin_sqrt(dx * dx + dy * dy);
    const double ax = __builtin_fabs(dx), ay = __builtin_fabs(dy);
    if (kind == ASTAR_H_MANHATTAN) return ax + ay;
    if (kind == ASTAR_H_OCTILE) {
        const double hi = ax > ay ? ax : ay, lo = ax > ay ? ay : ax;
        return hi + (mult - 1.0) * lo;
    }
    return kind == ASTAR_H_TABLE ? tab : 0.0;
}

}  // namespace t2d
