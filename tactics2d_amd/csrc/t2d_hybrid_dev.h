// t2d_hybrid_dev.h -- the pieces of the hybrid A* (search/hybrid_a_star.py: HybridAStar.plan with the grid collision checker of the
// reference's tests/test_search.py: create_grid_collision_checker) as device functions.  fp64 throughout, one rounding per
// operation; tests/hybrid_astar_ref.py states the same operations in Python.  The collision checker and the wave-wide argmin are
// t2d_gridplan_dev.h's.  DESIGN.md 4.22.
#pragma once
#include "t2d_gridplan_dev.h"

namespace t2d {

enum { HYBRID_FOUND = 0, HYBRID_NO_PATH = 1, HYBRID_MAX_ITER = 2, HYBRID_TRUNCATED = 3, HYBRID_OVERFLOW = 4, HYBRID_INVALID = 5 };
constexpr int kHybridMaxOpen = 2048;       // open entries of one query: (f, node) in 24 KiB of LDS, six queries per CU
constexpr int kHybridMaxXYCells = 32768;   // x_cells * y_cells of one query's cost grid: 16 headings of 2 bytes each, 1 MiB
constexpr int kHybridMaxSteer = 16;
constexpr int kHybridHeadingCells = 16;
constexpr int kHybridEmpty = 65535;        // the cost grid's +inf; a node's depth is 0 .. 65534
constexpr double kHybridHeadingRes = 3.141592653589793 / 8;
constexpr double kHybridAngleLimit = 1e9;

// The arguments of one launch (t2d_hybrid_astar), checked by the entry point.
struct HybridArgs {
    const double* weight;      // [n][stride]
    const int32_t* hw;         // [n][2]
    const double* start;       // [n][3]
    const double* target;      // [n][3]
    const double* boundary;    // [n][4]
    const double* delta;       // [n_steer]
    int n_steer, stride, max_iter, max_nodes, max_path;
    double step, cell, ox, oy;
    unsigned char* ws;         // the caller's workspace: ws_row bytes per query
    long long ws_row;
    double* path;              // [n][max_path][3]
    int32_t* path_len;         // [n]
    int32_t* status;           // [n]
    int32_t* iterations;       // [n]
    int32_t* nodes;            // [n]
};

// One query's share of the workspace: the nodes' x, y, heading, g (32 bytes each), their parent and depth (8 bytes each), the
// cost grid.  Every part starts on a multiple of 16 bytes.
__host__ __device__ inline long long hybrid_pd_offset(int max_nodes) { return (long long)max_nodes * 32; }
__host__ __device__ inline long long hybrid_grid_offset(int max_nodes) {
    return hybrid_pd_offset(max_nodes) + (((long long)max_nodes * 8 + 15) & ~15ll);
}
__host__ __device__ inline long long hybrid_row_bytes(int max_nodes) {
    return (hybrid_grid_offset(max_nodes) + (long long)kHybridMaxXYCells * kHybridHeadingCells * 2 + 255) & ~255ll;
}

T2D_DEV bool hybrid_bad_angle(double v) { return !(__builtin_fabs(v) <= kHybridAngleLimit); }

// _heuristic as written: it goes negative for a heading difference above 2 pi
T2D_DEV double hybrid_heuristic(double x, double y, double h, double tx, double ty, double th) {
    const double dx = x - tx, dy = y - ty;
    const double dist = __builtin_sqrt(dx * dx + dy * dy);
    double d = __builtin_fabs(h - th);
    const double d2 = kTwoPi - d;
    if (d2 < d) d = d2;
    return dist + d * 0.1;
}

// state_to_grid's heading index
T2D_DEV int hybrid_heading_cell(double h) {
    const int hi = (int)(mod_two_pi(h) / kHybridHeadingRes);
    return hi >= kHybridHeadingCells ? kHybridHeadingCells - 1 : (hi < 0 ? 0 : hi);   // (mod_two_pi is never negative)
}

}  // namespace t2d
