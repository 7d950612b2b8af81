// t2d_hybrid_dev.h -- the pieces of the hybrid A* (search/hybrid_a_star.py: HybridAStar.plan with the grid collision checker of the
// reference's tests/test_search.py: create_grid_collision_checker) as device functions.  fp64 throughout, one rounding per
// operation; tests/hybrid_astar_ref.py states the same operations in Python.  DESIGN.md 4.22.
#pragma once
#include "t2d_math.h"

namespace t2d {

enum { HYBRID_FOUND = 0, HYBRID_NO_PATH = 1, HYBRID_MAX_ITER = 2, HYBRID_TRUNCATED = 3, HYBRID_OVERFLOW = 4, HYBRID_INVALID = 5 };
constexpr int kHybridMaxOpen = 2048;       // open entries of one query: (f, node) in 24 KiB of LDS, six queries per CU
constexpr int kHybridMaxXYCells = 32768;   // x_cells * y_cells of one query's cost grid: 16 headings of 2 bytes each, 1 MiB
constexpr int kHybridMaxSteer = 16;
constexpr int kHybridHeadingCells = 16;
constexpr int kHybridEmpty = 65535;        // the cost grid's +inf; a node's depth is 0 .. 65534
constexpr double kHybridHeadingRes = 3.141592653589793 / 8;
constexpr double kHybridXYLimit = 1e150, kHybridAngleLimit = 1e9, kHybridStepMin = 1e-150, kHybridStepMax = 1e150;

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

T2D_DEV bool hybrid_bad(double v, double lim) { return !(__builtin_fabs(v) <= lim); }

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

// the cells of one axis whose centre o + k * cs lies in [lo - 1.5 cs, hi + 1.5 cs], rounded outwards, clamped to 0 .. n - 1
T2D_DEV void hybrid_range(double lo, double hi, double o, double cs, int n, int& a, int& b) {
    double fa = (lo - o) / cs - 1.5, fb = (hi - o) / cs + 1.5;
    if (fa < 0.0) fa = 0.0;
    if (fa > (double)n) fa = (double)n;
    if (fb < -1.0) fb = -1.0;
    if (fb > (double)(n - 1)) fb = (double)(n - 1);
    a = (int)__builtin_floor(fa);
    b = (int)__builtin_ceil(fb);
}

// one obstacle of collide_fn, operation by operation: the closed square of half side `half` centred at (cx, cy)
T2D_DEV bool hybrid_slab(double x1, double y1, double x2, double y2, double cx, double cy, double half) {
    const double dx = x2 - x1, dy = y2 - y1;
    const double ox_min = cx - half, ox_max = cx + half, oy_min = cy - half, oy_max = cy + half;
    const double inf = __builtin_huge_val();
    double tx_min = -inf, tx_max = inf, ty_min = -inf, ty_max = inf;
    if (__builtin_fabs(dx) < 1e-9) {
        if (!(ox_min <= x1 && x1 <= ox_max)) return false;
    } else {
        const double t1 = (ox_min - x1) / dx, t2 = (ox_max - x1) / dx;
        tx_min = t2 < t1 ? t2 : t1;
        tx_max = t2 > t1 ? t2 : t1;
    }
    if (__builtin_fabs(dy) < 1e-9) {
        if (!(oy_min <= y1 && y1 <= oy_max)) return false;
    } else {
        const double t1 = (oy_min - y1) / dy, t2 = (oy_max - y1) / dy;
        ty_min = t2 < t1 ? t2 : t1;
        ty_max = t2 > t1 ? t2 : t1;
    }
    double t_min = ty_min > tx_min ? ty_min : tx_min;
    if (0.0 > t_min) t_min = 0.0;
    double t_max = ty_max < tx_max ? ty_max : tx_max;
    if (1.0 < t_max) t_max = 1.0;
    return t_min <= t_max;
}

// ---- wave-wide pieces (64 lanes) ---------------------------------------------------------------------------------------------------
T2D_DEV double hybrid_bcast(double v, int lane) {   // lane: the same in every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// One step of the min scan: every lane takes the (f, idx, pos) a DPP move brings it -- (+inf, INT_MAX, 0) where the move has no
// source lane or its row is masked -- and keeps the smaller (f, idx).
template <int CTRL, int ROWS>
T2D_DEV void hybrid_min_step(double& f, int& idx, int& pos) {
    const int inf_hi = 0x7ff00000;
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(f), CTRL, ROWS, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(inf_hi, __double2hiint(f), CTRL, ROWS, 0xf, false);
    const int oi = __builtin_amdgcn_update_dpp(0x7fffffff, idx, CTRL, ROWS, 0xf, false);
    const int op = __builtin_amdgcn_update_dpp(0, pos, CTRL, ROWS, 0xf, false);
    const double of = __hiloint2double(hi, lo);
    if (of < f || (of == f && oi < idx)) {
        f = of;
        idx = oi;
        pos = op;
    }
}

// the smallest (f, idx) of the wave with its pos, in every lane: the inclusive scan of the step kernel's prefix sums (row_shr 1, 2,
// 4, 8, row_bcast 15 and 31) with min in the place of +, read from lane 63
T2D_DEV void hybrid_wave_argmin(double& f, int& idx, int& pos) {
    hybrid_min_step<0x111, 0xf>(f, idx, pos);
    hybrid_min_step<0x112, 0xf>(f, idx, pos);
    hybrid_min_step<0x114, 0xf>(f, idx, pos);
    hybrid_min_step<0x118, 0xf>(f, idx, pos);
    hybrid_min_step<0x142, 0xa>(f, idx, pos);
    hybrid_min_step<0x143, 0xc>(f, idx, pos);
    f = hybrid_bcast(f, 63);
    idx = __builtin_amdgcn_readlane(idx, 63);
    pos = __builtin_amdgcn_readlane(pos, 63);
}

}  // namespace t2d
