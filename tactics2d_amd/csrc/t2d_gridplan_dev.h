// t2d_gridplan_dev.h -- what the planners over a weighted obstacle grid share on the device (hybrid A*, the sampling planners, the
// probabilistic roadmap, grid A*): the wave-wide pieces, the obstacle grid of one row with the grid collision checker of the
// reference's tests/test_search.py (create_grid_collision_checker), the row check, the tail of `path` and the limits.  fp64
// throughout, one rounding per operation; tests/hybrid_astar_ref.py, sample_plan_ref.py and prm_ref.py state the same operations in
// Python.  DESIGN.md 4.27.
#pragma once
#include "t2d_math.h"

namespace t2d {

// what a coordinate, a cell size and a step may be: beyond them a product or a quotient of two leaves the doubles
constexpr double kPlanXYLimit = 1e150, kPlanStepMin = 1e-150, kPlanStepMax = 1e150;

// ---- wave-wide pieces (64 lanes) ---------------------------------------------------------------------------------------------------
T2D_DEV double wave_bcast(double v, int lane) {   // lane: the same in every lane
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), lane), hi = __builtin_amdgcn_readlane(__double2hiint(v), lane);
    return __hiloint2double(hi, lo);
}

// One step of the min scan: every lane takes the (f, idx, pos) a DPP move brings it -- (+inf, INT_MAX, 0) where the move has no
// source lane or its row is masked -- and keeps the smaller (f, idx).
template <int CTRL, int ROWS>
T2D_DEV void wave_min_step(double& f, int& idx, int& pos) {
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
T2D_DEV void wave_argmin(double& f, int& idx, int& pos) {
    wave_min_step<0x111, 0xf>(f, idx, pos);
    wave_min_step<0x112, 0xf>(f, idx, pos);
    wave_min_step<0x114, 0xf>(f, idx, pos);
    wave_min_step<0x118, 0xf>(f, idx, pos);
    wave_min_step<0x142, 0xa>(f, idx, pos);
    wave_min_step<0x143, 0xc>(f, idx, pos);
    f = wave_bcast(f, 63);
    idx = __builtin_amdgcn_readlane(idx, 63);
    pos = __builtin_amdgcn_readlane(pos, 63);
}

// Exclusive prefix sum of `cnt` over the 64 lanes of a wave (the step kernel's wave_excl_scan: row_shr 1, 2, 4, 8, row_bcast 15
// and 31); `total` is the sum of all 64.  Must be called by all 64 lanes.
T2D_DEV int plan_wave_excl_scan(int cnt, int& total) {
    int v = cnt;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
    total = __builtin_amdgcn_readlane(v, 63);
    return v - cnt;
}

// ---- the obstacle grid of one row ------------------------------------------------------------------------------------------------
// A cell that is +inf or NaN is an obstacle: the closed square of side `cell` centred at (ox, oy) + (col, row) * cell.
struct ObstacleGrid {
    const double* weight;   // the row's H * W weights, row-major
    int H, W;
    double ox, oy, cell;

    static T2D_DEV bool obstacle(double w) { return w != w || w == __builtin_huge_val(); }

    // the cells of one axis whose centre o + k * cs lies in [lo - 1.5 cs, hi + 1.5 cs], rounded outwards, clamped to 0 .. n - 1
    static T2D_DEV void range(double lo, double hi, double o, double cs, int n, int& a, int& b) {
        double fa = (lo - o) / cs - 1.5, fb = (hi - o) / cs + 1.5;
        if (fa < 0.0) fa = 0.0;
        if (fa > (double)n) fa = (double)n;
        if (fb < -1.0) fb = -1.0;
        if (fb > (double)(n - 1)) fb = (double)(n - 1);
        a = (int)__builtin_floor(fa);
        b = (int)__builtin_ceil(fb);
    }

    // one obstacle of collide_fn, operation by operation: the closed square of half side `half` centred at (cx, cy)
    static T2D_DEV bool slab(double x1, double y1, double x2, double y2, double cx, double cy, double half) {
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

    // The cells near the segment p1 -> p2: `range`'s box on each axis, row-major: cnt cells in rows of wc from (r0, c0)
    struct Box { int c0, r0, wc, cnt; };
    T2D_DEV Box box(double x1, double y1, double x2, double y2) const {
        int c0, c1, r0, r1;
        range(x2 < x1 ? x2 : x1, x2 > x1 ? x2 : x1, ox, cell, W, c0, c1);
        range(y2 < y1 ? y2 : y1, y2 > y1 ? y2 : y1, oy, cell, H, r0, r1);
        const int wc = c1 - c0 + 1;
        return {c0, r0, wc, wc > 0 && r1 >= r0 ? wc * (r1 - r0 + 1) : 0};
    }

    // the cell (r, c): does the segment touch it, if it is an obstacle
    T2D_DEV bool hit_at(int r, int c, double x1, double y1, double x2, double y2) const {
        if (!obstacle(weight[r * W + c])) return false;
        return slab(x1, y1, x2, y2, ox + (double)c * cell, oy + (double)r * cell, cell / 2.0);
    }
    // cell j of the box
    T2D_DEV bool cell_hit(const Box& b, int j, double x1, double y1, double x2, double y2) const {
        return hit_at(b.r0 + j / b.wc, b.c0 + j % b.wc, x1, y1, x2, y2);
    }

    // collide_fn for the whole WAVE: the cells of the segment's box, 64 at a time; the same answer in every lane.  Must be called
    // by all 64 lanes with the same segment.
    T2D_DEV bool wave_seg_hit(double x1, double y1, double x2, double y2, int lane) const {
        const Box b = box(x1, y1, x2, y2);
        for (int base = 0; base < b.cnt; base += 64) {
            const int j = base + lane;
            const bool hit = j < b.cnt && cell_hit(b, j, x1, y1, x2, y2);
            if (__ballot(hit)) return true;
        }
        return false;
    }

    // collide_fn for ONE lane with a segment of its own: the cells of the same box, row by row.  Which obstacle answers first does
    // not matter: the result is "any".
    T2D_DEV bool lane_seg_hit(double x1, double y1, double x2, double y2) const {
        int c0, c1, r0, r1;
        range(x2 < x1 ? x2 : x1, x2 > x1 ? x2 : x1, ox, cell, W, c0, c1);
        range(y2 < y1 ? y2 : y1, y2 > y1 ? y2 : y1, oy, cell, H, r0, r1);
        for (int r = r0; r <= r1; ++r) {
            for (int c = c0; c <= c1; ++c) {
                if (hit_at(r, c, x1, y1, x2, y2)) return true;
            }
        }
        return false;
    }
};

// ---- a row's checks and the tail of its path ----------------------------------------------------------------------------------------
T2D_DEV bool plan_bad_xy(double v) { return !(__builtin_fabs(v) <= kPlanXYLimit); }

// a row no planner takes: a start, target or boundary that is not finite (or beyond the limit), no cells, more cells than the row holds
T2D_DEV bool plan_row_bad(double sx, double sy, double tx, double ty, double x_min, double x_max, double y_min, double y_max, int H,
                          int W, int stride) {
    return plan_bad_xy(sx) || plan_bad_xy(sy) || plan_bad_xy(tx) || plan_bad_xy(ty) || plan_bad_xy(x_min) || plan_bad_xy(x_max) ||
           plan_bad_xy(y_min) || plan_bad_xy(y_max) || H < 1 || W < 1 || (long long)H * (long long)W > (long long)stride;
}

// NaN past the end of one row of `path`: COLS doubles per point, from point min(len, max_path) on, by THREADS threads
template <int COLS, int THREADS>
T2D_DEV void plan_path_tail(double* out, int len, int max_path, int tid) {
    const int from = (len < max_path ? len : max_path) * COLS;
    for (int i = from + tid; i < max_path * COLS; i += THREADS) out[i] = __builtin_nan("");
}

}  // namespace t2d
