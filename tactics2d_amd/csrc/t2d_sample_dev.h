// t2d_sample_dev.h -- the pieces of the sampling planners (search/rrt.py: RRT.plan, search/rrt_star.py: RRTStar.plan and
// _choose_parent, search/rrt_connect.py: RRTConnect.plan, with the grid collision checker of the reference's tests/test_search.py)
// as device functions.  fp64 throughout, one rounding per operation; tests/sample_plan_ref.py states the same operations in
// Python.  The slab test, the cell range and the wave-wide argmin are t2d_hybrid_dev.h's.  DESIGN.md 4.23.
#pragma once
#include "t2d_hybrid_dev.h"
#include "t2d_rng.h"

namespace t2d {

enum { SAMPLE_RRT = 0, SAMPLE_RRT_STAR = 1, SAMPLE_RRT_CONNECT = 2 };
enum { SAMPLE_FOUND = 0, SAMPLE_MAX_ITER = 1, SAMPLE_TRUNCATED = 2, SAMPLE_OVERFLOW = 3, SAMPLE_INVALID = 4 };
constexpr int kSampleLdsNodes = 512;   // nodes whose x, y one query keeps in LDS: 8 KiB, twenty queries per CU
constexpr double kSampleXYLimit = 1e150, kSampleStepMin = 1e-150, kSampleStepMax = 1e150;

// The arguments of one launch (t2d_sample_plan), checked by the entry point.
struct SampleArgs {
    const double* weight;      // [n][stride]
    const int32_t* hw;         // [n][2]
    const double* start;       // [n][2]
    const double* target;      // [n][2]
    const double* boundary;    // [n][4]
    const uint64_t* seed;      // [n]
    int kind, stride, max_iter, max_nodes, max_path;
    double step, radius, cell, ox, oy;
    unsigned char* ws;         // the caller's workspace: ws_row bytes per query
    long long ws_row;
    double* path;              // [n][max_path][2]
    int32_t* path_len;         // [n]
    int32_t* status;           // [n]
    int32_t* iterations;       // [n]
    int32_t* nodes;            // [n][2]
};

// One query's share of the workspace: the nodes' x, y (16 bytes each), their cost (8 bytes each), their parent (4 bytes each).
// Every part starts on a multiple of 8 bytes, the row on a multiple of 256.
__host__ __device__ inline long long sample_cost_offset(int max_nodes) { return (long long)max_nodes * 16; }
__host__ __device__ inline long long sample_parent_offset(int max_nodes) { return (long long)max_nodes * 24; }
__host__ __device__ inline long long sample_row_bytes(int max_nodes) { return ((long long)max_nodes * 28 + 255) & ~255ll; }

// The obstacle cells near the segment p1 -> p2: hybrid_range's box on each axis, row-major.
struct SampleBox { int c0, r0, wc, cnt; };
T2D_DEV SampleBox sample_box(double x1, double y1, double x2, double y2, double ox, double oy, double cell, int H, int W) {
    int c0, c1, r0, r1;
    hybrid_range(x2 < x1 ? x2 : x1, x2 > x1 ? x2 : x1, ox, cell, W, c0, c1);
    hybrid_range(y2 < y1 ? y2 : y1, y2 > y1 ? y2 : y1, oy, cell, H, r0, r1);
    const int wc = c1 - c0 + 1;
    return {c0, r0, wc, wc > 0 && r1 >= r0 ? wc * (r1 - r0 + 1) : 0};
}

// cell j of the box: does the segment touch it, if it is an obstacle
T2D_DEV bool sample_cell_hit(const SampleBox& b, int j, const double* weight, int W, double x1, double y1, double x2, double y2,
                             double ox, double oy, double cell) {
    const int r = b.r0 + j / b.wc, c = b.c0 + j % b.wc;
    const double w = weight[r * W + c];
    if (!(w != w || w == __builtin_huge_val())) return false;
    return hybrid_slab(x1, y1, x2, y2, ox + (double)c * cell, oy + (double)r * cell, cell / 2.0);
}

}  // namespace t2d
