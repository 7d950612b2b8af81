// t2d_sample_dev.h -- the pieces of the sampling planners (search/rrt.py: RRT.plan, search/rrt_star.py: RRTStar.plan and
// _choose_parent, search/rrt_connect.py: RRTConnect.plan, with the grid collision checker of the reference's tests/test_search.py)
// as device functions.  fp64 throughout, one rounding per operation; tests/sample_plan_ref.py states the same operations in
// Python.  The collision checker and the wave-wide argmin are t2d_gridplan_dev.h's.  DESIGN.md 4.23.
#pragma once
#include "t2d_gridplan_dev.h"
#include "t2d_rng.h"

namespace t2d {

enum { SAMPLE_RRT = 0, SAMPLE_RRT_STAR = 1, SAMPLE_RRT_CONNECT = 2 };
enum { SAMPLE_FOUND = 0, SAMPLE_MAX_ITER = 1, SAMPLE_TRUNCATED = 2, SAMPLE_OVERFLOW = 3, SAMPLE_INVALID = 4 };
constexpr int kSampleLdsNodes = 512;   // nodes whose x, y one query keeps in LDS: 8 KiB, twenty queries per CU

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

}  // namespace t2d
