// t2d_prm_dev.h -- the pieces of the probabilistic roadmap (search/prm.py: PRM.plan, with the grid collision checker of the
// reference's tests/test_search.py) as device functions.  fp64 throughout, one rounding per operation; tests/prm_ref.py states the
// same operations in Python.  The collision checker and the wave's prefix sum are t2d_gridplan_dev.h's, the stream is t2d_rng.h's.
// DESIGN.md 4.25.
#pragma once
#include "t2d_gridplan_dev.h"
#include "t2d_rng.h"

namespace t2d {

enum { PRM_FOUND = 0, PRM_NO_PATH = 1, PRM_TRUNCATED = 2, PRM_OVERFLOW = 3, PRM_INVALID = 4 };
constexpr int kPrmMaxNodes = 1024;   // start, target and the samples of one query: x, y in 16 KiB of LDS, two planes of g in 16 KiB, two words each in 8 KiB
constexpr int kPrmMaxK = 16;         // k_nearest: the sorted list of k + 1 (d2, index) lives in registers
constexpr int kPrmThreads = 256;     // one query per workgroup of four waves
constexpr double kPrmBoundaryEps = 1e-9;

// The arguments of one launch (t2d_prm_plan), checked by the entry point.
struct PrmArgs {
    const double* weight;      // [n][stride]
    const int32_t* hw;         // [n][2]
    const double* start;       // [n][2]
    const double* target;      // [n][2]
    const double* boundary;    // [n][4]
    const uint64_t* seed;      // [n]
    int stride, n_samples, k, max_path;   // k: k_nearest, or max_degree in radius mode
    double radius, cell, ox, oy;          // radius 0: k-nearest mode
    unsigned char* ws;         // the caller's workspace: ws_row bytes per query
    long long ws_row;
    double* path;              // [n][max_path][2]
    int32_t* path_len;         // [n]
    int32_t* status;           // [n]
    int32_t* n_edges;          // [n]
    int32_t* sweeps;           // [n]
};

// One query's share of the workspace, for N = n_samples + 2 nodes of at most K = min(k, N - 1) kept neighbours each, so at most
// E = N * K edges: the nodes' x, y f64 [N][2]; dist f64 [N]; edge_cost f64 [E]; edge_ij i32 [E][2]; scratch i32 [E] (the candidate
// lists).  Every part starts on a multiple of 8 bytes, the row on a multiple of 256.
__host__ __device__ inline int prm_degree(int n_nodes, int k) { return k < n_nodes - 1 ? k : n_nodes - 1; }
__host__ __device__ inline long long prm_max_edges(int n_nodes, int k) { return (long long)n_nodes * prm_degree(n_nodes, k); }
__host__ __device__ inline long long prm_dist_offset(int n_nodes) { return (long long)n_nodes * 16; }
__host__ __device__ inline long long prm_cost_offset(int n_nodes) { return (long long)n_nodes * 24; }
__host__ __device__ inline long long prm_ij_offset(int n_nodes, int k) { return prm_cost_offset(n_nodes) + prm_max_edges(n_nodes, k) * 8; }
__host__ __device__ inline long long prm_scratch_offset(int n_nodes, int k) { return prm_cost_offset(n_nodes) + prm_max_edges(n_nodes, k) * 16; }
__host__ __device__ inline long long prm_row_bytes(int n_nodes, int k) {
    return (prm_cost_offset(n_nodes) + prm_max_edges(n_nodes, k) * 20 + 255) & ~255ll;
}

// The sorted list of the kPrmMaxK + 1 smallest (d2, index) seen so far: one compare-exchange per entry, every index a constant
// after unrolling, so the list stays in registers.  The order is the total order (d2, index).
struct PrmNearest {
    double d[kPrmMaxK + 1];
    int id[kPrmMaxK + 1];
    T2D_DEV void clear() {
#pragma unroll
        for (int t = 0; t <= kPrmMaxK; ++t) {
            d[t] = __builtin_huge_val();
            id[t] = 0x7fffffff;
        }
    }
    T2D_DEV bool admits(double cd, int cj) const { return cd < d[kPrmMaxK] || (cd == d[kPrmMaxK] && cj < id[kPrmMaxK]); }
    T2D_DEV void insert(double cd, int cj) {
#pragma unroll
        for (int t = 0; t <= kPrmMaxK; ++t) {
            const bool lt = cd < d[t] || (cd == d[t] && cj < id[t]);
            const double td = d[t];
            const int ti = id[t];
            d[t] = lt ? cd : td;
            id[t] = lt ? cj : ti;
            cd = lt ? td : cd;
            cj = lt ? ti : cj;
        }
    }
};

}  // namespace t2d
