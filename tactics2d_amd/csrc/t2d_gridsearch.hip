// t2d_gridsearch.hip -- the cost-to-go field and the shortest path of n weighted obstacle grids in one launch
// (grid_dijkstra_kernel).  The formulas are t2d_gridsearch_dev.h; what they restate is search/dijkstra.py over the graph of
// search/graph_utils.py: grid_to_csr.  DESIGN.md 4.21.
#include <cmath>
#include <string>

#include "t2d_gridsearch_dev.h"
#include "t2d_plan_host.h"

namespace t2d {

static_assert(GRID_FOUND == T2D_GRID_FOUND && GRID_NO_PATH == T2D_GRID_NO_PATH && GRID_TRUNCATED == T2D_GRID_TRUNCATED &&
              GRID_INVALID == T2D_GRID_INVALID && GRID_FIELD_ONLY == T2D_GRID_FIELD_ONLY, "t2d.h");
static_assert(kGridMaxCells == T2D_GRID_MAX_CELLS, "t2d.h");

namespace {

// One grid per workgroup, CELLS / THREADS = 4 cells per lane (cell v of lane t: t, t + THREADS, ...: consecutive lanes read
// consecutive 8-byte LDS words).  A round of relaxation is Jacobi's: every lane computes the new value of its cells from the
// plane as it stands, a barrier, every lane stores what improved -- no cell is read while it is written, and the number of
// rounds does not depend on how the waves are scheduled.  The fixed point is the reference's g_score whatever the order (DESIGN.md
// 4.21); it is reached after at most as many rounds as the longest shortest path has cells, which the loop also bounds.
template <int CELLS, int THREADS>
__global__ __launch_bounds__(THREADS) void grid_dijkstra_kernel(GridArgs a) {
    constexpr int CPT = CELLS / THREADS;
    __shared__ double s_g[CELLS];
    __shared__ double s_w[CELLS];
    __shared__ int s_flag[2], s_bad, s_len;
    const int e = blockIdx.x, tid = threadIdx.x;
    const int H = a.hw[2 * e], W = a.hw[2 * e + 1], src = a.source[e], tgt = a.target[e];
    const long long cells = (long long)H * (long long)W;
    const bool shape_ok = H > 0 && W > 0 && cells <= (long long)a.stride && cells <= (long long)CELLS;
    const int n = shape_ok ? (int)cells : 0;
    bool ok = shape_ok && src >= 0 && src < n && tgt >= -1 && tgt < n;
    if (tid == 0) s_flag[0] = s_flag[1] = s_bad = s_len = 0;
    __syncthreads();

    const double* w_in = a.weight + (size_t)e * a.stride;
    double wv[CPT];
    int mask[CPT];
    bool negative = false;
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int v = tid + k * THREADS;
        wv[k] = grid_inf();
        mask[k] = 0;
        if (v < n) {
            double x = w_in[v];
            if (x != x) x = grid_inf();   // NaN is an obstacle, as in grid_to_csr
            negative = negative || x < 0.0;
            wv[k] = x;
            mask[k] = grid_neighbour_mask(v / W, v % W, H, W, a.diagonals);
            s_w[v] = x;
            s_g[v] = ok && v == src ? 0.0 : grid_inf();
        }
    }
    if (negative) s_bad = 1;
    __syncthreads();
    if (ok && (s_bad || !(s_w[src] < grid_inf()) || (tgt >= 0 && !(s_w[tgt] < grid_inf())))) ok = false;

    double* g_out = a.g + (size_t)e * a.stride;
    int32_t* path_out = a.path + (size_t)e * a.max_path;
    if (!ok) {   // (the whole workgroup: every term above is the same for all its lanes)
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int v = tid + k * THREADS;
            if (v < n) g_out[v] = grid_inf();
        }
        for (int i = tid; i < a.max_path; i += THREADS) path_out[i] = -1;
        if (tid == 0) {
            a.path_len[e] = 0;
            a.status[e] = GRID_INVALID;
            a.sweeps[e] = 0;
        }
        return;
    }

    int round = 0;
    for (;;) {
        double best[CPT];
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int v = tid + k * THREADS;
            best[k] = v < n ? grid_relax(s_g, s_w, v, W, mask[k], wv[k], a.mult) : 0.0;
        }
        __syncthreads();   // every read of this round is done
        bool changed = false;
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int v = tid + k * THREADS;
            if (v < n && best[k] < s_g[v]) {
                s_g[v] = best[k];
                changed = true;
            }
        }
        // the flag of round r is slot r & 1; the other slot was last read before this round's first barrier
        if (tid == 0) s_flag[(round + 1) & 1] = 0;
        if (changed) s_flag[round & 1] = 1;
        __syncthreads();
        const bool again = s_flag[round & 1] != 0;
        ++round;
        if (!again || round > n) break;
    }

    const bool walk = tgt >= 0 && s_g[tgt] < grid_inf();
    int pred[CPT];
#pragma unroll
    for (int k = 0; k < CPT; ++k) {
        const int v = tid + k * THREADS;
        pred[k] = walk && v < n && v != src ? grid_pred(s_g, s_w, v, W, mask[k], wv[k], a.mult) : -1;
        if (v < n) g_out[v] = s_g[v];
    }
    int len = 0;
    if (walk) {
        // both planes are dead now: the predecessors go where the weights were, the chain target -> source where g was
        __syncthreads();
        int* s_pred = reinterpret_cast<int*>(s_w);
        int* s_chain = reinterpret_cast<int*>(s_g);
#pragma unroll
        for (int k = 0; k < CPT; ++k) {
            const int v = tid + k * THREADS;
            if (v < n) s_pred[v] = pred[k];
        }
        __syncthreads();
        if (tid == 0) {
            int m = 0, cur = tgt;
            for (;;) {
                s_chain[m++] = cur;
                if (cur == src) break;
                const int p = s_pred[cur];
                if (p < 0 || m >= n) {   // (a dead end: only where a sum absorbed its edge)
                    m = 0;
                    break;
                }
                cur = p;
            }
            s_len = m;
        }
        __syncthreads();
        len = s_len;
        for (int i = tid; i < a.max_path; i += THREADS) path_out[i] = i < len ? s_chain[len - 1 - i] : -1;
    } else {
        for (int i = tid; i < a.max_path; i += THREADS) path_out[i] = -1;
    }
    if (tid == 0) {
        a.path_len[e] = len;
        a.status[e] = tgt < 0 ? GRID_FIELD_ONLY : (len == 0 ? GRID_NO_PATH : (len <= a.max_path ? GRID_FOUND : GRID_TRUNCATED));
        a.sweeps[e] = round;
    }
}

}  // namespace
}  // namespace t2d

extern "C" int t2d_grid_dijkstra(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, const int32_t* source_dev,
                                 const int32_t* target_dev, int32_t max_cells, int32_t connectivity, double diagonal_cost_multiplier,
                                 int32_t max_path, double* g_dev, int32_t* path_dev, int32_t* path_len_dev, int32_t* status_dev,
                                 int32_t* sweeps_dev, void* hip_stream) {
    using namespace t2d;
    host::PlanEntry entry("t2d_grid_dijkstra");
    if (n < 0 || max_cells < 1 || max_path < 0 || (connectivity != 4 && connectivity != 8))
        return entry.invalid("n >= 0, max_cells >= 1, max_path >= 0 and connectivity 4 or 8");
    if (!std::isfinite(diagonal_cost_multiplier) || diagonal_cost_multiplier < 0.0)
        return entry.invalid("diagonal_cost_multiplier must be finite and not negative");
    entry.required(7u, weight_dev, g_dev).required(3u, hw_dev, source_dev, target_dev, path_len_dev, status_dev, sweeps_dev);
    if (max_path > 0) entry.required(3u, path_dev);
    if (int rc = entry.pointers()) return rc;
    if (int rc = entry.grid_cap(max_cells, "two fp64 planes in LDS")) return rc;
    const GridArgs a{weight_dev, hw_dev, source_dev, target_dev, diagonal_cost_multiplier, max_cells, connectivity == 8, max_path,
                     g_dev, path_dev, path_len_dev, status_dev, sweeps_dev};
    return entry.launch(device_id, n, [&] {
        hipStream_t s = (hipStream_t)hip_stream;
        if (max_cells <= kGridSmallCells)
            hipLaunchKernelGGL((grid_dijkstra_kernel<kGridSmallCells, 256>), dim3((unsigned)n), dim3(256), 0, s, a);
        else
            hipLaunchKernelGGL((grid_dijkstra_kernel<kGridMaxCells, 1024>), dim3((unsigned)n), dim3(1024), 0, s, a);
    });
}
