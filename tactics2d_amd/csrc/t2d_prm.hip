// t2d_prm.hip -- the reference's probabilistic roadmap for n independent queries in one launch (prm_plan_kernel).  The formulas are
// t2d_prm_dev.h; what they restate is search/prm.py: PRM.plan with the grid collision checker the reference's tests pair with it.
// DESIGN.md 4.25.
#include <string>

#include "t2d_plan_host.h"
#include "t2d_prm_dev.h"

namespace t2d {

static_assert(PRM_FOUND == T2D_PRM_FOUND && PRM_NO_PATH == T2D_PRM_NO_PATH && PRM_TRUNCATED == T2D_PRM_TRUNCATED &&
              PRM_OVERFLOW == T2D_PRM_OVERFLOW && PRM_INVALID == T2D_PRM_INVALID, "t2d.h");
static_assert(kPrmMaxNodes == T2D_PRM_MAX_NODES && kPrmMaxK == T2D_PRM_MAX_K, "t2d.h");

namespace {

// One query per workgroup of four waves.  Every phase of PRM.plan is parallel over something else, and a barrier stands between
// two phases: (1) a node per thread draws its sample; (2) a node per thread scans all nodes out of LDS -- every lane reads the
// same address, a broadcast -- for its neighbours; (3) a candidate edge per LANE walks the obstacle cells of its own box; (4) a
// node per thread counts its surviving edges, a workgroup prefix sum gives them their places in the reference's order; (5) an
// edge per thread relaxes both directions into the next plane of g with an LDS 64-bit unsigned min -- doubles that are not
// negative order as their bit patterns do --, plane by plane until nothing changes, two more passes over the edges give every
// node its predecessor, and one lane walks back from the target.  Every branch around a barrier is taken by the whole workgroup.
__global__ __launch_bounds__(kPrmThreads) void prm_plan_kernel(PrmArgs a) {
    __shared__ double2 s_xy[kPrmMaxNodes];
    __shared__ unsigned long long s_g[kPrmMaxNodes], s_next[kPrmMaxNodes];
    __shared__ int s_cnt[kPrmMaxNodes], s_settled[kPrmMaxNodes];
    __shared__ int s_wave[kPrmThreads / 64];
    const int e = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const double inf = __builtin_huge_val();
    const unsigned long long inf_bits = 0x7ff0000000000000ull;

    const int H = a.hw[2 * e], W = a.hw[2 * e + 1];
    const double sx = a.start[2 * e], sy = a.start[2 * e + 1], tx = a.target[2 * e], ty = a.target[2 * e + 1];
    const double x_min = a.boundary[4 * e], x_max = a.boundary[4 * e + 1], y_min = a.boundary[4 * e + 2], y_max = a.boundary[4 * e + 3];
    const Stream stream{a.seed[e]};
    const int N = a.n_samples + 2, K = prm_degree(N, a.k);
    const bool by_radius = a.radius > 0.0;

    unsigned char* row = a.ws + (long long)e * a.ws_row;
    double2* g_xy = reinterpret_cast<double2*>(row);
    double* g_dist = reinterpret_cast<double*>(row + prm_dist_offset(N));
    double* g_cost = reinterpret_cast<double*>(row + prm_cost_offset(N));
    int* g_ij = reinterpret_cast<int*>(row + prm_ij_offset(N, a.k));
    int* g_cand = reinterpret_cast<int*>(row + prm_scratch_offset(N, a.k));
    const ObstacleGrid obstacles{a.weight + (size_t)e * (size_t)a.stride, H, W, a.ox, a.oy, a.cell};

    int status = -1, n_edges = 0, sweeps = 0, len = 0;
    {
        const auto within = [](double lo, double v, double hi) { return lo - kPrmBoundaryEps <= v && v <= hi + kPrmBoundaryEps; };
        if (plan_row_bad(sx, sy, tx, ty, x_min, x_max, y_min, y_max, H, W, a.stride) || x_min >= x_max || y_min >= y_max ||
            !within(x_min, sx, x_max) || !within(y_min, sy, y_max) || !within(x_min, tx, x_max) || !within(y_min, ty, y_max))
            status = PRM_INVALID;
    }
    if (status < 0) {
        // ---- 1. the nodes: start, target, then sample s from draws 2 s and 2 s + 1 ----
        for (int i = tid; i < N; i += kPrmThreads) {
            double x = i == 0 ? sx : tx, y = i == 0 ? sy : ty;
            if (i >= 2) {
                const uint64_t s = (uint64_t)(i - 2);
                x = x_min + (x_max - x_min) * stream.peek(2ull * s);
                y = y_min + (y_max - y_min) * stream.peek(2ull * s + 1ull);
            }
            s_xy[i] = make_double2(x, y);
            g_xy[i] = make_double2(x, y);
        }
        __syncthreads();
        // ---- 2. node i's neighbours, of which only j > i become candidates, in the neighbour order ----
        bool over = false;
        for (int i = tid; i < N; i += kPrmThreads) {
            const double2 p = s_xy[i];
            int* out = g_cand + i * K;
            int c = 0;
            if (by_radius) {
                int deg = 0;
                for (int j = 0; j < N; ++j) {
                    const double2 q = s_xy[j];
                    const double dx = q.x - p.x, dy = q.y - p.y;
                    if (j != i && __builtin_sqrt(dx * dx + dy * dy) <= a.radius) {
                        if (j > i && c < K) out[c++] = j;
                        ++deg;
                    }
                }
                over = over || deg > a.k;
            } else {
                PrmNearest best;
                best.clear();
                for (int j = 0; j < N; ++j) {
                    const double2 q = s_xy[j];
                    const double dx = q.x - p.x, dy = q.y - p.y, d2 = dx * dx + dy * dy;
                    if (best.admits(d2, j)) best.insert(d2, j);
                }
                // the first K + 1 = min(k_nearest + 1, N) entries; i itself is among them unless K + 1 coincident nodes of a
                // smaller index are, and then no entry is above i
#pragma unroll
                for (int t = 0; t <= kPrmMaxK; ++t) {
                    if (t <= K && best.id[t] > i && c < K) out[c++] = best.id[t];
                }
            }
            s_cnt[i] = c;
        }
        if (__syncthreads_or(over)) status = PRM_OVERFLOW;
    }
    if (status < 0) {
        // ---- 3. a candidate per lane against the obstacle cells of its box; a hit empties its place ----
        const int E = N * K;
        for (int w = tid; w < E; w += kPrmThreads) {
            const int i = w / K, t = w - i * K;
            if (t < s_cnt[i]) {
                const double2 p = s_xy[i], q = s_xy[g_cand[w]];
                if (obstacles.lane_seg_hit(p.x, p.y, q.x, q.y)) g_cand[w] = -1;
            }
        }
        __syncthreads();
        // ---- 4. the surviving edges in the reference's order: i ascending, within i the neighbour order ----
        for (int i0 = 0; i0 < N; i0 += kPrmThreads) {
            const int i = i0 + tid;
            int c = 0;
            if (i < N) {
                for (int t = 0; t < s_cnt[i]; ++t) c += g_cand[i * K + t] >= 0;
            }
            int total;
            const int before = plan_wave_excl_scan(c, total);
            if (lane == 0) s_wave[wave] = total;
            __syncthreads();
            int at = n_edges + before, all = 0;
            for (int v = 0; v < kPrmThreads / 64; ++v) {
                if (v < wave) at += s_wave[v];
                all += s_wave[v];
            }
            if (i < N) {
                const double2 p = s_xy[i];
                for (int t = 0; t < s_cnt[i]; ++t) {
                    const int j = g_cand[i * K + t];
                    if (j < 0) continue;
                    const double2 q = s_xy[j];
                    const double dx = p.x - q.x, dy = p.y - q.y;
                    g_ij[2 * at] = i;
                    g_ij[2 * at + 1] = j;
                    g_cost[at] = __builtin_sqrt(dx * dx + dy * dy);
                    ++at;
                }
            }
            n_edges += all;
            __syncthreads();
        }
        // ---- 5. the min-plus fixed point: every sweep reads one plane and lowers the other ----
        for (int i = tid; i < N; i += kPrmThreads) {
            s_g[i] = s_next[i] = i == 0 ? 0ull : inf_bits;
            s_settled[i] = 0;   // the sweep that gave the node the value it has: 0 for the start
        }
        __syncthreads();
        for (;;) {
            bool changed = false;
            const auto relax = [&](int u, int v, double w) {
                const double cand = __longlong_as_double((long long)s_g[u]) + w;
                if (cand < __longlong_as_double((long long)s_g[v])) {
                    const unsigned long long bits = (unsigned long long)__double_as_longlong(cand);
                    if (bits < atomicMin(&s_next[v], bits)) changed = true;
                }
            };
            for (int k = tid; k < n_edges; k += kPrmThreads) {
                const int i = g_ij[2 * k], j = g_ij[2 * k + 1];
                const double w = g_cost[k];
                relax(i, j, w);
                relax(j, i, w);
            }
            ++sweeps;
            if (!__syncthreads_or(changed)) break;
            for (int i = tid; i < N; i += kPrmThreads) {
                if (s_next[i] != s_g[i]) s_settled[i] = sweeps;
                s_g[i] = s_next[i];
            }
            __syncthreads();
        }
        // ---- the predecessor of v: the smallest (g[u], u) among the neighbours with fl(g[u] + w) == g[v] that precede v: g[u] <
        // g[v], or, at equal g (an edge of cost 0 between coincident nodes), u settled in an earlier sweep than v.  Whoever gave v
        // its value precedes it, so every walk ends at the start.  First the smallest such g[u] (into s_next), then the smallest
        // u that has it (into s_cnt) ----
        for (int i = tid; i < N; i += kPrmThreads) {
            s_next[i] = ~0ull;
            s_cnt[i] = 0x7fffffff;
            g_dist[i] = __longlong_as_double((long long)s_g[i]);
        }
        __syncthreads();
        const auto precedes = [&](int u, int v, double w) {
            const double gu = __longlong_as_double((long long)s_g[u]), gv = __longlong_as_double((long long)s_g[v]);
            return gv < inf && gu + w == gv && (gu < gv || (gu == gv && s_settled[u] < s_settled[v]));
        };
        for (int k = tid; k < n_edges; k += kPrmThreads) {
            const int i = g_ij[2 * k], j = g_ij[2 * k + 1];
            const double w = g_cost[k];
            if (precedes(i, j, w)) atomicMin(&s_next[j], s_g[i]);
            if (precedes(j, i, w)) atomicMin(&s_next[i], s_g[j]);
        }
        __syncthreads();
        for (int k = tid; k < n_edges; k += kPrmThreads) {
            const int i = g_ij[2 * k], j = g_ij[2 * k + 1];
            const double w = g_cost[k];
            if (precedes(i, j, w) && s_g[i] == s_next[j]) atomicMin(&s_cnt[j], i);
            if (precedes(j, i, w) && s_g[j] == s_next[i]) atomicMin(&s_cnt[i], j);
        }
        __syncthreads();
        // ---- the path, start first: one lane walks back from node 1; (g, sweep) falls at every step, so no node comes twice ----
        if (tid == 0) {
            int l = 0;
            if (s_g[1] < inf_bits) {
                for (int v = 1; v != 0x7fffffff && l < N; v = s_cnt[v]) ++l;
                double* out = a.path + (size_t)e * (size_t)a.max_path * 2;
                int k = l - 1;
                for (int v = 1; k >= 0; v = s_cnt[v], --k) {
                    if (k < a.max_path) {
                        const double2 p = s_xy[v];
                        out[2 * k] = p.x;
                        out[2 * k + 1] = p.y;
                    }
                }
            }
            s_wave[0] = l;
        }
        __syncthreads();
        len = s_wave[0];
        status = len == 0 ? PRM_NO_PATH : (len > a.max_path ? PRM_TRUNCATED : PRM_FOUND);
    }
    plan_path_tail<2, kPrmThreads>(a.path + (size_t)e * (size_t)a.max_path * 2, len, a.max_path, tid);
    if (tid == 0) {
        a.path_len[e] = len;
        a.status[e] = status;
        a.n_edges[e] = n_edges;
        a.sweeps[e] = sweeps;
    }
}

}  // namespace
}  // namespace t2d

extern "C" int64_t t2d_prm_plan_workspace_bytes(int32_t n, int32_t n_samples, int32_t k_or_degree) {
    if (n < 0 || n_samples < 1 || n_samples + 2 > T2D_PRM_MAX_NODES || k_or_degree < 1) return -1;
    return (int64_t)n * (int64_t)t2d::prm_row_bytes(n_samples + 2, k_or_degree);
}

extern "C" int t2d_prm_plan(int32_t device_id, int32_t n, const double* weight_dev, const int32_t* hw_dev, int32_t max_cells,
                            const double* start_dev, const double* target_dev, const double* boundary_dev, const uint64_t* seed_dev,
                            int32_t n_samples, int32_t k_nearest, double connection_radius, int32_t max_degree, double cell_size,
                            double origin_x, double origin_y, int32_t max_path, void* workspace_dev, int64_t workspace_bytes,
                            double* path_dev, int32_t* path_len_dev, int32_t* status_dev, int32_t* n_edges_dev, int32_t* sweeps_dev,
                            void* hip_stream) {
    using namespace t2d;
    host::PlanEntry entry("t2d_prm_plan");
    if (n < 0 || max_cells < 1 || max_path < 0) return entry.invalid("n >= 0, max_cells >= 1 and max_path >= 0");
    if (n_samples < 1 || n_samples + 2 > T2D_PRM_MAX_NODES) return entry.invalid("n_samples must be in 1 .. T2D_PRM_MAX_NODES - 2");
    if (!(connection_radius >= 0.0 && connection_radius <= kPlanXYLimit))
        return entry.invalid("connection_radius must be 0 (k-nearest mode) or positive and finite");
    const bool by_radius = connection_radius > 0.0;
    if (!by_radius && (k_nearest < 1 || k_nearest > T2D_PRM_MAX_K)) return entry.invalid("k_nearest must be in 1 .. T2D_PRM_MAX_K");
    if (by_radius && max_degree < 1) return entry.invalid("max_degree must be at least 1");
    if (int rc = entry.cell_origin(cell_size, origin_x, origin_y)) return rc;
    entry.required(7u, weight_dev, start_dev, target_dev, boundary_dev, seed_dev);
    entry.required(3u, hw_dev, path_len_dev, status_dev, n_edges_dev, sweeps_dev);
    if (max_path > 0) entry.required(7u, path_dev);
    if (int rc = entry.workspace(workspace_dev).pointers()) return rc;
    const int k = by_radius ? max_degree : k_nearest;
    if (int rc = entry.workspace_bytes(workspace_bytes, t2d_prm_plan_workspace_bytes(n, n_samples, k))) return rc;
    const PrmArgs a{weight_dev, hw_dev, start_dev, target_dev, boundary_dev, seed_dev,
                    max_cells, n_samples, k, max_path, by_radius ? connection_radius : 0.0, cell_size, origin_x, origin_y,
                    static_cast<unsigned char*>(workspace_dev), prm_row_bytes(n_samples + 2, k),
                    path_dev, path_len_dev, status_dev, n_edges_dev, sweeps_dev};
    return entry.launch(device_id, n, [&] { hipLaunchKernelGGL(prm_plan_kernel, dim3((unsigned)n), dim3(kPrmThreads), 0, (hipStream_t)hip_stream, a); });
}
