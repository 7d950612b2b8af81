// t2d_track.hip -- tile progress of every racing env in one launch (t2d_track_progress, include/t2d.h).
//
// Replaces (reference, tactics2d v0.1.9rc3):
//   _RacingScenarioManager._locate_agent   envs/racing.py:261-301   which tiles the car touches, which count as visited
//   _RacingScenarioManager.check_status    envs/racing.py:339-369   time-exceeded / no-action / out-of-bound / completed
//   RacingEnv._get_rewards                 envs/racing.py:121-139
//
// One wave per env (four envs per workgroup, nothing shared between them).  Round c of the march: lane j tests tile
// (tile_visiting + j + 64 c) % n_tile of the env's track against the car's box (t2d_track_dev.h); one ballot gives the first
// touched tile and the first untouched one behind it (tiles whose bounding box is more than a metre from the car's skip the
// predicate: they cannot touch).  A car on the track ends in round 0; only a car that touches nothing
// reads the whole ring (or the whole window of the forward rule).  Tiles are read from the shared track set (32 B per lane,
// two 16-byte loads; a reference track is 14 KB: L2-resident).  The visited mask is 64 words per env: lane w owns word w, sets
// its bits of the newly visited range itself, and the count is a popcount summed over the wave.  No LDS, no atomics, vector
// stores only.
#include "t2d_math.h"
#include "t2d_pool.h"
#include "t2d_track_dev.h"

namespace t2d {

namespace {

constexpr int kBlock = 256;
constexpr int kWords = T2D_MAX_TRACK_TILES / 32;   // mask words per env
static_assert(kWords == 64, "lane w of the env's wave owns mask word w");

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

__global__ __launch_bounds__(kBlock) void track_progress_kernel(PoolView pv, TrackView tv, int write_status) {
    const int lane = threadIdx.x & 63;
    const int e = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    if (e >= pv.n_env) return;   // (wave-uniform)

    // ---- everything that does not depend on anything else, first -------------------------------------------------------
    const int set = tv.set_of_env[e];
    const uchar4 prev = reinterpret_cast<const uchar4*>(tv.status)[e];
    const bool restart = (prev.z | prev.w) != 0;   // the previous launch ended this env's episode
    const int visiting0 = tv.visiting[e], start_visiting = tv.start_visiting[e];
    const uint32_t word_cur = tv.mask[(size_t)e * kWords + lane], word_start = tv.start_mask[(size_t)e * kWords + lane];
    const int idx = e * pv.A + tv.ego_index;
    const uint32_t ids = pv.ids[idx];
    const float fx = pv.x[idx], fy = pv.y[idx], fh = pv.heading[idx];
    const uchar4 pst = reinterpret_cast<const uchar4*>(pv.status)[e];
    const uint32_t flags = pv.flags[idx];
    const int cnt = pv.cnt_step[e];
    const int t0 = tv.set_start[set], n = tv.n_tile[set];
    const float4* tiles = reinterpret_cast<const float4*>(tv.tiles) + 2 * (size_t)t0;

    const int visiting = restart ? start_visiting : visiting0;
    uint32_t word = restart ? word_start : word_cur;

    // ---- the car's box: Vehicle.get_pose with the event kernels' expressions --------------------------------------------
    const int type = (ids >> kIdsTypeShift) & 0xff;
    const bool boxed = ((ids >> kIdsActiveShift) & 0xffu) && (int)pv.params[T2D_P_SHAPE * T2D_MAX_TYPES + type] == T2D_SHAPE_OBB &&
                       __builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(fh);
    double qx[4], qy[4];
    {
        const double L = pv.params[T2D_P_LENGTH * T2D_MAX_TYPES + type], W = pv.params[T2D_P_WIDTH * T2D_MAX_TYPES + type];
        const double cx = (double)fx, cy = (double)fy;
        double s, c;
        sincos_det(boxed ? (double)fh : 0.0, s, c);
        const double hl = 0.5 * L, hw = 0.5 * W;
        const double lx[4] = {hl, hl, -hl, -hl};
        const double ly[4] = {-hw, hw, hw, -hw};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            qx[k] = c * lx[k] - s * ly[k] + cx;
            qy[k] = s * lx[k] + c * ly[k] + cy;
        }
    }

    // the box's bounding box widened by kFar: a tile whose own bounding box lies beyond it cannot touch (the predicate's
    // rounding errors are of the order of 1e-13 m at these coordinates, kFar is a metre), so the 32 cross products are spent
    // on the tiles near the car only -- in the rounds of a march that finds nothing, on none
    constexpr double kFar = 1.0;
    double blo_x = qx[0], bhi_x = qx[0], blo_y = qy[0], bhi_y = qy[0];
#pragma unroll
    for (int k = 1; k < 4; ++k) {
        blo_x = qx[k] < blo_x ? qx[k] : blo_x; bhi_x = qx[k] > bhi_x ? qx[k] : bhi_x;
        blo_y = qy[k] < blo_y ? qy[k] : blo_y; bhi_y = qy[k] > bhi_y ? qy[k] : bhi_y;
    }
    blo_x -= kFar; bhi_x += kFar; blo_y -= kFar; bhi_y += kFar;

    // ---- the march: offsets 0 .. limit - 1 behind tile_visiting, 64 per round ------------------------------------------
    const bool whole = tv.rule == T2D_TRACK_RULE_REFERENCE || tv.max_advance <= 0 || tv.max_advance >= n;
    const int limit = whole ? n : tv.max_advance + 1;
    int j0 = -1, j1 = -1;   // the run of touched tiles: offsets [j0, j1)
    if (boxed) {            // (wave-uniform: a car without a box touches nothing)
        for (int base = 0; base < limit; base += 64) {
            const int off = base + lane;
            bool touched = false;
            if (off < limit) {
                int t = visiting + off;
                t -= t >= n ? n : 0;
                const float4 a = tiles[2 * t], b = tiles[2 * t + 1];
                const double vx[4] = {(double)a.x, (double)a.z, (double)b.x, (double)b.z};
                const double vy[4] = {(double)a.y, (double)a.w, (double)b.y, (double)b.w};
                const float tlo_x = fminf(fminf(a.x, a.z), fminf(b.x, b.z)), thi_x = fmaxf(fmaxf(a.x, a.z), fmaxf(b.x, b.z));
                const float tlo_y = fminf(fminf(a.y, a.w), fminf(b.y, b.w)), thi_y = fmaxf(fmaxf(a.y, a.w), fmaxf(b.y, b.w));
                const bool near = (double)thi_x >= blo_x && (double)tlo_x <= bhi_x && (double)thi_y >= blo_y && (double)tlo_y <= bhi_y;
                if (near) touched = track_touch(qx, qy, vx, vy);
            }
            const unsigned long long hit = __ballot(touched);
            unsigned long long miss = ~hit;   // (never empty past the limit: those lanes report no touch)
            if (j0 < 0) {
                if (hit == 0ull) continue;
                const int f = __builtin_ctzll(hit);
                j0 = base + f;
                miss &= ~0ull << f;
            }
            if (miss != 0ull) {
                j1 = base + __builtin_ctzll(miss);
                break;
            }
        }
        if (j0 >= 0 && j1 < 0) j1 = limit;   // (the run reached the end of the last, full round)
    }

    // ---- visited tiles, tile_visiting (racing.py:290-301) --------------------------------------------------------------
    int visiting_new = visiting;
    if (j0 >= 0) {
        // tiles between tile_visiting and the run, then the run: offsets [1, j1), and offset 0 with them when the run starts there.
        // The reference's gap loop starts at offset 1 and stops at the first member of the run: when the run is [tile_visiting]
        // alone it goes all the way round.  (The forward rule fills strictly between tile_visiting and the run: no such case.)
        const bool all = tv.rule == T2D_TRACK_RULE_REFERENCE && j0 == 0 && j1 == 1;
        const int lo = j0 == 0 ? 0 : 1;
        int a = visiting + lo;
        a -= a >= n ? n : 0;
        const int len = all ? n : j1 - lo;   // (<= n)
        const int b = a + len;
        word |= track_range_bits(lane, a, b < n ? b : n);
        if (b > n) word |= track_range_bits(lane, 0, b - n);
        visiting_new = visiting + j1 - 1;
        visiting_new -= visiting_new >= n ? n : 0;
    }
    const int count = wave_sum(__builtin_popcount(word));

    // ---- status (racing.py:339-369) from what the step launch left, reward (racing.py:121-139) -------------------------
    int scen = T2D_SCENARIO_NORMAL, traf = T2D_TRAFFIC_NORMAL;
    if (pst.x == T2D_SCENARIO_TIME_EXCEEDED) scen = T2D_SCENARIO_TIME_EXCEEDED;
    else if (pst.y == T2D_TRAFFIC_NO_ACTION_QUIRK) traf = T2D_TRAFFIC_NO_ACTION_QUIRK;   // racing.py:351
    else if (pst.x == T2D_SCENARIO_OUT_BOUND) traf = T2D_SCENARIO_OUT_BOUND;             // racing.py:356 (a ScenarioStatus in traffic_status)
    else if (tv.check_off_road && (flags & T2D_FLAG_OFF_LANE)) traf = T2D_TRAFFIC_OFF_LANE;   // build-defined (the reference's detector is a stub)
    else if (count == n) scen = T2D_SCENARIO_COMPLETED;
    double rd;
    if (scen == T2D_SCENARIO_TIME_EXCEEDED) rd = -1.0;
    else if (traf == T2D_SCENARIO_OUT_BOUND || traf == T2D_TRAFFIC_OFF_LANE) rd = -5.0;
    else if (scen == T2D_SCENARIO_COMPLETED) rd = ((double)n - 0.1 * (double)cnt) / (double)n * 100.0;
    else {
        const double time_penalty = -0.1 * (double)cnt, tile_reward = 0.1 * (double)count;
        rd = time_penalty + tile_reward;
    }
    const bool terminated = scen == T2D_SCENARIO_COMPLETED;
    const bool truncated = !terminated && (scen != T2D_SCENARIO_NORMAL || traf != T2D_TRAFFIC_NORMAL);

    tv.mask[(size_t)e * kWords + lane] = word;
    if (lane == 0) {
        uchar4 st;
        st.x = (unsigned char)scen; st.y = (unsigned char)traf; st.z = terminated; st.w = truncated;
        const float r = (float)rd;
        tv.visiting[e] = visiting_new;
        tv.num_visited[e] = count;
        reinterpret_cast<uchar4*>(tv.status)[e] = st;
        tv.reward[e] = r;
        if (write_status) {
            reinterpret_cast<uchar4*>(pv.status)[e] = st;
            pv.reward[e] = r;
        }
    }
}

}  // namespace

hipError_t launch_track_progress(const PoolView& v, const TrackView& tv, int write_status, hipStream_t s) {
    const int per_block = kBlock / 64;
    hipLaunchKernelGGL(track_progress_kernel, dim3((v.n_env + per_block - 1) / per_block), dim3(kBlock), 0, s, v, tv, write_status);
    return hipGetLastError();
}

}  // namespace t2d
