// t2d_track_dev.h -- the arithmetic of the racing tile march (t2d_track.hip): does the ring of a lane tile touch the closed
// box of the car?  fp64 throughout, one rounding per operation (-ffp-contract=off is part of the build's contract);
// tests/track_ref.py states the same operations in numpy, in the same order.
//
// Replaces (reference, tactics2d v0.1.9rc3): `tile_shape.intersects(agent_pose) or tile_shape.contains(agent_pose)` of
// _RacingScenarioManager._locate_agent (envs/racing.py:273, :279), where tile_shape is a LinearRing (map/element/lane.py:
// 125-128: left side, then the right side reversed) and agent_pose the Polygon of Vehicle.get_pose.  A ring is its four
// EDGES: the predicate is "one of the four edges meets the closed box"; a car wholly inside a tile touches nothing.
#pragma once
#include <hip/hip_runtime.h>

namespace t2d {

// (ax, ay) x (bx, by): two products, one difference
__device__ __forceinline__ double track_cross(double ax, double ay, double bx, double by) { return ax * by - ay * bx; }

// The box Q (CCW, the vertex order of the event kernels' pose) against the tile ring V (four vertices in ring order, either
// winding, convex or not).  An edge P0 -> P1 of the ring and the closed convex box are disjoint exactly when a line separates
// them strictly, and in the plane the candidates are the four box edges and the edge's own line:
//   side[k][v] = (Q[k+1] - Q[k]) x (V[v] - Q[k])        < 0: vertex v strictly outside box edge k
//   s[i][k]    = (V[i+1] - V[i]) x (Q[k] - V[i])         all four > 0 or all four < 0: the box strictly on one side of edge i
// edge i touches = no box edge k with side[k][i] < 0 and side[k][i+1] < 0, and the s[i][.] not all of one strict sign.
// (A zero-length edge has s = 0 everywhere and is decided by the box edges alone: it is the point test.)
__device__ __forceinline__ bool track_touch(const double qx[4], const double qy[4], const double vx[4], const double vy[4]) {
    unsigned out[4];   // bit k: vertex v strictly outside box edge k
#pragma unroll
    for (int v = 0; v < 4; ++v) out[v] = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int k1 = (k + 1) & 3;
        const double ex = qx[k1] - qx[k], ey = qy[k1] - qy[k];
#pragma unroll
        for (int v = 0; v < 4; ++v) {
            const double side = track_cross(ex, ey, vx[v] - qx[k], vy[v] - qy[k]);
            out[v] |= side < 0.0 ? 1u << k : 0u;
        }
    }
    bool touch = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int i1 = (i + 1) & 3;
        const double dx = vx[i1] - vx[i], dy = vy[i1] - vy[i];
        bool all_pos = true, all_neg = true;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double s = track_cross(dx, dy, qx[k] - vx[i], qy[k] - vy[i]);
            all_pos = all_pos && s > 0.0;
            all_neg = all_neg && s < 0.0;
        }
        const bool separated = (out[i] & out[i1]) != 0u || all_pos || all_neg;
        touch = touch || !separated;
    }
    return touch;
}

// bits of mask word w (tiles 32 w .. 32 w + 31) that lie in the tile range [a, b), 0 <= a, b <= 2048
__device__ __forceinline__ uint32_t track_range_bits(int w, int a, int b) {
    const int lo = a - 32 * w, hi = b - 32 * w;
    const int l = lo < 0 ? 0 : lo, h = hi > 32 ? 32 : hi;
    if (h <= l) return 0u;
    const uint32_t upto_h = h >= 32 ? 0xffffffffu : (1u << h) - 1u;
    return upto_h & ~((1u << l) - 1u);   // (l < 32 here)
}

}  // namespace t2d
