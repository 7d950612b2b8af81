// t2d_route_dev.h -- the arithmetic of the off-route detector (t2d_route.hip): squared distance of a point to one segment of a
// polyline, and the running minimum over the segments in vertex order.  fp64 throughout, one rounding per operation
// (-ffp-contract=off is part of the build's contract); tests/route_ref.py states the same operations in numpy.
//
// Replaces (reference, tactics2d v0.1.9rc3): OffRoute.update  traffic/event_detection/off_route.py:24-34
// (`route.distance(location) > threshold`).
#pragma once
#include <hip/hip_runtime.h>

namespace t2d {

// squared distance of P to the segment A -> B.  A zero-length segment has t = 0 and takes the first branch.
__device__ __forceinline__ double route_seg_d2(double ax, double ay, double bx, double by, double px, double py) {
    const double ux = bx - ax, uy = by - ay, wx = px - ax, wy = py - ay;
    const double L2 = ux * ux + uy * uy;
    const double t = wx * ux + wy * uy;
    if (t <= 0.0) return wx * wx + wy * wy;
    if (t >= L2) {
        const double vx = px - bx, vy = py - by;
        return vx * vx + vy * vy;
    }
    const double c = wx * uy - wy * ux;
    return (c * c) / L2;
}

// the verdict of one participant from the minimum over its route's segments (strict `<` in vertex order: the first minimum
// wins; a segment whose d2 is NaN never becomes the minimum)
__device__ __forceinline__ void route_verdict(double d2min, float thr, float* dist, uint8_t* off) {
    const double d = __builtin_sqrt(d2min);
    *dist = (float)d;
    *off = d > (double)thr ? 1 : 0;
}

// The projection of P = (x, y) onto one route of a set staged in LDS (lv = the set's vertices as fp32 pairs, k0 / k1 = the
// route's first vertex and one past its last): the measurement of t2d_pid_actions and t2d_pursuit_actions (include/t2d.h;
// tests/pid_ref.py `measure`).  route_seg_d2's operations over the segments in vertex order with zero-length segments skipped,
// the first strict minimum wins.  seg = -1: the route has no segment of non-zero length.
struct RouteMeasure {
    double d2min;        // squared distance to the winning segment
    double c, ux, uy;    // of the winning segment: the cross product w x u and its direction u = B - A
    int seg, last_seg;   // the winning segment and the route's last non-degenerate one (indices within the route)
    bool end;            // t >= L2 on the winning segment (the nearest point is its end vertex)
};

__device__ __forceinline__ RouteMeasure route_measure(const float2* lv, int k0, int k1, double x, double y) {
    RouteMeasure m;
    m.d2min = __builtin_inf();
    m.c = m.ux = m.uy = 0.0;
    m.seg = m.last_seg = -1;
    m.end = false;
    int k = k0;
    float2 A = lv[k];
    for (++k; k < k1; ++k) {
        const float2 B = lv[k];
        // route_seg_d2's operations, with t, L2 and c kept
        const double ux = (double)B.x - (double)A.x, uy = (double)B.y - (double)A.y;
        const double wx = x - (double)A.x, wy = y - (double)A.y;
        A = B;
        if (ux == 0.0 && uy == 0.0) continue;   // a zero-length segment is skipped
        const double L2 = ux * ux + uy * uy;
        const double t = wx * ux + wy * uy;
        const double cr = wx * uy - wy * ux;
        double d2;
        if (t <= 0.0) {
            d2 = wx * wx + wy * wy;
        } else if (t >= L2) {
            const double vx = x - (double)B.x, vy = y - (double)B.y;
            d2 = vx * vx + vy * vy;
        } else {
            d2 = (cr * cr) / L2;
        }
        m.last_seg = k - 1 - k0;
        if (d2 < m.d2min) {
            m.d2min = d2;
            m.seg = m.last_seg;
            m.c = cr;
            m.ux = ux;
            m.uy = uy;
            m.end = t >= L2;
        }
    }
    return m;
}

}  // namespace t2d
