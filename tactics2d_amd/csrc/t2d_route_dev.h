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

}  // namespace t2d
