// t2d_route_write_dev.h -- what the kernels that write one curve per env into the installed route sets share (curve_routes_kernel,
// spline_routes_kernel, planview_kernel<true>): the writable slot of a route, the "point k, else the tail" fill and the saturating
// point count.  What a point and the tail are stays in each kernel; the host's side is write_routes in t2d_api.hip.  DESIGN.md 4.18a.
#pragma once
#include "t2d_pool.h"

namespace t2d {

// the count a caller reads: the points of the whole curve, saturating at INT32_MAX
T2D_DEV int32_t point_count(long long total) { return total > 2147483647ll ? 2147483647 : (int32_t)total; }

// Route `route` of env e's own set as fp32 pairs to write: the only place that computes a writable slot.  RouteView is the readers'
// view, hence the const_cast; it is sound because the host has checked (write_routes) that no two envs share a set and that every
// env's set has the route.
struct RouteSlot { float2* out; int cap; };
T2D_DEV RouteSlot route_slot(const RouteView& rv, int e, int route) {
    const int r = rv.set_route_start[rv.set_of_env[e]] + route, v0 = rv.route_vert_off[r];
    return {reinterpret_cast<float2*>(const_cast<float*>(rv.verts)) + v0, rv.route_vert_off[r + 1] - v0};
}

// Vertex k = lane, lane + n_lanes, ... of the slot: point(k, x, y) rounded to fp32 where k < total, else `tail`.
template <class Point>
T2D_DEV void route_fill(const RouteSlot& slot, int lane, int n_lanes, long long total, float2 tail, Point point) {
    for (int k = lane; k < slot.cap; k += n_lanes) {
        float2 v = tail;
        if (k < total) {
            double x, y;
            point(k, x, y);
            v = make_float2((float)x, (float)y);
        }
        slot.out[k] = v;
    }
}

}  // namespace t2d
