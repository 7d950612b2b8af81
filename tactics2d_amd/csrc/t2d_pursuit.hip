// t2d_pursuit.hip -- path-following scripted traffic: the reference's PurePursuitController and AccelerationController (cruise
// and adaptive cruise) for every controlled participant of every env in one launch in front of the step launch
// (t2d_pursuit_actions, include/t2d.h).
//
// Replaces (reference, tactics2d v0.1.9rc3):
//   AccelerationController._cruise_control            controller/acceleration_controller.py:73-93
//   AccelerationController._adaptive_cruise_control   controller/acceleration_controller.py:95-124
//   AccelerationController.step                       controller/acceleration_controller.py:126-145  (steering 0.0)
//   PurePursuitController._lateral_control            controller/pure_pursuit_controller.py:53-74
//   PurePursuitController.step                        controller/pure_pursuit_controller.py:76-98
// The reference interpolates its look-ahead point from the start of whatever line string the caller passes; which line string
// that is stays BUILD-DEFINED here: the rest of the installed route from the participant's projection onward (include/t2d.h
// states the walk, tests/pursuit_ref.py restates it in numpy).
//
// Built from t2d_scripted_dev.h, as pid_kernel is: one workgroup per env, one lane per participant (scripted_launch); the env's
// route set staged in LDS by stage_route_set; the lane's participant, the caller's row and the wheel-base fallback from
// scripted_lane, action_row_in / _out and wheel_base_or_type; the projection is route_measure (t2d_route_dev.h), the one
// pid_kernel runs.  Its own: the lane's T2D_F_APPLIED0, and when a row uses ACC the env's (x, y) through LDS as fp64 pairs
// (scripted_xy: NaN = inactive) beside its speed and applied acceleration, for idm::find_leader.  The walk is a per-lane loop over LDS of data-dependent length, bounded by the
// route's segment count.  fp64 in registers, plain vector stores, no atomics, no cross-lane traffic, no state.
#include "t2d_idm_dev.h"
#include "t2d_route_dev.h"
#include "t2d_scripted_dev.h"

namespace t2d {

namespace {

// the two clips both acceleration laws end with (acceleration_controller.py:86-91, :117-122)
T2D_DEV double accel_clips(double accel, double accel_last, const double* c) {
    const double step = c[T2D_PURSUIT_ACCEL_CHANGE_RATE] * c[T2D_PURSUIT_DELTA_T];
    accel = clipd(accel, accel_last - step, accel_last + step);
    return clipd(accel, c[T2D_PURSUIT_MIN_ACCEL], c[T2D_PURSUIT_MAX_ACCEL]);
}

// grid = n_env, block = max_agents rounded up to whole waves; dynamic LDS = RouteView::lds_bytes (route sets installed):
//   float2 verts[nv] | int32 first_vertex[nr + 1]   of the env's set (nv <= T2D_MAX_ROUTE_SET_VERTS)
__global__ __launch_bounds__(kScriptedBlock) void pursuit_kernel(PoolView pv, PursuitView cv, RouteView rv, const uint32_t* act_in,
                                                                uint32_t* act_out, t2d_pursuit_record* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pursuit_lds[];
    __shared__ double2 s_xy[kScriptedBlock];
    __shared__ float2 s_va[kScriptedBlock];   // (speed, applied acceleration)
    const int e = blockIdx.x, a = threadIdx.x;
    StagedRoutes routes{reinterpret_cast<const float2*>(pursuit_lds), nullptr};
    if (rv.kind == 1) routes = stage_route_set(pursuit_lds, rv, e);
    const float2* lv = routes.verts;
    const int32_t* lo = routes.first;
    const ScriptedLane ln = scripted_lane<true>(pv, cv.ctrl_id, e, a, pv.applied0);   // (+ the acceleration the last step applied)
    const bool active = ln.active;
    const int i = ln.i, ctrl = ln.ctrl;
    const uint32_t ids = ln.ids;
    // an env that a step's own epilogue has just restarted still holds the ended episode's column: nothing is applied yet
    const bool restarted = cv.episode_gate && pv.cnt_step[e] == 0;
    const float fx = ln.x, fy = ln.y, fh = ln.heading, fv = ln.speed, fa = restarted ? 0.f : ln.also;
    const double qnan = __builtin_nan("");
    if (cv.stage_xy) {
        s_xy[a] = scripted_xy(ln);
        s_va[a] = make_float2(fv, fa);
    }
    __syncthreads();
    if (!ln.valid) return;

    const ActionRow in = action_row_in(act_in, i);
    ActionRow o = in;
    t2d_pursuit_record r;
    r.point[0] = r.point[1] = qnan;
    r.pre_aiming_distance = qnan;
    r.distance = qnan;
    r.cross_track = qnan;
    r.segment = -1;
    r.target_segment = -1;
    r.leader = -1;
    r.events = 0;
    r.action[0] = r.action[1] = qnan;
    if (ctrl != T2D_PURSUIT_NONE && ctrl < cv.n_ctrl) {
        const double* c = cv.rows + (size_t)ctrl * T2D_PURSUIT_COLS;
        const int lat_mode = (int)c[T2D_PURSUIT_LAT_MODE], lon_mode = (int)c[T2D_PURSUIT_LON_MODE];
        const float ts = cv.target_speed[i];
        const double x = (double)fx, y = (double)fy, h = (double)fh, v = (double)fv, accel_last = (double)fa;
        const bool finite_in = __builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(fh) && __builtin_isfinite(fv) &&
                               __builtin_isfinite(fa) && (lon_mode == 2 || __builtin_isfinite(ts));
        if (active && !finite_in) r.events |= T2D_PURSUIT_NONFINITE;
        if (active && finite_in) {
            // ---- lateral: the projection, the walk, the pure-pursuit law
            double steering = 0.0;
            if (lat_mode == 1) {
                const double pre = v * c[T2D_PURSUIT_INTERVAL_LAT], min_pre = c[T2D_PURSUIT_MIN_PRE_AIMING];
                const double d = pre > min_pre ? pre : min_pre;   // np.max of two finite numbers
                r.pre_aiming_distance = d;
                const int ro = rv.kind == 1 ? rv.route_of[i] : -1;
                int seg = -1, k0 = 0, nseg = 0;
                if (ro >= 0) {
                    k0 = lo[ro];
                    const int k1 = lo[ro + 1];
                    nseg = k1 - k0 - 1;
                    const RouteMeasure m = route_measure(lv, k0, k1, x, y);
                    seg = m.seg;
                    if (seg >= 0) {
                        const double dist = __builtin_sqrt(m.d2min);
                        r.cross_track = m.c > 0.0 ? dist : m.c < 0.0 ? -dist : 0.0;
                        r.segment = seg;
                    }
                }
                if (seg < 0) {
                    r.events |= T2D_PURSUIT_NO_ROUTE;   // steering 0.0
                } else {
                    // the start point Q on the winning segment (its t and L2 again: the same operations, the same bits)
                    const float2 A = lv[k0 + seg], B = lv[k0 + seg + 1];
                    const double ux = (double)B.x - (double)A.x, uy = (double)B.y - (double)A.y;
                    const double wx = x - (double)A.x, wy = y - (double)A.y;
                    const double L2 = ux * ux + uy * uy;
                    const double t = wx * ux + wy * uy;
                    const double tc = t <= 0.0 ? 0.0 : t >= L2 ? L2 : t;
                    const double q = tc / L2;
                    double cx = (double)A.x + ux * q, cy = (double)A.y + uy * q;
                    const float2 first = lv[k0], last = lv[k0 + nseg];
                    const bool closed = __float_as_uint(first.x) == __float_as_uint(last.x) &&
                                        __float_as_uint(first.y) == __float_as_uint(last.y);
                    const int visits = closed ? nseg : nseg - seg;
                    double rem = d, tx = 0.0, ty = 0.0;
                    int s = seg, tseg = seg;
                    bool found = false;
                    for (int n = 0; n < visits && !found; ++n) {
                        if (s == nseg) {   // (closed: vertex nseg IS vertex 0, so cur carries over the seam)
                            s = 0;
                        }
                        if (s < seg) r.events |= T2D_PURSUIT_WRAPPED;
                        const float2 E = lv[k0 + s + 1];
                        const double vx = (double)E.x - cx, vy = (double)E.y - cy;
                        const double L = __builtin_sqrt(vx * vx + vy * vy);
                        tseg = s;
                        if (rem <= L && L > 0.0) {
                            const double f = rem / L;
                            tx = cx + vx * f;
                            ty = cy + vy * f;
                            found = true;
                        } else {
                            rem = rem - L;
                            cx = (double)E.x;
                            cy = (double)E.y;
                            ++s;
                        }
                    }
                    if (!found) {
                        tx = cx;
                        ty = cy;
                        r.events |= T2D_PURSUIT_ROUTE_END;
                    }
                    r.point[0] = tx;
                    r.point[1] = ty;
                    r.target_segment = tseg;
                    // _lateral_control
                    const double wb = wheel_base_or_type(c[T2D_PURSUIT_WHEEL_BASE], pv, ids);
                    const double dy = ty - y, dx = tx - x;
                    const double angle = atan2_det(dy, dx);
                    const double distance = __builtin_sqrt(dy * dy + dx * dx);
                    r.distance = distance;
                    double sn, cs;
                    sincos_det(angle - h, sn, cs);
                    steering = atan_det(2.0 * wb * sn / distance);
                }
            }
            // ---- longitudinal
            double accel;
            if (lon_mode == 2) {
                accel = (double)__uint_as_float(in.w1);
            } else {
                const double kp = c[T2D_PURSUIT_KP];
                int lead = -1;
                if (lon_mode == 1) {
                    idm::IdmRow ic;
                    ic.des = ic.T = ic.s0 = ic.amax = ic.b = ic.delta = 0.0;
                    ic.hw = c[T2D_PURSUIT_LANE_HALF_WIDTH];
                    ic.horizon = c[T2D_PURSUIT_HORIZON];
                    double sn, cs;
                    sincos_det(h, sn, cs);
                    lead = idm::find_leader<false>([&](int j) { return s_xy[j]; }, pv.A, ic, x, y, sn, cs);
                    r.leader = lead;
                    if (lead < 0) r.events |= T2D_PURSUIT_NO_LEADER;
                }
                if (lead >= 0) {
                    const double dx = x - s_xy[lead].x, dy = y - s_xy[lead].y;
                    const float2 va = s_va[lead];
                    const double distance_front = __builtin_sqrt(dx * dx + dy * dy);
                    const double distance_target = clipd(v * c[T2D_PURSUIT_INTERVAL_LON] + 5.0, 7.0, 80.0);
                    const double relative_speed = (double)va.x - v;
                    const double relative_target_speed = (distance_target - distance_front) / kp;
                    const double relative_accel = (relative_target_speed - relative_speed) / kp;
                    accel = accel_clips((double)va.y - relative_accel, accel_last, c);
                } else {
                    accel = accel_clips(((double)ts - v) / kp, accel_last, c);
                }
            }
            // ---- commit
            if (__builtin_isfinite(steering) && __builtin_isfinite(accel)) {
                r.action[0] = steering;
                r.action[1] = accel;
                o = {__float_as_uint((float)steering), __float_as_uint((float)accel)};
            } else {
                r.events |= T2D_PURSUIT_NONFINITE;
            }
        }
    }
    out[i] = r;
    action_row_out(act_out, i, o);
}

}  // namespace

hipError_t launch_pursuit(const PoolView& v, const PursuitView& cv, const RouteView& rv, const float* act_in, float* act_out,
                          t2d_pursuit_record* out, hipStream_t s) {
    const ScriptedLaunch l = scripted_launch(v, rv);
    hipLaunchKernelGGL(pursuit_kernel, dim3(v.n_env), dim3(l.block), l.lds, s, v, cv, rv, reinterpret_cast<const uint32_t*>(act_in),
                       reinterpret_cast<uint32_t*>(act_out), out);
    return hipGetLastError();
}

}  // namespace t2d
