// t2d_pid.hip -- lane-keeping scripted traffic: the reference's PIDController for every controlled participant of every env in
// one launch in front of the step launch (t2d_pid_actions, include/t2d.h).
//
// Replaces (reference, tactics2d v0.1.9rc3):
//   PIDController._compute_pid             controller/pid_controller.py:159-234  (filtered derivative, anti-windup, both clips)
//   PIDController._compute_lateral_error   controller/pid_controller.py:249-283  (target_heading before cross_track_error)
//   PIDController.step                     controller/pid_controller.py:309-406  (lateral, then longitudinal; 2.0 / wheel_base)
//   PIDController.reset                    controller/pid_controller.py:408-418
// The reference leaves cross_track_error / target_heading / target_speed to its caller and ships no caller: the measurement
// against the installed route is BUILD-DEFINED (include/t2d.h states it, tests/pid_ref.py restates it in numpy).
//
// One workgroup per env, one lane per participant (scripted_launch, t2d_scripted_dev.h).  The env's route set is staged in LDS
// by stage_route_set (fp32 pairs behind the set's route offsets, widened on read): lanes on the same route read the same
// address in the same iteration (one broadcast 8-byte read).  The lane's participant, the caller's row and the wheel-base
// fallback are that header's too (scripted_lane, action_row_in / _out, wheel_base_or_type).  When a row uses the IDM law the
// env's (x, y) go through LDS as fp64 pairs, NaN = inactive (scripted_xy) -- idm_kernel's scheme -- for find_leader.  fp64 in registers, plain vector
// stores, no atomics, no cross-lane traffic.  State: six fp64 words per participant, struct-of-arrays.
#include "t2d_idm_dev.h"
#include "t2d_route_dev.h"
#include "t2d_scripted_dev.h"

namespace t2d {

namespace {

// _compute_pid: `integral / prev_error / prev_der` in, the state AFTER the call out; limits = (lo, hi) when LIMITS
template <bool LIMITS>
T2D_DEV double pid_compute(double error, double& integral, double& prev_error, double& prev_der, double kp, double ki, double kd,
                           double dt, double alpha, double lo, double hi, bool& saturated) {
    const double p_term = kp * error;
    const double raw = dt > 0.0 ? (error - prev_error) / dt : 0.0;
    const double der = alpha * raw + (1.0 - alpha) * prev_der;
    const double d_term = kd * der;
    double out = p_term + d_term;
    saturated = false;
    if (LIMITS) {
        if (out > hi) {
            saturated = true;
            out = hi;
        } else if (out < lo) {
            saturated = true;
            out = lo;
        }
    }
    if (!saturated) integral = integral + error * dt;
    else integral = integral * 0.99;
    const double i_term = ki * integral;
    out = out + i_term;
    if (LIMITS) out = clipd(out, lo, hi);
    prev_error = error;
    prev_der = der;
    return out;
}

// grid = n_env, block = max_agents rounded up to whole waves; dynamic LDS = RouteView::lds_bytes (route sets installed):
//   float2 verts[nv] | int32 first_vertex[nr + 1]   of the env's set (nv <= T2D_MAX_ROUTE_SET_VERTS)
__global__ __launch_bounds__(kScriptedBlock) void pid_kernel(PoolView pv, PidView cv, RouteView rv, const uint32_t* act_in, uint32_t* act_out,
                                                        t2d_pid_record* out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char pid_lds[];
    __shared__ double2 s_xy[kScriptedBlock];
    __shared__ float s_v[kScriptedBlock];
    const int e = blockIdx.x, a = threadIdx.x;
    StagedRoutes routes{reinterpret_cast<const float2*>(pid_lds), nullptr};
    if (rv.kind == 1) routes = stage_route_set(pid_lds, rv, e);
    const float2* lv = routes.verts;
    const int32_t* lo = routes.first;
    const ScriptedLane ln = scripted_lane(pv, cv.ctrl_id, e, a);
    const bool active = ln.active;
    const int i = ln.i, ctrl = ln.ctrl;
    const uint32_t ids = ln.ids;
    const float fx = ln.x, fy = ln.y, fh = ln.heading, fv = ln.speed;
    const double qnan = __builtin_nan("");
    if (cv.stage_xy) {
        s_xy[a] = scripted_xy(ln);
        s_v[a] = fv;
    }
    __syncthreads();
    if (!ln.valid) return;

    const ActionRow in = action_row_in(act_in, i);
    ActionRow o = in;
    t2d_pid_record r;
    r.cross_track = qnan;
    r.lat_error = qnan;
    r.segment = -1;
    r.leader = -1;
    r.events = 0;
    r.reserved = 0;
    r.action[0] = r.action[1] = qnan;
    if (ctrl != T2D_PID_NONE && ctrl < cv.n_ctrl) {
        const size_t N = (size_t)pv.N;
        const double* c = cv.rows + (size_t)ctrl * T2D_PID_COLS;
        const double dt = c[T2D_PID_DT], alpha = c[T2D_PID_ALPHA];
        const int lat_mode = (int)c[T2D_PID_LAT_MODE], lon_mode = (int)c[T2D_PID_LON_MODE];
        double S[T2D_PID_STATE_WORDS];
        // the episode ended in the last step: controller.reset() for every participant of the env
        const uchar4 st = reinterpret_cast<const uchar4*>(pv.status)[e];
        if (st.z | st.w) {
#pragma unroll
            for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) S[w] = 0.0;
            r.events |= T2D_PID_RESET;
        } else {
#pragma unroll
            for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) S[w] = cv.state[w * N + i];
        }
        const float ts = cv.target_speed[i];
        const double x = (double)fx, y = (double)fy, h = (double)fh, v = (double)fv;
        const bool finite_in = __builtin_isfinite(fx) && __builtin_isfinite(fy) && __builtin_isfinite(fh) && __builtin_isfinite(fv) &&
                               (lon_mode != 1 || __builtin_isfinite(ts));
        if (active && !finite_in) r.events |= T2D_PID_NONFINITE;
        if (active && finite_in) {
            double T[T2D_PID_STATE_WORDS];
#pragma unroll
            for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) T[w] = S[w];
            // ---- the measurement against the route
            bool measured = false;
            double cte = 0.0, th = 0.0;
            const int ro = (lat_mode != 0 && rv.kind == 1) ? rv.route_of[i] : -1;
            if (ro >= 0) {
                const RouteMeasure m = route_measure(lv, lo[ro], lo[ro + 1], x, y);
                const double d2min = m.d2min, wc = m.c, wux = m.ux, wuy = m.uy;
                const int seg = m.seg, last_seg = m.last_seg;
                const bool wend = m.end;
                if (seg >= 0) {
                    const double d = __builtin_sqrt(d2min);
                    cte = wc > 0.0 ? d : wc < 0.0 ? -d : 0.0;
                    th = atan2_det(wuy, wux);
                    measured = true;
                    r.cross_track = cte;
                    r.segment = seg;
                    if (wend && seg == last_seg) r.events |= T2D_PID_ROUTE_END;
                }
            }
            // ---- lateral
            double steering = 0.0;
            if (lat_mode != 0) {
                if (!measured) {
                    r.events |= T2D_PID_NO_ROUTE;   // the combined-mode fallback: steering 0.0, lateral state untouched
                } else {
                    double err = cte;
                    if (lat_mode == 1) {
                        double se, ce;
                        sincos_det(th - h, se, ce);
                        err = atan2_det(se, ce);
                    }
                    r.lat_error = err;
                    bool sat;
                    const double lat_out = pid_compute<false>(err, T[0], T[1], T[2], c[T2D_PID_KP_LAT], c[T2D_PID_KI_LAT], c[T2D_PID_KD_LAT],
                                                              dt, alpha, 0.0, 0.0, sat);
                    const double ms = c[T2D_PID_MAX_STEERING];
                    if (lat_mode == 2) {
                        const double wb = wheel_base_or_type(c[T2D_PID_WHEEL_BASE], pv, ids);
                        if (wb <= 0.0) r.events |= T2D_PID_BAD_WHEEL_BASE;   // (the state above is updated all the same)
                        else steering = clipd(lat_out * (2.0 / wb), -ms, ms);
                    } else {
                        steering = clipd(lat_out, -ms, ms);
                    }
                }
            }
            // ---- longitudinal
            double accel = 0.0;
            if (lon_mode == 1) {
                const double lo_a = c[T2D_PID_MIN_ACCEL], hi_a = c[T2D_PID_MAX_ACCEL];
                bool sat;
                const double lon_out = pid_compute<true>((double)ts - v, T[3], T[4], T[5], c[T2D_PID_KP_LON], c[T2D_PID_KI_LON],
                                                         c[T2D_PID_KD_LON], dt, alpha, lo_a, hi_a, sat);
                accel = clipd(lon_out, lo_a, hi_a);
                if (sat) r.events |= T2D_PID_SATURATED;
            } else if (lon_mode == 2) {
                const int irow = cv.idm_row[i];
                accel = qnan;   // (rows that are gone: the host refuses the call; never read past them)
                if (cv.idm_rows && irow >= 0 && irow < cv.n_idm) {
                    const idm::IdmRow ic = idm::load_row((const T2D_GLOBAL double*)(cv.idm_rows + (size_t)irow * T2D_IDM_COLS));
                    double sn, cs;
                    sincos_det(h, sn, cs);
                    const int lead = idm::find_leader<false>([&](int j) { return s_xy[j]; }, pv.A, ic, x, y, sn, cs);
                    double dx = 0.0, dy = 0.0, vl = 0.0;
                    if (lead >= 0) {
                        dx = s_xy[lead].x - x;
                        dy = s_xy[lead].y - y;
                        vl = (double)s_v[lead];
                    }
                    accel = idm::idm_law(ic, v, lead >= 0, dx, dy, vl);
                    r.leader = lead;
                }
            } else if (lon_mode == 3) {
                accel = (double)__uint_as_float(in.w1);
            }
            // ---- commit
            if (__builtin_isfinite(steering) && __builtin_isfinite(accel)) {
#pragma unroll
                for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) S[w] = T[w];
                r.action[0] = steering;
                r.action[1] = accel;
                o = {__float_as_uint((float)steering), __float_as_uint((float)accel)};
            } else {
                r.events |= T2D_PID_NONFINITE;
            }
        }
#pragma unroll
        for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) cv.state[w * N + i] = S[w];
    }
    out[i] = r;
    action_row_out(act_out, i, o);
}

__global__ __launch_bounds__(kScriptedBlock) void pid_reset_kernel(int N, int A, PidView cv, const uint8_t* mask) {
    const int i = blockIdx.x * kScriptedBlock + threadIdx.x;
    if (i >= N || (mask && !mask[i / A])) return;
#pragma unroll
    for (int w = 0; w < T2D_PID_STATE_WORDS; ++w) cv.state[(size_t)w * N + i] = 0.0;
}

}  // namespace

hipError_t launch_pid(const PoolView& v, const PidView& cv, const RouteView& rv, const float* act_in, float* act_out,
                      t2d_pid_record* out, hipStream_t s) {
    const ScriptedLaunch l = scripted_launch(v, rv);
    hipLaunchKernelGGL(pid_kernel, dim3(v.n_env), dim3(l.block), l.lds, s, v, cv, rv, reinterpret_cast<const uint32_t*>(act_in),
                       reinterpret_cast<uint32_t*>(act_out), out);
    return hipGetLastError();
}

hipError_t launch_pid_reset(const PoolView& v, const PidView& cv, const uint8_t* mask, hipStream_t s) {
    hipLaunchKernelGGL(pid_reset_kernel, dim3((v.N + kScriptedBlock - 1) / kScriptedBlock), dim3(kScriptedBlock), 0, s, v.N, v.A, cv, mask);
    return hipGetLastError();
}

}  // namespace t2d
