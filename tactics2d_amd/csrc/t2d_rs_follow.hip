// t2d_rs_follow.hip -- following a Reeds-Shepp plan: the parking tutorial's RSAgent with its three PID controllers
// (docs/tutorial/train_parking_demo.ipynb cells 14 and 17) and the wrapper's action scaling (cell 7) for the ego of every env,
// one launch in front of the step launch.  include/t2d.h (t2d_rs_follow) says what one call does; DESIGN.md 4.15a.
//
// One lane per env, 64-thread workgroups (4096 envs = 64 workgroups, one per CU of the first 64): some hundred fp64
// operations behind four fp32 loads, no LDS, no cross-lane traffic, no atomics.  The state is struct-of-arrays -- row r of a
// table is n_env consecutive values -- so a wave's loads and stores of one field coalesce; segment fields are indexed by the
// lane's own head, which differs between lanes by at most four rows.
#include "t2d_pool.h"
#include "t2d_math.h"

namespace t2d {
namespace {

T2D_DEV double rf_sign(double v) { return v > 0.0 ? 1.0 : v < 0.0 ? -1.0 : 0.0; }
T2D_DEV double rf_clip(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }   // (np.clip: a NaN stays)
// _preprocess_action for one component of the symmetric box +-bound, in fp32 and in the wrapper's order
T2D_DEV float rf_wrap(double a, float bound) {
    float v = (float)a;
    v = v < -1.0f ? -1.0f : v > 1.0f ? 1.0f : v;
    const float high = bound, low = -bound;
    return v * (high - low) / 2.0f + (high + low) / 2.0f;
}
struct RfPid {
    double target, prev, integral, out;
};
// PIDController.update(value, target): the state AFTER it in `c`, committed by the caller only if the whole action is finite
T2D_DEV void rf_pid(RfPid& c, double kp, double ki, double kd, double value, double target) {
    const double error = target - value;
    c.integral = c.integral + error;
    const double derivative = error - c.prev;
    c.out = kp * error + ki * c.integral + kd * derivative;
    c.prev = error;
    c.target = target;
}

__global__ __launch_bounds__(64) void rs_follow_kernel(PoolView pv, RsFollowView fv, const t2d_rs_plan_record* plan,
                                                       const uint32_t* act_in, uint32_t* act_out, t2d_rs_follow_record* out) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= pv.n_env) return;
    const size_t E = (size_t)pv.n_env;
    const t2d_rs_follow_params& c = fv.cfg;
    double* const f = fv.f64;
    int32_t* const w = fv.i32;
    const double nan_v = __builtin_nan(""), inf = __builtin_inf();
    const uint32_t in0 = act_in ? act_in[2 * (size_t)e] : 0u, in1 = act_in ? act_in[2 * (size_t)e + 1] : 0u;
    uint32_t events = 0;
    int n_seg = w[kRfNSeg * E + e], head = w[kRfHead * E + e], steps = w[kRfSteps * E + e];
    double last = f[kRfLast * E + e];

    // 1. the episode ended in the last step: agent.reset()
    const uchar4 st = reinterpret_cast<const uchar4*>(pv.status)[e];
    if (st.z | st.w) {
        n_seg = head = steps = 0;
        last = inf;
        for (int k = 0; k < 3; ++k) f[(kRfPid + 3 * k + 1) * E + e] = f[(kRfPid + 3 * k + 2) * E + e] = 0.0;   // (the target stays)
        events |= T2D_RS_FOLLOW_RESET;
    }
    const int ie = e * pv.A + fv.ego_index;
    const bool active = ((pv.ids[ie] >> kIdsActiveShift) & 0xffu) != 0;
    const double x = (double)pv.x[ie], y = (double)pv.y[ie], yaw = (double)pv.heading[ie], v = (double)pv.speed[ie];
    const bool finite = __builtin_isfinite(x) && __builtin_isfinite(y) && __builtin_isfinite(yaw) && __builtin_isfinite(v);
    bool acted = false;
    double a0 = nan_v, a1 = nan_v, d_out = nan_v, total_out = nan_v;
    if (active && !finite) {
        n_seg = head = steps = 0;
        last = inf;
        events |= T2D_RS_FOLLOW_DROPPED;
    } else if (active) {
        double sy, cy;
        sincos_det(yaw, sy, cy);
        const double rx = x - c.dr * cy, ry = y - c.dr * sy;   // rear_center_coord
        // 2. adopt: calculate_target_points
        const t2d_rs_plan_record* pr = plan + e;
        if (head >= n_seg && pr->status == T2D_RS_FOUND && pr->n_seg >= 1 && pr->n_seg <= T2D_RS_MAX_SEGMENTS) {
            n_seg = pr->n_seg;
            head = steps = 0;
            events |= T2D_RS_FOLLOW_ADOPTED;
            double px = rx, py = ry, pyaw = yaw;
            for (int i = 0; i < n_seg; ++i) {
                const int steer = pr->steer[i] > 0 ? 1 : pr->steer[i] < 0 ? -1 : 0;
                const double dist = pr->distance[i];
                double s0, c0, tx, ty, tyaw, cx = nan_v, cyy = nan_v;
                sincos_det(pyaw, s0, c0);
                if (steer == 0) {
                    tx = px + dist * c0;
                    ty = py + dist * s0;
                    tyaw = pyaw;
                } else {
                    const double da = dist / c.radius;
                    double s1, c1;
                    if (steer > 0) {
                        cx = px - c.radius * s0;
                        cyy = py + c.radius * c0;
                        sincos_det(pyaw + da, s1, c1);
                        tx = cx + c.radius * s1;
                        ty = cyy - c.radius * c1;
                        tyaw = pyaw + da;
                    } else {   // (the notebook's R branch: sin / cos of -yaw + delta)
                        cx = px + c.radius * s0;
                        cyy = py - c.radius * c0;
                        sincos_det(-pyaw + da, s1, c1);
                        tx = cx + c.radius * s1;
                        ty = cyy + c.radius * c1;
                        tyaw = pyaw - da;
                    }
                }
                w[(kRfSteer + i) * E + e] = steer;
                double* g = f + (size_t)(kRfSeg + kRfSegFields * i) * E + e;
                g[0 * E] = dist; g[1 * E] = tx; g[2 * E] = ty; g[3 * E] = tyaw; g[4 * E] = cx; g[5 * E] = cyy; g[6 * E] = px; g[7 * E] = py;
                px = tx; py = ty; pyaw = tyaw;
            }
        }
        // 3. act: get_action
        if (head < n_seg) {
            acted = true;
            steps += 1;
            const double* g = f + (size_t)(kRfSeg + kRfSegFields * head) * E + e;
            double dx = rx - g[1 * E], dy = ry - g[2 * E];
            double d = __builtin_sqrt(dx * dx + dy * dy);
            d_out = d;
            if (d < c.reach_radius || (last < d && d < c.rising_radius)) {
                events |= d < c.reach_radius ? T2D_RS_FOLLOW_POP_REACHED : T2D_RS_FOLLOW_POP_RISING;
                last = inf;
                head += 1;
            } else {
                last = d;
            }
            if (head >= n_seg) {
                events |= T2D_RS_FOLLOW_FINISHED;
                a0 = a1 = 0.0;
            } else {
                g = f + (size_t)(kRfSeg + kRfSegFields * head) * E + e;
                const int steer = w[(kRfSteer + head) * E + e];
                const double dist = g[0], tx = g[1 * E], ty = g[2 * E], tyaw = g[3 * E], cx = g[4 * E], cyy = g[5 * E], sx = g[6 * E],
                             sy0 = g[7 * E];
                dx = rx - tx; dy = ry - ty;
                d = __builtin_sqrt(dx * dx + dy * dy);
                d_out = d;
                RfPid pid[3];
                for (int k = 0; k < 3; ++k) {
                    pid[k].target = f[(kRfPid + 3 * k) * E + e];
                    pid[k].prev = f[(kRfPid + 3 * k + 1) * E + e];
                    pid[k].integral = f[(kRfPid + 3 * k + 2) * E + e];
                }
                rf_pid(pid[0], c.kp_v, c.ki_v, c.kd_v, -d * rf_sign(dist), 0.0);
                const double target_v = rf_clip(pid[0].out, -c.max_speed, c.max_speed);
                rf_pid(pid[1], c.kp_a, c.ki_a, c.kd_a, v, target_v);
                const double target_a = rf_clip(pid[1].out, -c.max_acceleration, c.max_acceleration);
                double err, want_yaw;
                if (steer != 0) {
                    const double ex = rx - cx, ey = ry - cyy, sg = (double)steer;
                    err = (__builtin_sqrt(ex * ex + ey * ey) - c.radius) * sg;
                    want_yaw = atan2_det(ey, ex) + 3.141592653589793 / 2.0 * sg;
                } else {   // _calc_pt_error: the signed distance to the line start -> target, by which way the car points along it
                    const double ly = ty - sy0, lx = tx - sx;
                    const double line_yaw = atan2_det(ly, lx);
                    double sl, cl;
                    sincos_det(line_yaw - yaw, sl, cl);
                    err = ly * rx - lx * ry + tx * sy0 - ty * sx;
                    err = err / __builtin_sqrt(ly * ly + lx * lx);
                    err = err * (cl > 0.0 ? 1.0 : -1.0);
                    want_yaw = tyaw;
                }
                double ew = -(want_yaw - yaw), se, ce;
                sincos_det(ew, se, ce);
                ew = atan2_det(se, ce);
                const double total = err + c.yaw_weight * ew;
                rf_pid(pid[2], c.kp_s, c.ki_s, c.kd_s, -total, 0.0);
                const double target_steer = rf_clip((double)steer * c.steer_ratio + pid[2].out, -1.0, 1.0);
                a0 = target_steer;
                a1 = target_a / c.max_acceleration;
                total_out = total;
                if (__builtin_isfinite(a0) && __builtin_isfinite(a1)) {
                    for (int k = 0; k < 3; ++k) {
                        f[(kRfPid + 3 * k) * E + e] = pid[k].target;
                        f[(kRfPid + 3 * k + 1) * E + e] = pid[k].prev;
                        f[(kRfPid + 3 * k + 2) * E + e] = pid[k].integral;
                    }
                } else {   // build-defined (a): the path is dropped, the controllers keep what they had
                    acted = false;
                    n_seg = head = steps = 0;
                    last = inf;
                    a0 = a1 = d_out = total_out = nan_v;
                    events |= T2D_RS_FOLLOW_DROPPED;
                }
            }
        }
    }
    const int left = head < n_seg ? n_seg - head : 0;
    t2d_rs_follow_record r;
    r.executing = left;
    r.segment = left ? head : -1;
    r.events = events;
    r.steps = steps;
    r.action[0] = a0;
    r.action[1] = a1;
    r.distance_to_go = d_out;
    r.total_error = total_out;
    out[e] = r;
    if (!left) n_seg = head = steps = 0;
    w[kRfNSeg * E + e] = n_seg;
    w[kRfHead * E + e] = head;
    w[kRfSteps * E + e] = steps;
    f[kRfLast * E + e] = last;
    // 4. the action row
    if (acted) {
        act_out[2 * (size_t)e] = __float_as_uint(rf_wrap(a0, (float)c.steer_bound));
        act_out[2 * (size_t)e + 1] = __float_as_uint(rf_wrap(a1, (float)c.accel_bound));
    } else {
        act_out[2 * (size_t)e] = in0;
        act_out[2 * (size_t)e + 1] = in1;
    }
}

__global__ __launch_bounds__(64) void rs_follow_reset_kernel(int n_env, RsFollowView fv, const uint8_t* mask) {
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= n_env || (mask && !mask[e])) return;
    const size_t E = (size_t)n_env;
    fv.i32[kRfNSeg * E + e] = fv.i32[kRfHead * E + e] = fv.i32[kRfSteps * E + e] = 0;
    fv.f64[kRfLast * E + e] = __builtin_inf();
    for (int k = 0; k < 3; ++k) fv.f64[(kRfPid + 3 * k + 1) * E + e] = fv.f64[(kRfPid + 3 * k + 2) * E + e] = 0.0;
}

}  // namespace

hipError_t launch_rs_follow(const PoolView& v, const RsFollowView& fv, const t2d_rs_plan_record* plan, const float* act_in,
                            float* act_out, t2d_rs_follow_record* out, hipStream_t s) {
    hipLaunchKernelGGL(rs_follow_kernel, dim3((v.n_env + 63) / 64), dim3(64), 0, s, v, fv, plan, reinterpret_cast<const uint32_t*>(act_in),
                       reinterpret_cast<uint32_t*>(act_out), out);
    return hipGetLastError();
}
hipError_t launch_rs_follow_reset(const PoolView& v, const RsFollowView& fv, const uint8_t* mask, hipStream_t s) {
    hipLaunchKernelGGL(rs_follow_reset_kernel, dim3((v.n_env + 63) / 64), dim3(64), 0, s, v.n_env, fv, mask);
    return hipGetLastError();
}

}  // namespace t2d
