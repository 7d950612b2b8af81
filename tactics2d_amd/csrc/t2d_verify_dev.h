// t2d_verify_dev.h -- the reference's "very rough check" of one state transition (device functions), shared by verify_kernel
// (t2d_integrate.hip: t2d_verify_state, last state = the pool's current state) and verify_states_kernel (t2d_history.hip:
// t2d_verify_states, last state = frame 0 of a recorded trajectory).
//   SingleTrackKinematics.verify_state physics/single_track_kinematics.py:200-250, SingleTrackDynamics :253-306 (same check),
//   PointMass.verify_state physics/point_mass.py:234-259.  Oracle: t2do_verify_state.
//
// Split in two so that a caller checking many candidates against ONE last state over ONE interval (a stable-frequency
// trajectory: physics_model_base.py:63-71 never advances last_state) computes the reachable ranges once: verify_reach holds
// everything that depends on the last state and the interval only, verify_candidate the comparisons.  Both halves are the
// expressions of the single-call check, so the split changes no bit.
#pragma once
#include "t2d_math.h"
#include "t2d_pool.h"

namespace t2d {

struct VerifyReach {
    int kind;        // 0: True whatever the candidate (interval 0, inactive, unbounded ranges); 1: point-mass accel; 2: single track
    double lx, ly, lvx, lvy, dt, den;       // point mass: last position / velocity, dt, 2 / dt^2
    double hr[2], sr[2], xr[2], yr[2];      // single track: heading / speed / x / y ranges
};

// params: the transposed device table [T2D_PARAM_COLS][T2D_MAX_TYPES]; last = x, y, heading, speed, vx, vy of the last state
T2D_DEV VerifyReach verify_reach(const double* params, int type, int model, double lx, double ly, double lh, double lv,
                                 double lvx, double lvy, double interval_ms) {
    VerifyReach r;
    r.kind = 0;
    if (interval_ms == 0) return r;   // "no time elapsed, state should be valid"
    auto P = [&](int col) -> double { return params[col * T2D_MAX_TYPES + type]; };
    const int flags = (int)P(T2D_P_RANGE_FLAGS);
    const double dt = interval_ms / 1000;
    if (model == T2D_MODEL_POINTMASS || model == T2D_MODEL_POINTMASS_EULER) {  // both back-ends: point_mass.py:234-259
        if (!(flags & T2D_RANGE_ACCEL)) return r;
        r.kind = 1;
        r.lx = lx; r.ly = ly; r.lvx = lvx; r.lvy = lvy; r.dt = dt;
        r.den = 2 / (dt * dt);
    } else if ((flags & 7) == 7) {
        r.kind = 2;
        const double wb = P(T2D_P_WB), k = P(T2D_P_LR) / wb;
        const double st[2] = {P(T2D_P_STEER_LO), P(T2D_P_STEER_HI)};
        const double ac[2] = {P(T2D_P_ACCEL_LO), P(T2D_P_ACCEL_HI)};
        const double vlo = P(T2D_P_SPEED_LO), vhi = P(T2D_P_SPEED_HI);
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const double beta = atan_det(k * st[e]);
            double sb, cb, sh, ch;
            sincos_det(beta, sb, cb);
            r.hr[e] = mod_two_pi(lh + lv / wb * sb * dt);
            r.sr[e] = clipd(lv + ac[e] * dt, vlo, vhi);
            sincos_det(lh + beta, sh, ch);
            r.xr[e] = lx + r.sr[e] * ch * dt;
            r.yr[e] = ly + r.sr[e] * sh * dt;
        }
    }
    return r;
}

T2D_DEV bool verify_candidate(const VerifyReach& r, const double* params, int type, double x, double y, double h, double v) {
    if (r.kind == 1) {
        const double ax = (x - r.lx - r.lvx * r.dt) * r.den;
        const double ay = (y - r.ly - r.lvy * r.dt) * r.den;
        const double acc = __builtin_sqrt(ax * ax + ay * ay);
        return params[T2D_P_ACCEL_LO * T2D_MAX_TYPES + type] <= acc && acc <= params[T2D_P_ACCEL_HI * T2D_MAX_TYPES + type];
    }
    if (r.kind == 2) {
        if (r.hr[0] < r.hr[1] && !(r.hr[0] <= h && h <= r.hr[1])) return false;
        if (r.hr[0] > r.hr[1] && !(r.hr[0] <= h || h <= r.hr[1])) return false;
        if (!(r.sr[0] <= v && v <= r.sr[1])) return false;
        if (!(r.xr[0] < x && x < r.xr[1]) || !(r.yr[0] < y && y < r.yr[1])) return false;
    }
    return true;
}

}  // namespace t2d
