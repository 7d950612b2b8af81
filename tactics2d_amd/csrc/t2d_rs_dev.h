// t2d_rs_dev.h -- Reeds-Shepp candidate curves (interpolator/reeds_shepp.py) as device functions.
//
// ReedsShepp.get_all_path (:495-527) returns 48 slots in a fixed order: _CSC (8, :207-257), _CCC (12, :259-312), _CCCC (8,
// :314-374), _CCSC (16, :376-449) and _CCSCC (4, :451-493).  A slot is one of eight base formulas (the paper's 8.1 - 8.11)
// evaluated on one of eight images of the normalised goal (x, y, phi) -- time flip (-x, y, -phi), reflection (x, -y, -phi),
// "backward" (x cos phi + y sin phi, x sin phi - y cos phi, phi) and their compositions -- and gives (t, u, v) or nothing.
// ReedsSheppPath.__init__ (:19-44) then takes segments = |[t, u, v(, 1)] . matrix| and signs = sign(column sums of matrix):
// every matrix of the file has ONE non-zero entry per column, so column i of a slot is (which of t, u, v, 1; a factor of
// +-1 or +-pi/2), and that pair together with the word letters is a constant of the slot.  T2D_RS_SLOT_ROWS below is the
// one statement of those constants: t2d_rs.hip makes its __constant__ and its host copy of it (t2d_rs_slot_info reads the
// host copy for the Python side), and nothing else in the tree spells a word or a matrix.
//
// The _CCSCC family (slots 44-47) is restated as the file writes it, including a matrix whose straight piece comes out with
// a positive sign for u <= 0; such a slot was valid for none of 12 000 random goals.
#pragma once
#include "t2d_math.h"

namespace t2d {

constexpr int kRsSlots = 48;
constexpr int kRsMaxSeg = 5;

// base formulas
enum { RS_LSL = 0, RS_LSR, RS_LRL, RS_LRLR_A, RS_LRLR_B, RS_LRSL, RS_LRSR, RS_LRSLR };
// curve types in the order get_all_path concatenates them
enum { RS_CSC = 0, RS_CCC, RS_CCCC, RS_CCSC, RS_CCSCC };

// One slot.  xform: bit 0 time flip, bit 1 reflection, bit 2 backward (applied first).  variant: the sign triple of LRL
// (:287-292: 0 = (+, -, +), 1 = (+, -, -), 2 = (-, -, +)).  letter: +1 L, -1 R, 0 S (the steer sign), zero padded.
// col[i]: column i of the slot's matrix, sign * (1 + source) with source 0 t, 1 u, 2 v, 3 the constant row whose factor is
// pi / 2; 0 = no such column.  The negated matrices of the odd slots are written out.
struct RsSlot {
    int8_t formula, variant, xform, n_seg, curve_type;
    int8_t letter[kRsMaxSeg];
    int8_t col[kRsMaxSeg];
    int8_t pad;
};
static_assert(sizeof(RsSlot) == 16, "one 16-byte record per slot");

// a group of four slots: images 0..3 (+ x4) of one formula; reflection swaps L and R, a time flip negates the matrix
#define T2D_RS_ROW(f, var, x, n, ct, sg, l0, l1, l2, l3, l4, c0, c1, c2, c3, c4) \
    {f, var, x, n, ct, {(int8_t)((sg) * (l0)), (int8_t)((sg) * (l1)), (int8_t)((sg) * (l2)), (int8_t)((sg) * (l3)), (int8_t)((sg) * (l4))}, \
     {(int8_t)(((x) & 1 ? -1 : 1) * (c0)), (int8_t)(((x) & 1 ? -1 : 1) * (c1)), (int8_t)(((x) & 1 ? -1 : 1) * (c2)), \
      (int8_t)(((x) & 1 ? -1 : 1) * (c3)), (int8_t)(((x) & 1 ? -1 : 1) * (c4))}, 0}
#define T2D_RS_GROUP(f, var, x4, n, ct, l0, l1, l2, l3, l4, c0, c1, c2, c3, c4)       \
    T2D_RS_ROW(f, var, (x4) + 0, n, ct, 1, l0, l1, l2, l3, l4, c0, c1, c2, c3, c4),   \
    T2D_RS_ROW(f, var, (x4) + 1, n, ct, 1, l0, l1, l2, l3, l4, c0, c1, c2, c3, c4),   \
    T2D_RS_ROW(f, var, (x4) + 2, n, ct, -1, l0, l1, l2, l3, l4, c0, c1, c2, c3, c4),  \
    T2D_RS_ROW(f, var, (x4) + 3, n, ct, -1, l0, l1, l2, l3, l4, c0, c1, c2, c3, c4)
// letters L = 1, S = 0, R = -1; columns T = 1, U = 2, V = 3, H = 4 (the pi / 2 row), negative = a negative factor
#define T2D_RS_SLOT_ROWS                                                                        \
    T2D_RS_GROUP(RS_LSL, 0, 0, 3, RS_CSC, 1, 0, 1, 0, 0, 1, 2, 3, 0, 0),        /*  0- 3 LSL LSL RSR RSR      :247-250 */ \
    T2D_RS_GROUP(RS_LSR, 0, 0, 3, RS_CSC, 1, 0, -1, 0, 0, 1, 2, 3, 0, 0),       /*  4- 7 LSR LSR RSL RSL      :251-254 */ \
    T2D_RS_GROUP(RS_LRL, 0, 0, 3, RS_CCC, 1, -1, 1, 0, 0, 1, -2, 3, 0, 0),      /*  8-11 LRL, matrix1         :298-301 */ \
    T2D_RS_GROUP(RS_LRL, 1, 0, 3, RS_CCC, 1, -1, 1, 0, 0, 1, -2, -3, 0, 0),     /* 12-15 LRL, matrix2         :302-305 */ \
    T2D_RS_GROUP(RS_LRL, 2, 0, 3, RS_CCC, 1, -1, 1, 0, 0, -1, -2, 3, 0, 0),     /* 16-19 LRL, matrix3         :306-309 */ \
    T2D_RS_GROUP(RS_LRLR_A, 0, 0, 4, RS_CCCC, 1, -1, 1, -1, 0, 1, 2, -2, -3, 0), /* 20-23 LRLR, matrix1        :364-367 */ \
    T2D_RS_GROUP(RS_LRLR_B, 0, 0, 4, RS_CCCC, 1, -1, 1, -1, 0, 1, -2, -2, 3, 0), /* 24-27 LRLR, matrix2        :368-371 */ \
    T2D_RS_GROUP(RS_LRSL, 0, 0, 4, RS_CCSC, 1, -1, 0, 1, 0, 1, -4, -2, -3, 0),  /* 28-31 LRSL, matrix1        :431-434 */ \
    T2D_RS_GROUP(RS_LRSL, 0, 4, 4, RS_CCSC, 1, 0, -1, 1, 0, -3, -2, -4, 1, 0),  /* 32-35 LSRL, matrix2        :435-438 */ \
    T2D_RS_GROUP(RS_LRSR, 0, 0, 4, RS_CCSC, 1, -1, 0, -1, 0, 1, -4, -2, -3, 0), /* 36-39 LRSR, matrix1        :439-442 */ \
    T2D_RS_GROUP(RS_LRSR, 0, 4, 4, RS_CCSC, -1, 0, -1, 1, 0, -3, -2, -4, 1, 0), /* 40-43 RSRL, matrix2        :443-446 */ \
    T2D_RS_GROUP(RS_LRSLR, 0, 0, 5, RS_CCSCC, 1, -1, 0, 1, -1, 1, -4, 2, -4, 3)  /* 44-47 LRSLR                :487-490 */

#ifdef __HIPCC__
// _M (:164-173): np.mod(theta, 2 pi), then into (-pi, pi]
T2D_DEV double rs_mod(double theta) {
    const double pi = 3.141592653589793;
    double phi = mod_two_pi(theta);
    if (phi > pi) phi -= 2.0 * pi;
    if (phi < -pi) phi += 2.0 * pi;
    return phi;
}
T2D_DEV double rs_hypot(double x, double y) { return __builtin_sqrt(x * x + y * y); }   // _R's r (:160)
// arcsin / arccos through atan2 and a square root
T2D_DEV double rs_asin(double z) { return atan2_det(z, __builtin_sqrt((1.0 - z) * (1.0 + z))); }
T2D_DEV double rs_acos(double z) { return atan2_det(__builtin_sqrt((1.0 - z) * (1.0 + z)), z); }

// _tau_omega (:175-187)
T2D_DEV void rs_tau_omega(double u, double v, double xi, double eta, double phi, double& tau, double& omega) {
    const double pi = 3.141592653589793;
    const double delta = rs_mod(u - v);
    double su, cu, sd, cd, sv, cv;
    sincos_det(u, su, cu);
    sincos_det(delta, sd, cd);
    sincos_det(v, sv, cv);
    const double A = su - sd, B = cu - cd - 1.0;
    const double t1 = atan2_det(eta * A - xi * B, xi * A + eta * B);
    const double t2 = 2.0 * (cd - cv - cu) + 3.0;
    tau = t2 < 0.0 ? rs_mod(t1 + pi) : rs_mod(t1);
    omega = rs_mod(tau - u + v - phi);
}

// The base formula `f` on (x, y, phi) with s = sin phi, c = cos phi: false = the reference returns None.
T2D_DEV bool rs_formula(int f, int variant, double x, double y, double phi, double s, double c, double& t, double& u, double& v) {
    const double pi = 3.141592653589793, pio2 = 1.5707963267948966;
    switch (f) {
    case RS_LSL: {   // LpSpLp :208-219
        const double ex = x - s, ey = y - 1.0 + c;
        u = rs_hypot(ex, ey);
        t = atan2_det(ey, ex);
        if (t < 0.0) return false;
        v = rs_mod(phi - t);
        return !(v < 0.0);
    }
    case RS_LSR: {   // LpSpRp :221-236
        const double ex = x + s, ey = y - 1.0 - c;
        const double u1 = rs_hypot(ex, ey), t1 = atan2_det(ey, ex);
        if (u1 * u1 < 4.0) return false;
        u = __builtin_sqrt(u1 * u1 - 4.0);
        const double theta = atan2_det(2.0, u);
        t = rs_mod(t1 + theta);
        v = rs_mod(t - phi);
        return !(t < 0.0 || v < 0.0);
    }
    case RS_LRL: {   // LRL :260-278
        const double xi = x - s, eta = y - 1.0 + c;
        const double u1 = rs_hypot(xi, eta), theta = atan2_det(eta, xi);
        if (u1 > 4.0) return false;
        const double A = pi - rs_asin(u1 / 4.0);
        t = rs_mod(theta + A);
        u = rs_mod(2.0 * A);
        v = rs_mod(phi - t + u);
        const double s0 = variant == 2 ? -1.0 : 1.0, s2 = variant == 1 ? -1.0 : 1.0;
        return !(t * s0 < 0.0 || u * -1.0 < 0.0 || v * s2 < 0.0);
    }
    case RS_LRLR_A: {   // LpRpLnRn :315-330
        const double xi = x + s, eta = y - 1.0 - c;
        const double rho = (2.0 + __builtin_sqrt(xi * xi + eta * eta)) / 4.0;
        if (rho > 1.0 || rho < 0.0) return false;
        u = rs_acos(rho);
        rs_tau_omega(u, -u, xi, eta, phi, t, v);
        return !(t < 0.0 || v > 0.0);
    }
    case RS_LRLR_B: {   // LpRnLnRp :332-350
        const double xi = x + s, eta = y - 1.0 - c;
        const double rho = (20.0 - xi * xi - eta * eta) / 16.0;
        if (rho > 1.0 || rho < 0.0) return false;
        u = -rs_acos(rho);
        if (u < -pio2) return false;
        rs_tau_omega(u, u, xi, eta, phi, t, v);
        return !(t < 0.0 || v < 0.0);
    }
    case RS_LRSL: {   // LpRnSnLn :377-394
        const double xi = x - s, eta = y - 1.0 + c;
        const double rho = rs_hypot(xi, eta), theta = atan2_det(eta, xi);
        if (rho < 2.0) return false;
        const double r = __builtin_sqrt(rho * rho - 4.0);
        u = 2.0 - r;
        t = rs_mod(theta + atan2_det(r, -2.0));
        v = rs_mod(phi - pio2 - t);
        return !(t < 0.0 || u > 0.0 || v > 0.0);
    }
    case RS_LRSR: {   // LpRnSnRn :396-412
        const double xi = x + s, eta = y - 1.0 - c;
        const double rho = rs_hypot(-eta, xi), theta = atan2_det(xi, -eta);
        if (rho < 2.0) return false;
        t = theta;
        u = 2.0 - rho;
        v = rs_mod(t + pio2 - phi);
        return !(t < 0.0 || u > 0.0 || v > 0.0);
    }
    default: {   // LpRnSnLnRp :452-472
        const double xi = x + s, eta = y - 1.0 - c;
        const double rho = rs_hypot(xi, eta), theta = atan2_det(eta, xi);
        if (rho < 2.0) return false;
        t = rs_mod(theta - rs_acos(-2.0 / rho));
        if (t <= 0.0) return false;
        double st, ct;
        sincos_det(t, st, ct);
        u = 4.0 - (xi + 2.0 * ct) / st;
        v = rs_mod(t - phi);
        return !(u > 0.0 || v < 0.0);
    }
    }
}

// The normalised goal of get_all_path (:513-517) and what every slot needs of it.
struct RsGoal {
    double x, y, phi, s, c;   // s, c = sin phi, cos phi
    bool finite;
};
T2D_DEV RsGoal rs_normalise(double sx, double sy, double sh, double ex, double ey, double eh, double radius) {
    RsGoal g;
    const double dx = (ex - sx) / radius, dy = (ey - sy) / radius;
    double ss, cs;
    sincos_det(sh, ss, cs);
    g.x = dx * cs + dy * ss;
    g.y = -dx * ss + dy * cs;
    g.phi = eh - sh;
    sincos_det(g.phi, g.s, g.c);
    g.finite = __builtin_isfinite(g.x) && __builtin_isfinite(g.y) && __builtin_isfinite(g.phi);
    return g;
}

// Slot `sl` of get_all_path for the normalised goal: false = None.  seg[i] = signs[i] * segments[i] of ReedsSheppPath (:35-42) in
// units of the radius, zero padded; sum = np.abs(segments).sum() (:44, added in index order).  A goal that is not finite
// has no valid slot.
T2D_DEV bool rs_slot(const RsSlot& sl, const RsGoal& g, double seg[kRsMaxSeg], double& sum) {
    const double pio2 = 1.5707963267948966;
    double x = g.x, y = g.y, phi = g.phi, s = g.s, c = g.c;
    if (sl.xform & 4) {   // _backward (:195-198)
        const double xb = x * c + y * s, yb = x * s - y * c;
        x = xb;
        y = yb;
    }
    if (sl.xform & 2) { y = -y; phi = -phi; s = -s; }   // _reflect (:192-193)
    if (sl.xform & 1) { x = -x; phi = -phi; s = -s; }   // _time_flip (:189-190)
    double tuv[4] = {0.0, 0.0, 0.0, 1.0};
    const bool ok = g.finite && rs_formula(sl.formula, sl.variant, x, y, phi, s, c, tuv[0], tuv[1], tuv[2]);
    sum = 0.0;
#pragma unroll
    for (int i = 0; i < kRsMaxSeg; ++i) {
        const int cc = sl.col[i];
        double m = 0.0;
        if (ok && cc != 0) {
            const int src = (cc < 0 ? -cc : cc) - 1;
            const double val = src == 0 ? tuv[0] : src == 1 ? tuv[1] : src == 2 ? tuv[2] : pio2;
            m = __builtin_fabs(val);
            sum += m;
        }
        seg[i] = cc < 0 ? -m : m;
    }
    return ok;
}

// One piece of a word from the pose (x, y, yaw): steer = +1 L / -1 R / 0 S, `d` = the signed distance, `r` the radius (all
// in one unit).  What the sweep, the specification (tests/rs_ref.py) and the word-integration test all use.
T2D_DEV void rs_advance(double& x, double& y, double& yaw, int steer, double d, double r) {
    double s0, c0;
    sincos_det(yaw, s0, c0);
    if (steer == 0) {
        x += d * c0;
        y += d * s0;
        return;
    }
    const double l = (double)steer, yaw1 = yaw + l * d / r;
    double s1, c1;
    sincos_det(yaw1, s1, c1);
    x += l * r * (s1 - s0);
    y += l * r * (c0 - c1);
    yaw = yaw1;
}
#endif   // __HIPCC__

}  // namespace t2d
