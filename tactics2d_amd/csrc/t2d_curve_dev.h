// t2d_curve_dev.h -- Dubins candidate paths (interpolator/dubins.py) and the sampled curve lines of a Dubins or Reeds-Shepp
// word (DubinsPath.get_curve_line dubins.py:28-104, ReedsSheppPath.get_curve_line reeds_shepp.py:46-139, Circle.get_arc
// geometry/circle.py:106-139) as device functions.  fp64 throughout, one rounding per operation, the library's own sincos /
// atan2 / mod 2 pi; tests/curve_ref.py states the same operations in numpy.  DESIGN.md 4.18.
//
// Dubins.get_all_path (:240-273) returns six slots in a fixed order: LRL, RLR, LSL, RSL, RSR, LSR.  T2D_DUBINS_SLOT_ROWS is
// the one statement of their letters.  _LRL (:216-231) is restated AS WRITTEN for lrl_rule 0 (t = mod(-alpha + tmp + p / 2):
// its curve misses the goal) and with the family's sign (-alpha - tmp + p / 2) for lrl_rule 1, which is build-defined.
#pragma once
#include "t2d_math.h"
#include "t2d_rs_dev.h"

namespace t2d {

constexpr int kDubinsSlots = 6;
enum { DUBINS_LRL = 0, DUBINS_RLR, DUBINS_LSL, DUBINS_RSL, DUBINS_RSR, DUBINS_LSR };
// letters L = 1, S = 0, R = -1 of slots 0..5 (:264-271)
#define T2D_DUBINS_SLOT_ROWS {1, -1, 1}, {-1, 1, -1}, {1, 0, 1}, {-1, 0, 1}, {-1, 0, -1}, {1, 0, -1}

// One curve of t2d_curve_lines / t2d_curve_routes: 48 bytes.  seg[i]: the signed length of segment i in units of the radius
// (the sign is the reference's `forward` under the Reeds-Shepp rule; the Dubins rule reads |seg|, as DubinsPath does);
// letter[i]: +1 L, -1 R, 0 S; n_seg 0 .. 5.
struct CurveWord {
    double seg[kRsMaxSeg];
    int8_t letter[kRsMaxSeg];
    int8_t n_seg;
    int8_t pad[2];
};
static_assert(sizeof(CurveWord) == 48, "one 48-byte record per curve");

enum { CURVE_RULE_DUBINS = 0, CURVE_RULE_RS = 1 };
enum { CURVE_POINT = 0, CURVE_LINE, CURVE_ARC };
constexpr double kCurveMaxCount = 1073741824.0;   // a segment's point count saturates here (2^30)

// What the lanes need of one curve: per segment its kind, point count and first point index, and the constants of its points.
//   CURVE_POINT  the single point (p0, p1) with yaw h
//   CURVE_LINE   linspace from (p0, p1) in steps (q0, q1) whose last point is (ex, ey): a straight, or the two-point stand-in of
//                a Reeds-Shepp arc that sampled fewer than two points (reeds_shepp.py:91-94)
//   CURVE_ARC    (p0, p1) + r (cos, sin)(q0 + k q1): the circle's centre, the start angle, numpy's arange increment
// yaw of point k of n: h + k hs, the last one of n > 1 is he (np.linspace).
struct CurvePlan {
    int kind[kRsMaxSeg], count[kRsMaxSeg];
    long long first[kRsMaxSeg + 1];
    double p0[kRsMaxSeg], p1[kRsMaxSeg], q0[kRsMaxSeg], q1[kRsMaxSeg], ex[kRsMaxSeg], ey[kRsMaxSeg];
    double h[kRsMaxSeg], hs[kRsMaxSeg], he[kRsMaxSeg];
    double end[3];
    int n_seg;
};

#ifdef __HIPCC__
// np.arange(start, stop, delta) as Circle.get_arc calls it: ceil((stop - start) / delta) values (none where that is <= 0),
// value k = start + k * ((start + delta) - start).  One statement for curve_plan below and the plan-view arcs of t2d_road_dev.h.
T2D_DEV double arange_count(double start, double stop, double delta) {
    const double cnt = __builtin_ceil((stop - start) / delta);
    return cnt > 0.0 ? cnt : 0.0;
}
T2D_DEV double arange_increment(double start, double delta) { return (start + delta) - start; }

// ---- Dubins -------------------------------------------------------------------------------------------------------------------
// The normalised query of get_all_path (:259-262) with the sines and cosines every word needs.
struct DubinsGoal {
    double alpha, beta, d, sa, ca, sb, cb, cab;
    bool finite;
};
T2D_DEV DubinsGoal dubins_normalise(double sx, double sy, double sh, double ex, double ey, double eh, double radius) {
    DubinsGoal g;
    const double dx = ex - sx, dy = ey - sy;
    const double theta = atan2_det(dy, dx);
    g.d = __builtin_sqrt(dx * dx + dy * dy) / radius;
    g.alpha = mod_two_pi(sh - theta);
    g.beta = mod_two_pi(eh - theta);
    sincos_det(g.alpha, g.sa, g.ca);
    sincos_det(g.beta, g.sb, g.cb);
    double s;
    sincos_det(g.alpha - g.beta, s, g.cab);
    g.finite = __builtin_isfinite(g.d) && __builtin_isfinite(g.alpha) && __builtin_isfinite(g.beta);
    return g;
}

// Slot `slot` of get_all_path: false = None.  (t, p, q) in units of the radius.
T2D_DEV bool dubins_slot(int slot, const DubinsGoal& g, int lrl_rule, double& t, double& p, double& q) {
    const double a = g.alpha, b = g.beta, d = g.d, sa = g.sa, ca = g.ca, sb = g.sb, cb = g.cb, cab = g.cab;
    const double d2 = d * d;
    t = p = q = 0.0;
    if (!g.finite) return false;
    switch (slot) {
    case DUBINS_LRL: {   // :216-231
        const double disc = (((6.0 - d2) + 2.0 * cab) + (2.0 * d) * (-sa + sb)) / 8.0;
        if (__builtin_fabs(disc) > 1.0) return false;
        p = mod_two_pi(kTwoPi - rs_acos(disc));
        const double tmp = atan2_det(ca - cb, (d + sa) - sb);
        t = lrl_rule ? mod_two_pi((-a - tmp) + p / 2.0) : mod_two_pi((-a + tmp) + p / 2.0);
        q = mod_two_pi(((b - a) - t) + p);
        return true;
    }
    case DUBINS_RLR: {   // :200-214
        const double disc = (((6.0 - d2) + 2.0 * cab) + (2.0 * d) * (sa - sb)) / 8.0;
        if (__builtin_fabs(disc) > 1.0) return false;
        const double tmp = atan2_det(ca - cb, (d - sa) + sb);
        p = mod_two_pi(kTwoPi - rs_acos(disc));
        t = mod_two_pi((a - tmp) + p / 2.0);
        q = mod_two_pi(((a - b) - t) + p);
        return true;
    }
    case DUBINS_LSL: {   // :165-179
        const double disc = ((2.0 + d2) - 2.0 * cab) + (2.0 * d) * (sa - sb);
        if (disc < 0.0) return false;
        const double tmp = atan2_det(-ca + cb, (d + sa) - sb);
        t = mod_two_pi(-(a - tmp));
        p = __builtin_sqrt(disc);
        q = mod_two_pi(b - tmp);
        return true;
    }
    case DUBINS_RSL: {   // :146-163
        const double disc = ((-2.0 + d2) + 2.0 * cab) - (2.0 * d) * (sa + sb);
        if (disc < 0.0) return false;
        p = __builtin_sqrt(disc);
        const double tmp = atan2_det(ca + cb, (d - sa) - sb) - atan2_det(2.0, p);
        t = mod_two_pi(a - tmp);
        q = mod_two_pi(b - tmp);
        return true;
    }
    case DUBINS_RSR: {   // :130-144
        const double disc = ((2.0 + d2) - 2.0 * cab) + (2.0 * d) * (-sa + sb);
        if (disc < 0.0) return false;
        const double tmp = atan2_det(ca - cb, (d - sa) + sb);
        t = mod_two_pi(a - tmp);
        p = __builtin_sqrt(disc);
        q = mod_two_pi(-(b - tmp));
        return true;
    }
    default: {   // LSR :181-198
        const double disc = ((-2.0 + d2) + 2.0 * cab) + (2.0 * d) * (sa + sb);
        if (disc < 0.0) return false;
        p = __builtin_sqrt(disc);
        const double tmp = -atan2_det(ca + cb, (d + sa) + sb) + atan2_det(2.0, p);
        t = mod_two_pi(-a + tmp);
        q = mod_two_pi(-b + tmp);
        return true;
    }
    }
}

// ---- curve lines --------------------------------------------------------------------------------------------------------------
// The serial part of get_curve_line: the word walked segment by segment from the start pose.  false = no curve (a word of 0
// segments or more than five, or a start or segment that is not finite).  `total` = the curve's point count.
T2D_DEV bool curve_plan(const CurveWord& w, double sx, double sy, double sh, double radius, double step, int rule, CurvePlan& c,
                        long long& total) {
    const double pio2 = 3.141592653589793 / 2.0;
    total = 0;
    c.n_seg = 0;
    const int n = w.n_seg;
    bool ok = n >= 1 && n <= kRsMaxSeg && __builtin_isfinite(sx) && __builtin_isfinite(sy) && __builtin_isfinite(sh);
    for (int i = 0; i < kRsMaxSeg; ++i) ok = ok && (i >= n || __builtin_isfinite(w.seg[i]));
    if (!ok) return false;
    c.n_seg = n;
    double px = sx, py = sy, h = sh;
    for (int i = 0; i < n; ++i) {
        // (the Dubins rule takes abs(segment) everywhere, dubins.py:94-98: a negative length drives forward there)
        const double a = __builtin_fabs(w.seg[i]), fwd = rule == CURVE_RULE_RS && w.seg[i] < 0.0 ? -1.0 : 1.0;
        const int letter = w.letter[i];
        c.first[i] = total;
        c.p0[i] = px;
        c.p1[i] = py;
        c.q0[i] = c.q1[i] = 0.0;
        c.ex[i] = px;
        c.ey[i] = py;
        c.h[i] = c.he[i] = h;
        c.hs[i] = 0.0;
        c.kind[i] = CURVE_POINT;
        double cnt = 1.0;
        if (!(a < 1e-15)) {
            double sn, cs;
            if (letter == 0) {   // get_straight_line
                sincos_det(h, sn, cs);
                const double ex = px + ((cs * radius) * a) * fwd, ey = py + ((sn * radius) * a) * fwd;
                const double dx = ex - px, dy = ey - py;
                const double len = __builtin_sqrt(dx * dx + dy * dy);
                cnt = __builtin_ceil(len / step);
                const double lo = rule == CURVE_RULE_RS ? 2.0 : 1.0;
                cnt = cnt > lo ? cnt : lo;            // max(1, ...) / max(2, ...); a NaN count cannot arise from finite inputs
                cnt = cnt < kCurveMaxCount ? cnt : kCurveMaxCount;
                c.kind[i] = CURVE_LINE;
                c.q0[i] = cnt > 1.0 ? dx / (cnt - 1.0) : 0.0;
                c.q1[i] = cnt > 1.0 ? dy / (cnt - 1.0) : 0.0;
                c.ex[i] = ex;
                c.ey[i] = ey;
                px = ex;
                py = ey;
            } else {             // get_arc
                const bool left = letter > 0;
                const bool cw = rule == CURVE_RULE_RS ? (left ? fwd < 0.0 : fwd > 0.0) : !left;
                sincos_det(left ? h + pio2 : h - pio2, sn, cs);
                const double cx = px + radius * cs, cy = py + radius * sn;   // get_circle_by_tangent_vector
                const double a0 = left ? h - pio2 : h + pio2;
                const double delta = cw ? -step / radius : step / radius;
                const double stop = cw ? a0 - a : a0 + a;
                cnt = arange_count(a0, stop, delta);
                cnt = cnt < kCurveMaxCount ? cnt : kCurveMaxCount;
                const double h_end = cw ? h - a : h + a;
                sincos_det(stop, sn, cs);
                const double ex = cx + cs * radius, ey = cy + sn * radius;
                if (rule == CURVE_RULE_RS && cnt < 2.0) {      // [point, end_point] with yaw [h, h_end]
                    cnt = 2.0;
                    c.kind[i] = CURVE_LINE;
                    c.ex[i] = ex;
                    c.ey[i] = ey;
                } else if (cnt < 1.0) {                        // [point]
                    cnt = 1.0;
                } else {
                    c.kind[i] = CURVE_ARC;
                    c.p0[i] = cx;
                    c.p1[i] = cy;
                    c.q0[i] = a0;
                    c.q1[i] = arange_increment(a0, delta);
                }
                c.he[i] = h_end;
                c.hs[i] = cnt > 1.0 ? (h_end - h) / (cnt - 1.0) : 0.0;
                px = ex;
                py = ey;
                h = h_end;
            }
        }
        c.count[i] = (int)cnt;
        total += (long long)cnt;
    }
    c.first[n] = total;
    c.end[0] = px;
    c.end[1] = py;
    c.end[2] = h;
    return true;
}

// Point `k` of the curve (0 <= k < total).  `c` lives in LDS: every index below is a runtime one.
T2D_DEV void curve_point(const CurvePlan& c, double radius, long long k, double& x, double& y, double& yaw) {
    int i = 0;
    while (i + 1 < c.n_seg && k >= c.first[i + 1]) ++i;
    const int j = (int)(k - c.first[i]), n = c.count[i];
    const bool last = n > 1 && j == n - 1;
    const double dj = (double)j;
    yaw = last ? c.he[i] : c.h[i] + dj * c.hs[i];
    const int kind = c.kind[i];
    if (kind == CURVE_ARC) {
        double sn, cs;
        sincos_det(c.q0[i] + dj * c.q1[i], sn, cs);
        x = c.p0[i] + cs * radius;
        y = c.p1[i] + sn * radius;
    } else if (kind == CURVE_LINE) {
        x = last ? c.ex[i] : c.p0[i] + dj * c.q0[i];
        y = last ? c.ey[i] : c.p1[i] + dj * c.q1[i];
    } else {
        x = c.p0[i];
        y = c.p1[i];
    }
}
#endif   // __HIPCC__

}  // namespace t2d
