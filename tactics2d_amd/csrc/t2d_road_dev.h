// t2d_road_dev.h -- Spiral.get_curve (interpolator/spiral.py), ParamPoly3.get_curve (interpolator/param_poly3.py) and the plan-view
// reference line of an OpenDRIVE road (map/parser/parse_xodr.py: _sample_line :256, _sample_spiral :280, _sample_arc :307,
// _sample_poly3 :351, _sample_param_poly3 :387, _sample_geometry :447 and the head of load_road :773-809) as device functions.
// fp64 throughout, one rounding per operation in the reference's order, the library's own sincos and Fresnel integrals;
// tests/road_ref.py states the same operations in numpy.  DESIGN.md 4.20.
//
// AS WRITTEN, and kept:
//   * Spiral is the Euler spiral only for start_curvature == 0 and gamma > 0: it scales by |gamma| and never mirrors, and it
//     shifts theta_0 by -k0^2 / (2 gamma) but not the Fresnel argument.  SPIRAL_STANDARD is the clothoid
//     heading + k0 s + gamma s^2 / 2 through the shifted argument (build-defined); the line and arc branches are the same.
//   * a plan-view spiral is sampled at 100 points whatever its length, so one shorter than about 1.98 m loses every point but
//     its first to the 0.02 m filter of load_road.
//   * an arc never samples its end point (np.arange), a line and a poly3 always do.
// BUILD-DEFINED: u ** 3 of numpy goes through libm's pow; here and in the specification it is (u * u) * u, at most one ulp from
// it.  speed_sq ** 1.5 likewise is speed_sq * sqrt(speed_sq).
#pragma once
#include "t2d_curve_dev.h"

namespace t2d {

enum { GEOM_LINE = 0, GEOM_SPIRAL = 1, GEOM_ARC = 2, GEOM_POLY3 = 3, GEOM_PARAM_POLY3 = 4 };
enum { SPIRAL_REFERENCE = 0, SPIRAL_STANDARD = 1 };
enum { P_RANGE_NORMALIZED = 0, P_RANGE_ARC_LENGTH = 1 };
constexpr int kPlanviewMaxGeom = 64;          // one lane plans one geometry
constexpr int kPlanviewMaxRaw = 1 << 20;      // raw points of one road (100 km of lines); more: the road has no line
constexpr int kPlanviewSpiralPoints = 100;    // Spiral.get_curve's default n_interpolation, which _sample_spiral takes
constexpr int kRoadWave = 64, kRoadsPerBlock = 4, kRoadBlock = kRoadWave * kRoadsPerBlock;

// One <geometry> of a <planView>: 112 bytes.  par: spiral {curvStart, curvEnd}, arc {curvature}, poly3 {a, b, c, d},
// paramPoly3 {aU, bU, cU, dU, aV, bV, cV, dV}; p_range is read for paramPoly3 only.
struct PlanviewRecord {
    int32_t kind, p_range;
    double s, x, y, hdg, length;
    double par[8];
};
static_assert(sizeof(PlanviewRecord) == 112, "one 112-byte record per geometry");

#ifdef __HIPCC__
// np.linspace(a, b, n)[j]: j * ((b - a) / (n - 1)) + a, the last one b itself; n == 1 gives a
T2D_DEV double linspace_at(double a, double b, int n, int j) {
    if (n < 2) return a;
    if (j == n - 1) return b;
    return (double)j * ((b - a) / (double)(n - 1)) + a;
}

// Point j of Spiral.get_curve(length, (x0, y0), h, k0, gamma, n): the three branches of spiral.py:53-87.
T2D_DEV void spiral_point(double length, double x0, double y0, double h, double k0, double gamma, int n, int j, int rule, double& x,
                          double& y) {
    const double s = linspace_at(0.0, length, n, j);
    double sn, cs;
    if (gamma == 0.0 && k0 == 0.0) {
        sincos_det(h, sn, cs);
        x = x0 + s * cs;
        y = y0 + s * sn;
    } else if (gamma == 0.0) {
        double s1, c1;
        sincos_det(h, sn, cs);
        sincos_det(h + k0 * s, s1, c1);
        const double inv = 1.0 / k0;
        x = x0 + inv * (s1 - sn);
        y = y0 + inv * (cs - c1);
    } else {
        const double pi = 3.141592653589793, ag = __builtin_fabs(gamma);
        const double a = __builtin_sqrt(pi / ag), scale = __builtin_sqrt(ag / pi);
        sincos_det(h - (k0 * k0) / (2.0 * gamma), sn, cs);
        double S, C;
        if (rule == SPIRAL_STANDARD) {
            // int_0^s exp(i (h + k0 t + gamma t^2 / 2)) dt = exp(i theta_0) a [C(t) - C(t0) + i sgn(gamma) (S(t) - S(t0))] with
            // w0 = k0 / gamma, t = (s + w0) / a, t0 = w0 / a
            const double w0 = k0 / gamma;
            double S0, C0;
            fresnel_det((s + w0) * scale, S, C);
            fresnel_det(w0 * scale, S0, C0);
            C = C - C0;
            S = gamma < 0.0 ? S0 - S : S - S0;
        } else {
            fresnel_det(s * scale, S, C);
        }
        const double re = a * C, im = a * S;
        x = x0 + (re * cs - im * sn);
        y = y0 + (re * sn + im * cs);
    }
}

// max(2, int(length / 0.1) + plus) of a finite length >= 0, as a double saturating at `cap`
T2D_DEV double tenth_count(double length, double plus, double cap) {
    const double q = length / 0.1;
    if (!(q < cap)) return cap;
    const double n = __builtin_trunc(q) + plus;
    return n > 2.0 ? n : 2.0;
}

// Point j of ParamPoly3.get_curve's n points (param_poly3.py:52-65) and, for the plan view, the curvature of
// _sample_param_poly3 (:431-444).  c = {aU, bU, cU, dU, aV, bV, cV, dV}.
T2D_DEV void param_poly3_point(double length, double x0, double y0, double h, const double* c, int arc_length, int n, int j, double& x,
                               double& y, double& kappa) {
    const double p = linspace_at(0.0, arc_length ? length : 1.0, n, j);
    const double p2 = p * p, p3 = p2 * p;
    const double u = ((c[0] + c[1] * p) + c[2] * p2) + c[3] * p3;
    const double v = ((c[4] + c[5] * p) + c[6] * p2) + c[7] * p3;
    double sn, cs;
    sincos_det(h, sn, cs);
    x = (u * cs + v * (-sn)) + x0;     // np.dot(uv, R.T) + start
    y = (u * sn + v * cs) + y0;
    const double dU = (c[1] + (2.0 * c[2]) * p) + (3.0 * c[3]) * p2, dV = (c[5] + (2.0 * c[6]) * p) + (3.0 * c[7]) * p2;
    const double d2U = 2.0 * c[2] + (6.0 * c[3]) * p, d2V = 2.0 * c[6] + (6.0 * c[7]) * p;
    double sp = dU * dU + dV * dV;
    sp = sp < 1e-12 ? 1e-12 : sp;
    kappa = (dU * d2V - dV * d2U) / (sp * __builtin_sqrt(sp));
}

// ---- the plan view ------------------------------------------------------------------------------------------------------------
// Does the sampler of `r` read only finite values, a length >= 0 and a known kind?
T2D_DEV bool geom_valid(const PlanviewRecord& r) {
    const int used = r.kind == GEOM_LINE ? 0 : r.kind == GEOM_SPIRAL ? 2 : r.kind == GEOM_ARC ? 1 : r.kind == GEOM_POLY3 ? 4 : 8;
    bool ok = r.kind >= GEOM_LINE && r.kind <= GEOM_PARAM_POLY3;
    ok = ok && __builtin_isfinite(r.s) && __builtin_isfinite(r.x) && __builtin_isfinite(r.y) && __builtin_isfinite(r.hdg) &&
         __builtin_isfinite(r.length) && r.length >= 0.0;
    for (int i = 0; i < 8; ++i) ok = ok && (i >= used || __builtin_isfinite(r.par[i]));
    if (r.kind == GEOM_PARAM_POLY3) ok = ok && (r.p_range == P_RANGE_NORMALIZED || r.p_range == P_RANGE_ARC_LENGTH);
    return ok;
}

T2D_DEV bool geom_is_line(const PlanviewRecord& r) { return r.kind == GEOM_LINE || (r.kind == GEOM_ARC && __builtin_fabs(r.par[0]) < 1e-9); }

// The number of points the geometry's _sample_* returns, before _sample_geometry pops; kPlanviewMaxRaw + 1 where it is more than
// kPlanviewMaxRaw.
T2D_DEV int geom_raw_count(const PlanviewRecord& r) {
    const double cap = (double)(kPlanviewMaxRaw + 1), L = r.length;
    double n;
    if (geom_is_line(r)) {
        n = L <= 0.0 ? 1.0 : tenth_count(L, 1.0, cap);
    } else if (r.kind == GEOM_SPIRAL) {
        n = L < 1e-6 ? 1.0 : (double)kPlanviewSpiralPoints;
    } else if (r.kind == GEOM_ARC) {
        const double radius = __builtin_fabs(1.0 / r.par[0]);
        const double angle = L / radius, pio2 = 3.141592653589793 / 2.0;
        const bool cw = r.par[0] < 0.0;
        const double start = cw ? r.hdg + pio2 : r.hdg - pio2;
        n = arange_count(start, cw ? start - angle : start + angle, cw ? -0.1 / radius : 0.1 / radius);
        n = n < cap ? n : cap;
    } else if (r.kind == GEOM_POLY3) {
        n = tenth_count(L, 1.0, cap);
    } else {
        n = tenth_count(L, 0.0, cap);
    }
    return (int)n;
}

// Point j of the geometry's n raw points and its curvature.
T2D_DEV void geom_point(const PlanviewRecord& r, int n, int j, int rule, double& x, double& y, double& kappa) {
    double sn, cs;
    if (geom_is_line(r)) {
        kappa = 0.0;
        if (r.length <= 0.0) {
            x = r.x;
            y = r.y;
            return;
        }
        const double s = linspace_at(0.0, r.length, n, j);
        sincos_det(r.hdg, sn, cs);
        x = r.x + s * cs;
        y = r.y + s * sn;
    } else if (r.kind == GEOM_SPIRAL) {
        const double k0 = r.par[0], k1 = r.par[1];
        if (r.length < 1e-6) {
            x = r.x;
            y = r.y;
            kappa = k0;
            return;
        }
        spiral_point(r.length, r.x, r.y, r.hdg, k0, (k1 - k0) / r.length, kPlanviewSpiralPoints, j, rule, x, y);
        kappa = linspace_at(k0, k1, kPlanviewSpiralPoints, j);
    } else if (r.kind == GEOM_ARC) {
        const double k = r.par[0], radius = __builtin_fabs(1.0 / k), pio2 = 3.141592653589793 / 2.0;
        const bool cw = k < 0.0;
        sincos_det(cw ? r.hdg - pio2 : r.hdg + pio2, sn, cs);          // get_circle_by_tangent_vector, side L for k > 0
        const double cx = r.x + cs * radius, cy = r.y + sn * radius;
        const double start = cw ? r.hdg + pio2 : r.hdg - pio2;           // hdg - pi/2 sign(k)
        const double inc = arange_increment(start, cw ? -0.1 / radius : 0.1 / radius);
        sincos_det(start + (double)j * inc, sn, cs);
        x = cx + cs * radius;
        y = cy + sn * radius;
        kappa = k;
    } else if (r.kind == GEOM_POLY3) {
        const double a = r.par[0], b = r.par[1], c = r.par[2], d = r.par[3];
        const double u = linspace_at(0.0, r.length, n, j);
        const double u2 = u * u;
        const double v = ((a + b * u) + c * u2) + d * (u2 * u);
        sincos_det(r.hdg, sn, cs);
        x = (r.x + u * cs) - v * sn;
        y = (r.y + u * sn) + v * cs;
        const double dv = (b + (2.0 * c) * u) + (3.0 * d) * u2, d2v = 2.0 * c + (6.0 * d) * u;
        double sp = 1.0 + dv * dv;
        sp = sp < 1e-12 ? 1e-12 : sp;
        kappa = d2v / (sp * __builtin_sqrt(sp));
    } else {
        param_poly3_point(r.length, r.x, r.y, r.hdg, r.par, r.p_range == P_RANGE_ARC_LENGTH, n, j, x, y, kappa);
    }
}

// What one wave keeps of its road in LDS: the records, and per geometry the point count of its sampler (raw), the one after
// _sample_geometry's pop (count) and the road's raw index of its first point.
struct RoadWork {
    PlanviewRecord rec[kPlanviewMaxGeom];
    int raw[kPlanviewMaxGeom], count[kPlanviewMaxGeom];
    int first[kPlanviewMaxGeom + 1];
    int total;   // raw points of the road; -1: the road has no line (a refusal)
};

// Lane g < n_geom plans geometry g of road `e`.  All 64 lanes call; the block's barrier follows.
T2D_DEV void road_plan(RoadWork& w, const PlanviewRecord* rec, const int32_t* n_geom, int max_geom, int e, int rule, int lane) {
    const int ng = n_geom[e];
    const bool road_ok = ng >= 1 && ng <= max_geom;
    int cnt = 0, raw = 0;
    bool ok = true;
    if (road_ok && lane < ng) {
        const PlanviewRecord r = rec[(size_t)e * max_geom + lane];
        w.rec[lane] = r;
        ok = geom_valid(r);
        if (ok) {
            cnt = geom_raw_count(r);
            raw = cnt;
            if (cnt > kPlanviewMaxRaw) {
                ok = false;
                cnt = 0;
            } else if (cnt >= 2) {      // _sample_geometry :471: the last point goes if it equals the one before it
                double xa, ya, xb, yb, k;
                geom_point(r, cnt, cnt - 1, rule, xa, ya, k);
                geom_point(r, cnt, cnt - 2, rule, xb, yb, k);
                if (xa == xb && ya == yb) --cnt;
            }
        }
    }
    const bool all_ok = road_ok && __ballot(!ok) == 0ull;
    int sum = all_ok ? cnt : 0;       // inclusive prefix sum over the lanes
    for (int d = 1; d < kRoadWave; d <<= 1) {
        const int up = __shfl_up(sum, d);
        if (lane >= d) sum += up;
    }
    w.raw[lane] = raw;
    w.count[lane] = cnt;
    w.first[lane + 1] = sum;
    if (lane == 0) w.first[0] = 0;
    const int total = __shfl(sum, kRoadWave - 1);
    if (lane == 0) w.total = all_ok && total <= kPlanviewMaxRaw ? total : -1;
}

// The walk over the raw points of a planned road, 64 per pass: keep[k] = k == 0 or |raw[k] - raw[k-1]| > 0.02 (load_road :802:
// against the previous RAW point), the previous point of lane 0 carried over from lane 63 of the pass before, across geometry
// seams too.  emit(q, point) runs in the lane of kept point q >= 1, in order of q from pass to pass; kept point 0 is raw
// point 0 and comes back in `head` (a road of fewer than two kept points has no line, so nothing may be written before the second
// one exists), the last kept point in `tail`.  Returns the number of kept points.  All 64 lanes call.
struct RoadPoint {
    double x, y, s, kappa;
};
template <class Emit>
T2D_DEV int road_walk(const RoadWork& w, int rule, int lane, RoadPoint& head, RoadPoint& tail, Emit emit) {
    const int total = w.total;
    int kept = 0, g0 = 0;
    double carry_x = 0.0, carry_y = 0.0;
    head = tail = RoadPoint{0.0, 0.0, 0.0, 0.0};
    for (int base = 0; base < total; base += kRoadWave) {
        while (base >= w.first[g0 + 1]) ++g0;      // (wave-uniform: the geometry of the pass's first point)
        const int k = base + lane;
        const bool active = k < total;
        RoadPoint p{0.0, 0.0, 0.0, 0.0};
        if (active) {
            int g = g0;
            while (k >= w.first[g + 1]) ++g;
            const PlanviewRecord& r = w.rec[g];
            const int n = w.count[g], j = k - w.first[g];
            geom_point(r, w.raw[g], j, rule, p.x, p.y, p.kappa);   // (a popped point changes the count of s only, not the abscissae)
            p.s = linspace_at(r.s, r.s + r.length, n, j);
        }
        double px = __shfl_up(p.x, 1), py = __shfl_up(p.y, 1);
        if (lane == 0) {
            px = carry_x;
            py = carry_y;
        }
        const double dx = p.x - px, dy = p.y - py;
        const bool keep = active && (k == 0 || __builtin_sqrt(dx * dx + dy * dy) > 0.02);
        const unsigned long long mask = __ballot(keep);
        const int q = kept + __popcll(mask & ((1ull << lane) - 1ull));
        if (keep && q > 0) emit(q, p);
        if (base == 0) head = RoadPoint{__shfl(p.x, 0), __shfl(p.y, 0), __shfl(p.s, 0), __shfl(p.kappa, 0)};
        if (mask) {
            const int top = 63 - __clzll((long long)mask);
            tail = RoadPoint{__shfl(p.x, top), __shfl(p.y, top), __shfl(p.s, top), __shfl(p.kappa, top)};
        }
        carry_x = __shfl(p.x, kRoadWave - 1);
        carry_y = __shfl(p.y, kRoadWave - 1);
        kept += __popcll(mask);
    }
    return kept;
}
#endif   // __HIPCC__

}  // namespace t2d
