// t2d_spline_dev.h -- Bezier, B-spline and cubic spline curves (interpolator/cpp_interpolator/src/bezier.cpp, b_spline.cpp,
// cubic_spline.cpp behind interpolator/bezier.py, b_spline.py, cubic_spline.py) as device functions.  fp64 throughout, one
// rounding per operation (+ - * / and comparisons only), every sum in the reference's order; tests/spline_ref.py states the same
// operations in Python floats.  DESIGN.md 4.19.
//
// A curve is worked on by one wave.  spline_load: its lanes bring the control points (and knots) into the wave's SplineWork in
// LDS; spline_setup: ONE lane checks the row and does the serial part -- the binomials, the knot interval, the tridiagonal or
// banded solve and the coefficient rows; spline_point: any lane computes any point from that.
#pragma once
#include "t2d_math.h"

namespace t2d {

enum { SPLINE_BEZIER = 0, SPLINE_BSPLINE = 1, SPLINE_CUBIC = 2 };
enum { SPLINE_NATURAL = 1, SPLINE_CLAMPED = 2, SPLINE_NOT_A_KNOT = 3 };
constexpr int kSplineMaxCtrl = 32, kSplineMaxDegree = 5, kSplineMaxKnots = kSplineMaxCtrl + kSplineMaxDegree + 1;
constexpr int kSplineMaxEq = kSplineMaxCtrl + 1;   // row stride of the not-a-knot matrix (odd: rows start on different banks)

// The arguments of one launch (t2d_spline_curves / t2d_spline_routes), checked by spline_args_error.
struct SplineArgs {
    const double2* ctrl;      // [n][max_ctrl]
    const int32_t* n_ctrl;    // [n]
    const double* knots;      // [n][max_ctrl + degree + 1] or null: np.linspace(0, 1, n_ctrl + degree + 1)
    const double* derivs;     // [n][2] or null: 0, 0
    int max_ctrl, n_interp, degree, boundary;
};

template <int KIND> struct SplineWork;
template <> struct SplineWork<SPLINE_BEZIER> {
    double px[kSplineMaxCtrl], py[kSplineMaxCtrl], binom[kSplineMaxCtrl];
    long long total;
    int n;
};
template <> struct SplineWork<SPLINE_BSPLINE> {
    double px[kSplineMaxCtrl], py[kSplineMaxCtrl], knots[kSplineMaxKnots], u_start, delta_u;
    long long total;
    int n;
};
template <> struct SplineWork<SPLINE_CUBIC> {
    // The solve's scratch is dead once m is known, and 10 KB per curve let four workgroups share a CU's LDS (11.3 KB: three):
    // m overwrites rhs (either solver reads rhs[i] for the last time before it writes m[i]); rows 0 and 1 of A are
    // ThomasSolve's c_prime / d_prime; rows 2 .. 4 take the coefficient rows b, c, d afterwards.  a[i] is py[i].
    double px[kSplineMaxCtrl], py[kSplineMaxCtrl], h[kSplineMaxCtrl], slope[kSplineMaxCtrl], rhs[kSplineMaxEq];
    double A[kSplineMaxEq][kSplineMaxEq];   // BandedSolve's full matrix
    long long total;
    int n;
};
enum { SPLINE_ROW_B = 2, SPLINE_ROW_C = 3, SPLINE_ROW_D = 4 };   // rows of A that hold b, c, d after the solve

#ifdef __HIPCC__
T2D_DEV int spline_min_ctrl(int kind, int degree) { return kind == SPLINE_BEZIER ? 2 : kind == SPLINE_CUBIC ? 3 : degree + 1; }

// Lane `lane` of the curve's wave: control point `lane`, knot `lane`, and the zeros of the not-a-knot matrix.  w.n = the row's
// n_ctrl, or 0 where it is out of range (nothing else is read then).
template <int KIND> T2D_DEV void spline_load(SplineWork<KIND>& w, const SplineArgs& a, int e, int lane) {
    int n = a.n_ctrl[e];
    if (n < spline_min_ctrl(KIND, a.degree) || n > a.max_ctrl) n = 0;
    if (lane == 0) w.n = n;
    if (lane < n) {
        const double2 p = a.ctrl[(size_t)e * a.max_ctrl + lane];
        w.px[lane] = p.x;
        w.py[lane] = p.y;
    }
    if constexpr (KIND == SPLINE_BSPLINE) {
        const int nk = n + a.degree + 1;   // <= kSplineMaxKnots < 64
        if (n > 0 && lane < nk) {
            double k;
            if (a.knots) {
                k = a.knots[(size_t)e * (a.max_ctrl + a.degree + 1) + lane];
            } else {   // numpy's linspace: arange(num) * (1 / (num - 1)) + 0, the last one the stop itself
                const double step = 1.0 / (double)(nk - 1);
                k = lane == nk - 1 ? 1.0 : (double)lane * step;
            }
            w.knots[lane] = k;
        }
    }
    if constexpr (KIND == SPLINE_CUBIC) {
        if (a.boundary == SPLINE_NOT_A_KNOT)
            for (int i = lane; i < n * kSplineMaxEq; i += 64) (&w.A[0][0])[i] = 0.0;
    }
}

// ---- the serial part, one lane per curve -----------------------------------------------------------------------------------
T2D_DEV bool spline_points_finite(const double* px, const double* py, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i) ok = ok && __builtin_isfinite(px[i]) && __builtin_isfinite(py[i]);
    return ok;
}

T2D_DEV void spline_setup(SplineWork<SPLINE_BEZIER>& w, const SplineArgs& a, int e) {
    const int N = w.n;
    w.total = 0;
    if (N == 0 || !spline_points_finite(w.px, w.py, N)) return;
    double b = 1.0;
    w.binom[0] = b;
    for (int k = 1; k < N; ++k) {   // bezier.cpp:31
        b = b * (double)(N - k) / (double)k;
        w.binom[k] = b;
    }
    w.total = a.n_interp;
}

T2D_DEV void spline_setup(SplineWork<SPLINE_BSPLINE>& w, const SplineArgs& a, int e) {
    const int n = w.n, nk = n + a.degree + 1;
    w.total = 0;
    if (n == 0 || !spline_points_finite(w.px, w.py, n)) return;
    bool ok = __builtin_isfinite(w.knots[0]);
    for (int i = 1; i < nk; ++i) ok = ok && __builtin_isfinite(w.knots[i]) && !(w.knots[i] < w.knots[i - 1]);   // b_spline.cpp:101-105
    if (!ok) return;
    w.u_start = w.knots[a.degree];
    w.delta_u = (w.knots[n] - w.u_start) / (double)a.n_interp;   // :114-116
    w.total = a.n_interp;
}

// CubicSpline::ThomasSolve (:170-235) for Natural and Clamped; m is left in w.rhs
T2D_DEV void spline_thomas(SplineWork<SPLINE_CUBIC>& w, int n, int boundary) {
    const double* h = w.h;
    double* cp = w.A[0];
    double* dp = w.A[1];
    const bool natural = boundary == SPLINE_NATURAL;
    {
        const double b0 = natural ? 1.0 : 2.0 * h[0], c0 = natural ? 0.0 : h[0];
        cp[0] = c0 / b0;
        dp[0] = w.rhs[0] / b0;
    }
    for (int i = 1; i <= n; ++i) {
        double ai, bi, ci;
        if (i < n) {
            ai = h[i - 1];
            bi = 2.0 * (h[i - 1] + h[i]);
            ci = h[i];
        } else {
            ai = natural ? 0.0 : h[n - 1];
            bi = natural ? 1.0 : 2.0 * h[n - 1];
            ci = 0.0;
        }
        const double denom = bi - ai * cp[i - 1];
        cp[i] = ci / denom;
        dp[i] = (w.rhs[i] - ai * dp[i - 1]) / denom;
    }
    double* m = w.rhs;
    m[n] = dp[n];
    for (int i = n - 1; i >= 0; --i) m[i] = dp[i] - cp[i] * m[i + 1];
}

// CubicSpline::BandedSolve (:238-327) for NotAKnot, as written: the pivot is sought in at most two rows below with a strict >,
// whole rows are swapped, the pivot row is normalised and the rows below are reduced over columns i .. i + 2 ONLY, and back
// substitution reads two columns.  An exactly zero pivot column (three control points) gives m = 0.  w.A arrives zeroed; m is
// left in w.rhs.
T2D_DEV void spline_banded(SplineWork<SPLINE_CUBIC>& w, int n) {
    const double* h = w.h;
    const int N = n + 1;
    for (int i = 1; i < n; ++i) {
        w.A[i][i - 1] = h[i - 1];
        w.A[i][i] = 2.0 * (h[i - 1] + h[i]);
        w.A[i][i + 1] = h[i];
    }
    w.A[0][0] = -h[1];
    w.A[0][1] = h[0] + h[1];
    w.A[0][2] = -h[0];
    w.A[n][n] = -h[n - 2];
    w.A[n][n - 1] = h[n - 2] + h[n - 1];
    w.A[n][n - 2] = -h[n - 1];
    for (int i = 0; i < N; ++i) {
        const int hi = N < i + 3 ? N : i + 3;
        int piv = i;
        double big = __builtin_fabs(w.A[i][i]);
        for (int j = i + 1; j < hi; ++j) {
            const double v = __builtin_fabs(w.A[j][i]);
            if (v > big) {
                big = v;
                piv = j;
            }
        }
        if (piv != i) {
            for (int k = 0; k < N; ++k) {
                const double t = w.A[i][k];
                w.A[i][k] = w.A[piv][k];
                w.A[piv][k] = t;
            }
            const double t = w.rhs[i];
            w.rhs[i] = w.rhs[piv];
            w.rhs[piv] = t;
        }
        if (big == 0.0 || __builtin_fabs(w.A[i][i]) < 1e-12 * big) {
            for (int k = 0; k < N; ++k) w.rhs[k] = 0.0;   // (m)
            return;
        }
        const double pivot = w.A[i][i];
        for (int j = i; j < hi; ++j) w.A[i][j] = w.A[i][j] / pivot;
        w.rhs[i] = w.rhs[i] / pivot;
        for (int j = i + 1; j < hi; ++j) {
            const double f = w.A[j][i];
            if (__builtin_fabs(f) > 1e-12) {
                for (int k = i; k < hi; ++k) w.A[j][k] = w.A[j][k] - f * w.A[i][k];
                w.rhs[j] = w.rhs[j] - f * w.rhs[i];
                w.A[j][i] = 0.0;
            }
        }
    }
    for (int i = N - 1; i >= 0; --i) {
        const int hi = N < i + 3 ? N : i + 3;
        double x = w.rhs[i];
        for (int j = i + 1; j < hi; ++j) x = x - w.A[i][j] * w.rhs[j];   // (rhs[j > i] already holds m[j])
        w.rhs[i] = x;
    }
}

T2D_DEV void spline_setup(SplineWork<SPLINE_CUBIC>& w, const SplineArgs& a, int e) {
    const int N = w.n, n = N - 1;
    w.total = 0;
    if (N == 0 || !spline_points_finite(w.px, w.py, N)) return;
    double d0 = 0.0, d1 = 0.0;
    if (a.boundary == SPLINE_CLAMPED && a.derivs) {
        d0 = a.derivs[2 * (size_t)e];
        d1 = a.derivs[2 * (size_t)e + 1];
        if (!__builtin_isfinite(d0) || !__builtin_isfinite(d1)) return;
    }
    bool ok = true;
    for (int i = 1; i < N; ++i) ok = ok && w.px[i] > w.px[i - 1];   // cubic_spline.cpp:72-76
    if (!ok) return;
    for (int i = 0; i < n; ++i) {   // get_parameters :20-36
        w.h[i] = w.px[i + 1] - w.px[i];
        w.slope[i] = (w.py[i + 1] - w.py[i]) / w.h[i];
    }
    w.rhs[0] = w.rhs[n] = 0.0;
    for (int i = 1; i < n; ++i) w.rhs[i] = 6.0 * (w.slope[i] - w.slope[i - 1]);
    if (a.boundary == SPLINE_CLAMPED) {
        w.rhs[0] = 6.0 * (w.slope[0] - d0);
        w.rhs[n] = 6.0 * (d1 - w.slope[n - 1]);
    }
    if (a.boundary == SPLINE_NOT_A_KNOT) spline_banded(w, n);
    else spline_thomas(w, n, a.boundary);
    for (int i = 0; i < n; ++i) {   // :43-49; a[i] = y[i] stays where it is
        const double mi = w.rhs[i], mj = w.rhs[i + 1], hi = w.h[i];
        w.A[SPLINE_ROW_C][i] = mi / 2.0;
        w.A[SPLINE_ROW_D][i] = (mj - mi) / (6.0 * hi);
        w.A[SPLINE_ROW_B][i] = w.slope[i] - (hi * (2.0 * mi + mj)) / 6.0;
    }
    w.total = (long long)n * a.n_interp + 1;
}

// ---- point k of the curve (0 <= k < total), any lane -----------------------------------------------------------------------
// bezier.cpp:41-61.  The powers are the reference's running products; (1 - t)^(N-1-k) is rebuilt for every k -- at most 31
// multiplications, the same ones in the same order -- instead of kept in a per-lane array.
T2D_DEV void spline_point(const SplineWork<SPLINE_BEZIER>& w, const SplineArgs& a, long long k, double& x, double& y) {
    const int N = w.n;
    const double delta_t = 1.0 / (double)(a.n_interp - 1);
    const double t = (double)k * delta_t, omt = 1.0 - t;
    double pt = 1.0;
    x = y = 0.0;
    for (int c = 0; c < N; ++c) {
        if (c > 0) pt = pt * t;
        double pomt = 1.0;
        for (int j = 1; j < N - c; ++j) pomt = pomt * omt;
        const double temp = (w.binom[c] * pomt) * pt;
        x = x + temp * w.px[c];
        y = y + temp * w.py[c];
    }
}

// BSpline::basis_function (b_spline.cpp:31-68): column p of the triangular table overwrites column p - 1 from the top, which
// reads entries j and j + 1 of the old column before either is replaced.  The loops are unrolled over the cap so that the column
// stays in registers; `degree` is the same in every lane.
T2D_DEV double spline_basis(const double* knots, int nk, int degree, int i, double u) {
    double col[kSplineMaxDegree + 1];
#pragma unroll
    for (int j = 0; j <= kSplineMaxDegree; ++j) {
        const int idx = i + j;
        col[j] = (j <= degree && idx < nk - 1 && knots[idx] <= u && u < knots[idx + 1]) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int p = 1; p <= kSplineMaxDegree; ++p) {
        if (p > degree) break;
#pragma unroll
        for (int j = 0; j <= kSplineMaxDegree - p; ++j) {
            if (j > degree - p) break;
            const int l = i + j, r = l + 1;
            const double dl = knots[l + p] - knots[l], dr = knots[r + p] - knots[r];
            const double left = dl != 0.0 ? ((u - knots[l]) / dl) * col[j] : 0.0;
            const double right = dr != 0.0 ? ((knots[r + p] - u) / dr) * col[j + 1] : 0.0;
            col[j] = left + right;
        }
    }
    return col[0];
}

// b_spline.cpp:121-132: the sum runs over ALL control points, in order
T2D_DEV void spline_point(const SplineWork<SPLINE_BSPLINE>& w, const SplineArgs& a, long long k, double& x, double& y) {
    const int n = w.n, nk = n + a.degree + 1;
    const double u = w.u_start + (double)k * w.delta_u;
    x = y = 0.0;
    for (int i = 0; i < n; ++i) {
        const double basis = spline_basis(w.knots, nk, a.degree, i, u);
        x = x + basis * w.px[i];
        y = y + basis * w.py[i];
    }
}

// cubic_spline.cpp:84-99: sample j of segment i is x_i after j ADDITIONS of the step (not x_i + j * step), so the last sample of
// a segment only approximates the next knot and the next segment starts on the knot itself; the last point is the last control
// point.  The lane redoes the j additions.
T2D_DEV void spline_point(const SplineWork<SPLINE_CUBIC>& w, const SplineArgs& a, long long k, double& x, double& y) {
    if (k == w.total - 1) {
        x = w.px[w.n - 1];
        y = w.py[w.n - 1];
        return;
    }
    // (any other k is an index into the caller's int32-sized output: a 32-bit division)
    const int i = (int)k / a.n_interp, j = (int)k - i * a.n_interp;
    const double x0 = w.px[i];
    const double step = (w.px[i + 1] - x0) / (double)(a.n_interp - 1);
    double xi = x0;
    for (int q = 0; q < j; ++q) xi = xi + step;
    const double xd = xi - x0, xd2 = xd * xd;
    x = xi;
    y = ((w.py[i] + w.A[SPLINE_ROW_B][i] * xd) + w.A[SPLINE_ROW_C][i] * xd2) + (w.A[SPLINE_ROW_D][i] * xd2) * xd;
}
#endif   // __HIPCC__

}  // namespace t2d
