"""The Bezier, B-spline and cubic spline curves of t2d_spline_curves / t2d_spline_routes (include/t2d.h) in plain Python floats,
one IEEE operation per line of arithmetic, in the order the kernels of tactics2d_amd/csrc/t2d_spline_dev.h take them.  What it
restates is interpolator/cpp_interpolator/src/{bezier,b_spline,cubic_spline}.cpp behind interpolator/{bezier,b_spline,
cubic_spline}.py; tests/golden/splines.npz holds what those gave, and tests/test_splines.py asks for bit equality.
DESIGN.md 4.19.

Every function returns a float64 array [count, 2], or None for a row the device answers with count 0 (the BUILD-DEFINED rules
of the header: too few control points, abscissae that do not increase, knots that decrease, an input that is not finite).
"""
import math

import numpy as np

BEZIER, BSPLINE, CUBIC = 0, 1, 2
NATURAL, CLAMPED, NOT_A_KNOT = 1, 2, 3


def _finite(values):
    return all(math.isfinite(float(v)) for v in values)


def default_knots(n_ctrl, degree):
    """np.linspace(0, 1, n_ctrl + degree + 1) as numpy computes it: i * (1 / (num - 1)), the last one exactly 1"""
    num = n_ctrl + degree + 1
    step = 1.0 / float(num - 1)
    k = [float(i) * step for i in range(num)]
    k[num - 1] = 1.0
    return k


def bezier(ctrl, n_interpolation):
    ctrl = np.asarray(ctrl, np.float64)
    N = len(ctrl)
    if N < 2 or not _finite(ctrl.ravel()):
        return None
    px, py = [float(v) for v in ctrl[:, 0]], [float(v) for v in ctrl[:, 1]]
    binom = [1.0] * N
    for k in range(1, N):
        binom[k] = binom[k - 1] * float(N - k) / float(k)
    delta_t = 1.0 / float(n_interpolation - 1)
    out = np.zeros((n_interpolation, 2))
    for i in range(n_interpolation):
        t = float(i) * delta_t
        omt = 1.0 - t
        pt, pomt = [1.0] * N, [1.0] * N
        for j in range(1, N):
            pt[j] = pt[j - 1] * t
            pomt[j] = pomt[j - 1] * omt
        x = y = 0.0
        for k in range(N):
            temp = binom[k] * pomt[N - k - 1] * pt[k]
            x += temp * px[k]
            y += temp * py[k]
        out[i] = x, y
    return out


def basis_function(i, degree, u, knots):
    """BSpline::basis_function: the triangular table, column by column"""
    col = [0.0] * (degree + 1)
    for j in range(degree + 1):
        idx = i + j
        col[j] = 1.0 if idx < len(knots) - 1 and knots[idx] <= u < knots[idx + 1] else 0.0
    for p in range(1, degree + 1):
        for j in range(degree - p + 1):
            l, r = i + j, i + j + 1
            dl, dr = knots[l + p] - knots[l], knots[r + p] - knots[r]
            left = ((u - knots[l]) / dl) * col[j] if dl != 0.0 else 0.0
            right = ((knots[r + p] - u) / dr) * col[j + 1] if dr != 0.0 else 0.0
            col[j] = left + right
    return col[0]


def bspline(ctrl, knots=None, degree=0, n_interpolation=100):
    ctrl = np.asarray(ctrl, np.float64)
    n = len(ctrl)
    if n < degree + 1 or not _finite(ctrl.ravel()):
        return None
    knots = default_knots(n, degree) if knots is None else [float(v) for v in knots]
    assert len(knots) == n + degree + 1
    if not _finite(knots) or any(knots[i] < knots[i - 1] for i in range(1, len(knots))):
        return None
    px, py = [float(v) for v in ctrl[:, 0]], [float(v) for v in ctrl[:, 1]]
    u_start, u_end = knots[degree], knots[n]
    with np.errstate(all="ignore"):
        delta_u = float(np.float64(u_end - u_start) / np.float64(n_interpolation))
    out = np.zeros((n_interpolation, 2))
    for j in range(n_interpolation):
        u = u_start + float(j) * delta_u
        x = y = 0.0
        for i in range(n):
            b = basis_function(i, degree, u, knots)
            x += b * px[i]
            y += b * py[i]
        out[j] = x, y
    return out


def _div(a, b):
    """a / b as the hardware gives it (inf or nan for a zero divisor, where Python raises)"""
    with np.errstate(all="ignore"):
        return float(np.float64(a) / np.float64(b))


def _thomas(h, B, boundary):
    n = len(h)
    N = n + 1
    a, b, c = [0.0] * N, [0.0] * N, [0.0] * N
    if boundary == NATURAL:
        b[0], b[n] = 1.0, 1.0
    else:
        b[0], c[0] = 2.0 * h[0], h[0]
        a[n], b[n] = h[n - 1], 2.0 * h[n - 1]
    for i in range(1, n):
        a[i], b[i], c[i] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
    cp, dp = [0.0] * N, [0.0] * N
    cp[0], dp[0] = _div(c[0], b[0]), _div(B[0], b[0])
    for i in range(1, N):
        denom = b[i] - a[i] * cp[i - 1]
        cp[i] = _div(c[i], denom)
        dp[i] = _div(B[i] - a[i] * dp[i - 1], denom)
    m = [0.0] * N
    m[N - 1] = dp[N - 1]
    for i in range(N - 2, -1, -1):
        m[i] = dp[i] - cp[i] * m[i + 1]
    return m


def _banded(h, B):
    """CubicSpline::BandedSolve: a full matrix, pivots from at most two rows below (strict >), normalisation and elimination over
    columns i .. i + 2 only"""
    n = len(h)
    N = n + 1
    A = [[0.0] * N for _ in range(N)]
    rhs = list(B)
    for i in range(1, n):
        A[i][i - 1], A[i][i], A[i][i + 1] = h[i - 1], 2.0 * (h[i - 1] + h[i]), h[i]
    A[0][0], A[0][1], A[0][2] = -h[1], h[0] + h[1], -h[0]
    A[n][n], A[n][n - 1], A[n][n - 2] = -h[n - 2], h[n - 2] + h[n - 1], -h[n - 1]
    for i in range(N):
        hi = min(N, i + 3)
        piv, big = i, abs(A[i][i])
        for j in range(i + 1, hi):
            if abs(A[j][i]) > big:
                big, piv = abs(A[j][i]), j
        if piv != i:
            A[i], A[piv] = A[piv], A[i]
            rhs[i], rhs[piv] = rhs[piv], rhs[i]
        if big == 0.0 or abs(A[i][i]) < 1e-12 * big:
            return [0.0] * N
        pivot = A[i][i]
        for j in range(i, hi):
            A[i][j] = _div(A[i][j], pivot)
        rhs[i] = _div(rhs[i], pivot)
        for j in range(i + 1, hi):
            f = A[j][i]
            if abs(f) > 1e-12:
                for k in range(i, hi):
                    A[j][k] -= f * A[i][k]
                rhs[j] -= f * rhs[i]
                A[j][i] = 0.0
    x = [0.0] * N
    for i in range(N - 1, -1, -1):
        x[i] = rhs[i]
        for j in range(i + 1, min(N, i + 3)):
            x[i] -= A[i][j] * x[j]
    return x


def cubic_parameters(ctrl, first_derivatives=(0.0, 0.0), boundary=NOT_A_KNOT):
    """(a, b, c, d, m) of CubicSpline::get_parameters"""
    x, y = [float(v) for v in ctrl[:, 0]], [float(v) for v in ctrl[:, 1]]
    n = len(x) - 1
    h = [x[i + 1] - x[i] for i in range(n)]
    slope = [_div(y[i + 1] - y[i], h[i]) for i in range(n)]
    B = [0.0] * (n + 1)
    for i in range(1, n):
        B[i] = 6.0 * (slope[i] - slope[i - 1])
    if boundary == CLAMPED:
        B[0] = 6.0 * (slope[0] - float(first_derivatives[0]))
        B[n] = 6.0 * (float(first_derivatives[1]) - slope[n - 1])
    m = _banded(h, B) if boundary == NOT_A_KNOT else _thomas(h, B, boundary)
    a, b, c, d = [0.0] * n, [0.0] * n, [0.0] * n, [0.0] * n
    for i in range(n):
        a[i] = y[i]
        c[i] = m[i] / 2.0
        d[i] = _div(m[i + 1] - m[i], 6.0 * h[i])
        b[i] = slope[i] - h[i] * (2.0 * m[i] + m[i + 1]) / 6.0
    return a, b, c, d, m


def cubic(ctrl, first_derivatives=(0.0, 0.0), n_interpolation=100, boundary=NOT_A_KNOT):
    ctrl = np.asarray(ctrl, np.float64)
    n_pts = len(ctrl)
    if n_pts < 3 or not _finite(ctrl.ravel()):
        return None
    if boundary == CLAMPED and not _finite(first_derivatives):
        return None
    if any(ctrl[i, 0] <= ctrl[i - 1, 0] for i in range(1, n_pts)):
        return None
    a, b, c, d, _ = cubic_parameters(ctrl, first_derivatives, boundary)
    n = n_pts - 1
    out = np.zeros((n * n_interpolation + 1, 2))
    k = 0
    for i in range(n):
        x0 = float(ctrl[i, 0])
        step = (float(ctrl[i + 1, 0]) - x0) / float(n_interpolation - 1)
        xi = x0
        for _ in range(n_interpolation):
            xd = xi - x0
            xd2 = xd * xd
            out[k] = xi, a[i] + b[i] * xd + c[i] * xd2 + d[i] * xd2 * xd
            k += 1
            xi += step
    out[k] = ctrl[n]
    return out


def curve(kind, ctrl, n_interpolation, degree=0, knots=None, boundary=NOT_A_KNOT, first_derivatives=(0.0, 0.0)):
    """the curve of one row of t2d_spline_curves"""
    if kind == BEZIER:
        return bezier(ctrl, n_interpolation)
    if kind == BSPLINE:
        return bspline(ctrl, knots, degree, n_interpolation)
    return cubic(ctrl, first_derivatives, n_interpolation, boundary)


def route_vertices(points, capacity):
    """what t2d_spline_routes leaves in a route of `capacity` vertices: the points rounded to fp32, the last point repeated"""
    p = np.asarray(points, np.float64).astype(np.float32)
    if len(p) >= capacity:
        return p[:capacity].copy()
    return np.concatenate([p, np.repeat(p[-1:], capacity - len(p), 0)])
