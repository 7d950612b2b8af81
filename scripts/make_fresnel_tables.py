#!/usr/bin/env python3
"""The coefficient tables of fresnel_det (tactics2d_amd/csrc/t2d_math.h), computed with mpmath at 45 digits and printed as the
header tactics2d_amd/csrc/t2d_fresnel_tab.h, which is committed as printed:

    python scripts/make_fresnel_tables.py > tactics2d_amd/csrc/t2d_fresnel_tab.h

tests/road_ref.py reads the same header, and tests/test_road.py runs this script and compares its output with the committed file.

The method.  S(x) = int_0^x sin(pi t^2 / 2) dt, C(x) likewise with cos.
  |x| < X[0]:   the Maclaurin series in z = x^4, SERIES_TERMS terms each:
                    S = x^3 sum_n s_n z^n,  s_n = (-1)^n (pi/2)^(2n+1) / ((2n+1)! (4n+3))
                    C = x   sum_n c_n z^n,  c_n = (-1)^n (pi/2)^(2n)   / ((2n)!   (4n+1))
  |x| >= X[0]:  the auxiliary functions f, g with  C = 1/2 + f sin(pi x^2/2) - g cos(pi x^2/2),
                                                    S = 1/2 - f cos(pi x^2/2) - g sin(pi x^2/2),
                written f = F(u) / (pi x), g = G(u) / (pi^2 x^3) in u = 1 / x^4 (F(0) = G(0) = 1), and F, G as one polynomial
                of AUX_TERMS coefficients in (u - MID[i]) per interval X[i] <= x < X[i+1] (the last one reaches u = 0): the
                Chebyshev interpolant of mpmath.chebyfit, in the monomial form it returns, highest power first.
"""
import mpmath as mp

X = ("1.5", "1.62", "1.78", "2.0", "2.35", "3.0", "4.5")
SERIES_TERMS = 18
AUX_TERMS = 13


def aux(x):
    """f(x), g(x) from mpmath's S and C"""
    half = mp.mpf(1) / 2
    S, C = mp.fresnels(x), mp.fresnelc(x)
    a = mp.pi * x * x / 2
    s, c = mp.sin(a), mp.cos(a)
    return (half - S) * c - (half - C) * s, (half - C) * c + (half - S) * s


def F(u):
    if u == 0:
        return mp.mpf(1)
    x = u ** (-mp.mpf(1) / 4)
    return aux(x)[0] * mp.pi * x


def G(u):
    if u == 0:
        return mp.mpf(1)
    x = u ** (-mp.mpf(1) / 4)
    return aux(x)[1] * mp.pi ** 2 * x ** 3


def tables():
    mp.mp.dps = 45
    h = mp.pi / 2
    s_series = [(-1) ** n * h ** (2 * n + 1) / (mp.factorial(2 * n + 1) * (4 * n + 3)) for n in range(SERIES_TERMS)]
    c_series = [(-1) ** n * h ** (2 * n) / (mp.factorial(2 * n) * (4 * n + 1)) for n in range(SERIES_TERMS)]
    edges = [1 / mp.mpf(x) ** 4 for x in X] + [mp.mpf(0)]
    mids, fs, gs, worst = [], [], [], mp.mpf(0)
    for i in range(len(X)):
        mid = mp.mpf(float((edges[i] + edges[i + 1]) / 2))   # (the device subtracts the ROUNDED centre: fit around that)
        lo, hi = edges[i + 1] - mid, edges[i] - mid
        cf, ef = mp.chebyfit(lambda v: F(mid + v), [lo, hi], AUX_TERMS, error=True)
        cg, eg = mp.chebyfit(lambda v: G(mid + v), [lo, hi], AUX_TERMS, error=True)
        x0 = mp.mpf(X[i])
        worst = max(worst, ef / (mp.pi * x0), eg / (mp.pi ** 2 * x0 ** 3))
        mids.append(mid)
        fs.append(cf)
        gs.append(cg)
    return s_series, c_series, mids, fs, gs, worst


def row(values):
    return ", ".join(repr(float(v)) for v in values)


def header():
    s_series, c_series, mids, fs, gs, worst = tables()
    out = ["// t2d_fresnel_tab.h -- the coefficient tables of fresnel_det (t2d_math.h).  GENERATED: the output of",
           "// scripts/make_fresnel_tables.py (mpmath, 45 digits), committed as printed; the method is stated there and in DESIGN.md 4.20.",
           "// Largest error of the interval fits, as an absolute error of f or g: %s." % mp.nstr(worst, 2),
           "#pragma once",
           "#define T2D_FRESNEL_SERIES_TERMS %d" % SERIES_TERMS,
           "#define T2D_FRESNEL_AUX_INTERVALS %d" % len(X),
           "#define T2D_FRESNEL_AUX_TERMS %d" % AUX_TERMS,
           "// interval i of the auxiliary form: T2D_FRESNEL_AUX_X[i] <= |x| (< the next one); below the first the series is used",
           "#define T2D_FRESNEL_AUX_X {%s}" % row(mp.mpf(x) for x in X),
           "// s_n, c_n of the series in z = x^4, n = 0 upward",
           "#define T2D_FRESNEL_S_SERIES {%s}" % row(s_series),
           "#define T2D_FRESNEL_C_SERIES {%s}" % row(c_series),
           "// per interval: the centre in u = 1 / x^4, then F and G as polynomials in (u - centre), highest power first",
           "#define T2D_FRESNEL_AUX_MID {%s}" % row(mids),
           "#define T2D_FRESNEL_AUX_F {%s}" % ", \\\n    ".join("{%s}" % row(r) for r in fs),
           "#define T2D_FRESNEL_AUX_G {%s}" % ", \\\n    ".join("{%s}" % row(r) for r in gs)]
    return "\n".join(out) + "\n"


if __name__ == "__main__":
    print(header(), end="")
