"""The C restatement of the deterministic math primitives (oracle t2do_*: the spec tactics2d_amd/csrc/t2d_math.h computes bit
for bit, tests/test_gpu_math.py) against the exact values: mpmath at 200 bits, exact rationals for mod 2 pi.  No GPU.

Errors are in ulps of the EXACT value (its own binade; the subnormal spacing below 2^-1022).  Every bound is one the project
states -- the header of t2d_math.h, DESIGN.md section 3 -- plus the rounding of the reference it was stated against, never a
figure read off the code under test.  What was measured on these arrays is tabulated in DESIGN.md section 3.
"""
import math
from fractions import Fraction

import mpmath
import numpy as np
import pytest

import math_cases as MC

mpmath.mp.prec = 200
mpf = mpmath.mpf


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def same_bits(a, b):
    """bit patterns equal, NaNs equal to each other"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def ulp_error(got, exact):
    """|got - exact| in ulps of the exact value (an mpf); an exact value that rounds to infinity wants infinity"""
    if exact == 0:
        return 0.0 if got == 0.0 else math.inf
    _, e = mpmath.frexp(exact)                  # |exact| in [2^(e-1), 2^e)
    if e > 1024:
        return 0.0 if (math.isinf(got) and (got > 0) == (exact > 0)) else math.inf
    if math.isinf(got) or math.isnan(got):
        return math.inf
    ulp = mpmath.ldexp(mpf(1), max(int(e) - 1, -1022) - 52)
    return float(abs(mpf(got) - exact) / ulp)


def worst(got, xs, exact_fn):
    """(largest ulp error, the argument it is at) of got[i] against exact_fn(*xs[i])"""
    w, at = 0.0, None
    for i in range(len(got)):
        args = tuple(float(x[i]) for x in xs)
        e = ulp_error(float(got[i]), exact_fn(*(mpf(a) for a in args)))
        if e > w:
            w, at = e, args
    return w, at


def report(name, case, w, at, bound):
    print(f"{name:8s} {case:28s} worst {w:7.3f} ulp at {at}   (bound {bound})")


# ---- sin / cos ---------------------------------------------------------------------------------------------------------------
# |x| <= 1e5: the header's "<= 1 ulp against libm" plus libm's own half ulp.
SINCOS_BOUND = 1.5
# 1e5 < |x| <= 1e9, where the project makes no claim: what the 3-term reduction implies.  k = rint(x 2/pi) < 2^30, so
# x - k PIO2_HI is a multiple of 2^-52 (or finer, for k <= 1) below 1 in magnitude: the first fma is exact.  The second and the
# third round once each, half an ulp of r; what PIO2_LO leaves out of pi/2 is below 2^-160 k < 1e-39, against |r| > 1e-19 for
# every double in range: nothing.  So r is within 1 ulp(r) of x - k pi/2.  sin and cos have condition numbers r / tan r <= 1
# and r tan r < 0.79 on |r| <= pi/4 (+ 2e-7 where the rounded quotient takes the neighbouring k), and sin r < r can lie one
# binade below r, where the same absolute error counts double: 2 ulp from the reduction.  The kernels on top are the classic
# minimax ones, < 1 ulp with their own rounding.  3 ulp in all -- and nothing in the argument depends on |x| beyond k < 2^30.
SINCOS_REDUCTION_BOUND = 3.0


@pytest.fixture(scope="module")
def sincos_results(oracle):
    return {name: (x, oracle.det_math("sincos", x)) for name, x in MC.sincos_cases().items()}


def test_sincos_within_the_claim_up_to_1e5_and_within_the_reduction_bound_up_to_1e9(sincos_results):
    for name, (x, (s, c)) in sincos_results.items():
        fin = np.isfinite(x)
        for lim_lo, lim_hi, bound in ((-1.0, MC.SINCOS_CLAIM_LIMIT, SINCOS_BOUND),
                                      (MC.SINCOS_CLAIM_LIMIT, MC.SINCOS_REDUCTION_LIMIT, SINCOS_REDUCTION_BOUND)):
            m = fin & (np.abs(x) > lim_lo) & (np.abs(x) <= lim_hi)
            if not m.any():
                continue
            ws, at_s = worst(s[m], (x[m],), mpmath.sin)
            wc, at_c = worst(c[m], (x[m],), mpmath.cos)
            report("sin", f"{name} <= {lim_hi:g}", ws, at_s, bound)
            report("cos", f"{name} <= {lim_hi:g}", wc, at_c, bound)
            assert ws <= bound, (name, "sin", ws, at_s)
            assert wc <= bound, (name, "cos", wc, at_c)


def test_sincos_exact_cases(oracle, sincos_results):
    assert oracle.sincos(0.0) == (0.0, 1.0)
    s, c = oracle.det_math("sincos", [0.0, -0.0, 5e-324, -5e-324, 1e-310])
    # Tiny arguments come back as they are, sign included.  NEGATIVE ZERO DOES NOT: the spec's sin(-0.0) is +0.0 where np.sin
    # keeps the sign -- the reduction's fma(-k, PIO2_HI, x) adds (+0)(pi/2) to -0, and the kernel's fma(r z, ps, r) does the same
    # in sincos_det_small.  No comparison in the project tells the two zeros apart (x == y on values; the device computes the
    # same +0, tests/test_gpu_math.py), so the case is pinned here as the spec's behaviour.
    assert same_bits(s, [0.0, 0.0, 5e-324, -5e-324, 1e-310]).all()
    assert same_bits(c, [1.0] * 5).all()
    # inf and nan give nan in both outputs, as np.sin / np.cos do
    x, (s, c) = sincos_results["non_finite"]
    with np.errstate(invalid="ignore"):
        assert np.isnan(s).all() and np.isnan(c).all() and np.isnan(np.sin(x)).all() and np.isnan(np.cos(x)).all()
    # 1e18 is where the bit-identity domain ends, far beyond the accuracy domain: k no longer fits 53 bits, the reduction leaves
    # an |r| of the order of 1e18 and the kernels return values that are no sine or cosine of anything.  Finite, and that is all.
    x, (s, c) = sincos_results["at_1e18"]
    assert np.isfinite(s).all() and np.isfinite(c).all()
    # odd / even
    x = MC.sincos_cases()["uniform_2000"]
    sp, cp = oracle.det_math("sincos", x)
    sn, cn = oracle.det_math("sincos", -x)
    assert same_bits(sn, -sp).all() and same_bits(cn, cp).all()


def test_tan_is_the_quotient_of_the_two(oracle):
    x = np.concatenate([MC.sincos_cases()[k] for k in ("uniform_8", "uniform_2000", "half_pi_multiples", "fp32_headings")])
    s, c = oracle.det_math("sincos", x)
    with np.errstate(divide="ignore", invalid="ignore"):
        assert same_bits(oracle.det_math("tan", x), s / c).all()
    assert same_bits([oracle.det_tan(0.0), oracle.det_tan(-0.0)], [0.0, 0.0]).all()      # (+0 / 1: see sin(-0.0) above)


# ---- atan / atan2 ------------------------------------------------------------------------------------------------------------
ATAN_BOUND = 1.5     # "<= 1 ulp from numpy/libm", plus libm's half ulp
ATAN2_BOUND = 2.0    # the quotient's rounding on top of atan's


def test_atan_within_the_claim(oracle):
    for name, x in MC.atan_cases().items():
        got = oracle.det_math("atan", x)
        fin = np.isfinite(x)
        w, at = worst(got[fin], (x[fin],), mpmath.atan)
        report("atan", name, w, at, ATAN_BOUND)
        assert w <= ATAN_BOUND, (name, w, at)
    got = oracle.det_math("atan", [0.0, -0.0, np.inf, -np.inf, np.nan])
    assert same_bits(got, [0.0, -0.0, np.pi / 2, -np.pi / 2, np.nan]).all()      # as np.arctan


def _atan2_exact(y, x):
    return mpmath.atan2(y, x)


def test_atan2_within_the_claim(oracle):
    cases = MC.atan2_cases()
    for name in ("unit_scale", "scales_1e300", "same_scale"):
        y, x = cases[name]
        got = oracle.det_math("atan2", y, x)
        w, at = worst(got, (y, x), _atan2_exact)
        report("atan2", name, w, at, ATAN2_BOUND)
        assert w <= ATAN2_BOUND, (name, w, at)


def test_atan2_special_values_follow_numpy(oracle):
    """signed zeros, axes, infinities and nan: np.arctan2's values (atan2(+-0, +0) = +-0, atan2(+-0, -0) = +-pi) to within the
    bound.  Both arguments infinite is outside the contract: the spec divides, and returns nan where numpy returns +-pi/4,
    +-3pi/4; the case is pinned so that a change of it is a decision."""
    y, x = MC.atan2_cases()["specials"]
    got = oracle.det_math("atan2", y, x)
    with np.errstate(invalid="ignore"):
        want = np.arctan2(y, x)
    both_inf = np.isinf(y) & np.isinf(x)
    assert np.isnan(got[both_inf]).all()
    for g, w_, yy, xx in zip(got[~both_inf], want[~both_inf], y[~both_inf], x[~both_inf]):
        if np.isnan(w_):
            assert np.isnan(g), (yy, xx)
        elif w_ == 0.0:
            assert g == 0.0 and math.copysign(1.0, g) == math.copysign(1.0, w_), (yy, xx, g)
        else:
            assert abs(g - w_) <= ATAN2_BOUND * np.spacing(abs(w_)), (yy, xx, g, w_)
    assert oracle.det_atan2(0.0, 0.0) == 0.0 and math.copysign(1.0, oracle.det_atan2(-0.0, 0.0)) == -1.0


# ---- mod 2 pi ----------------------------------------------------------------------------------------------------------------
def _exact_mod(phi):
    """np.mod(phi, fl(2 pi)) as numpy defines it, in exact rationals: the remainder of the truncated division, moved up by
    fl(2 pi) when it is negative, rounded once; a zero remainder is +0."""
    b = Fraction(MC.TWO_PI)
    p = Fraction(phi)
    q = abs(p) // b
    m = (abs(p) - q * b) * (1 if p >= 0 else -1)       # fmod: exact, sign of phi
    if m == 0:
        return 0.0
    if m < 0:
        m += b
    return float(m)                                      # int / int division of a Fraction rounds to nearest even


def test_mod_two_pi_is_numpy_mod_bit_for_bit(oracle):
    for name, phi in MC.mod_two_pi_cases().items():
        got = oracle.det_math("mod_two_pi", phi)
        with np.errstate(invalid="ignore"):
            want = np.mod(phi, MC.TWO_PI)
        bad = ~same_bits(got, want)
        assert not bad.any(), (name, phi[bad][:5], got[bad][:5], want[bad][:5])
        fin = np.isfinite(phi)
        exact = np.array([_exact_mod(float(p)) for p in phi[fin]])
        bad = ~same_bits(got[fin], exact)
        assert not bad.any(), (name, "exact rationals", phi[fin][bad][:5], got[fin][bad][:5], exact[bad][:5])
        assert (np.signbit(got[fin]) == 0).all() and (got[fin] <= MC.TWO_PI).all()
    assert oracle.det_mod_two_pi(-1e-20) == MC.TWO_PI            # the reference's np.mod quirk: the result CAN be 2 pi


# ---- exp / log / pow ---------------------------------------------------------------------------------------------------------
def test_exp_below_one_ulp(oracle):
    for name, x in MC.exp_cases().items():
        got = oracle.det_math("exp", x)
        fin = np.isfinite(x)
        w, at = worst(got[fin], (x[fin],), mpmath.exp)
        report("exp", name, w, at, "< 1")
        assert w < 1.0, (name, w, at)
    got = oracle.det_math("exp", [0.0, -0.0, np.inf, -np.inf, np.nan, 710.0, -746.0])
    assert same_bits(got, [1.0, 1.0, np.inf, 0.0, np.nan, np.inf, 0.0]).all()
    # the cut-offs are the last arguments with a finite / a non-zero result
    assert np.isfinite(oracle.det_exp(MC.EXP_OVERFLOW)) and oracle.det_exp(np.nextafter(MC.EXP_OVERFLOW, np.inf)) == np.inf
    assert oracle.det_exp(MC.EXP_UNDERFLOW) == 5e-324 and oracle.det_exp(np.nextafter(MC.EXP_UNDERFLOW, -np.inf)) == 0.0


def test_log_below_one_ulp(oracle):
    for name, x in MC.log_cases().items():
        got = oracle.det_math("log", x)
        w, at = worst(got, (x,), mpmath.log)
        report("log", name, w, at, "< 1")
        assert w < 1.0, (name, w, at)
    assert same_bits(oracle.det_math("log", [1.0]), [0.0]).all()


def test_pow_integer_chain_within_y_ulp(oracle):
    """|y| - 1 roundings of the multiplication chain plus the reciprocal's for y < 0: <= |y| ulp"""
    cases = MC.pow_cases()
    for name in ("integer_chain", "integer_chain_negative_base"):
        x, y = cases[name]
        got = oracle.det_math("pow", x, y)
        for e in np.unique(y):
            m = y == e
            w, at = worst(got[m], (x[m], y[m]), lambda a, b: mpmath.power(a, int(b)))
            report("pow", f"{name} y={e:g}", w, at, abs(e))
            assert w <= abs(e), (name, e, w, at)


def test_pow_non_integer_within_the_amplified_bound(oracle):
    """exp(y log x): log < 1 ulp and the product's rounding, amplified by exp, plus exp's own: <= 3 |y ln x| + 1 ulp"""
    cases = MC.pow_cases()
    worst_ratio, worst_at = 0.0, None
    for name in ("non_integer", "first_past_the_chain"):
        x, y = cases[name]
        got = oracle.det_math("pow", x, y)
        for g, a, b in zip(got, x, y):
            if a == 0.0:
                assert g == 0.0
                continue
            e = ulp_error(float(g), mpmath.power(mpf(float(a)), mpf(float(b))))
            bound = 3.0 * abs(float(b) * math.log(float(a))) + 1.0
            if e / bound > worst_ratio:
                worst_ratio, worst_at = e / bound, (float(a), float(b), e, bound)
            assert e <= bound, (name, float(a), float(b), e, bound)
    print(f"pow      non-integer: the closest to its bound: error / bound = {worst_ratio:.3f} at (x, y, ulp, bound) = {worst_at}")


def test_pow_special_values(oracle):
    cases = MC.pow_cases()
    x, y = cases["negative_base_non_integer"]
    assert np.isnan(oracle.det_math("pow", x[x < 0], y[x < 0])).all()      # Python gives a complex number: outside the contract
    x, y = cases["negative_base_past_the_chain"]
    assert np.isnan(oracle.det_math("pow", x, y)).all()                    # 65 is past the chain: the exp / log path, no sign rule
    x, y = cases["zero_base"]
    got = oracle.det_math("pow", x, y)
    with np.errstate(divide="ignore"):
        want = np.where(y > 0, np.where((np.abs(y) <= 64) & (y % 2 == 1), x, 0.0), np.where((np.abs(y) <= 64) & (y % 2 == 1), 1.0 / x, np.inf))
    assert same_bits(got, want).all(), (got, want)
    x, y = cases["zero_exponent"]
    assert same_bits(oracle.det_math("pow", x, y), np.ones(x.size)).all()  # x ** 0 = 1, nan ** 0 included (float.__pow__)
    x, y = cases["nan"]
    assert np.isnan(oracle.det_math("pow", x, y)).all()
    x, y = cases["one"]
    got = oracle.det_math("pow", x, y)
    assert same_bits(got[:5], np.ones(5)).all() and same_bits(got[5:], x[5:]).all()
    # sign of an odd power of a negative base, and the chain against exact integers
    assert oracle.det_pow(-2.0, 3.0) == -8.0 and oracle.det_pow(-2.0, 64.0) == 2.0 ** 64 and oracle.det_pow(2.0, -3.0) == 0.125
