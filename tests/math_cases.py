"""Input arrays for the math primitives of tactics2d_amd/csrc/t2d_math.h (= oracle t2do_*), shared by tests/test_math_oracle.py
(the C restatement against mpmath, no GPU) and tests/test_gpu_math.py (the device code against the restatement, bit for bit).

Every array is seeded and deterministic.  A family is a dict  case name -> fp64 array  (two-argument functions: a pair of
arrays); the names say which edge a case is there for, and a failing assertion reports the name.
"""
import numpy as np

TWO_PI = 2.0 * np.pi
N_UNIFORM = 4000


def neighbours(v):
    """every value with its one-ulp neighbour on either side"""
    v = np.atleast_1d(np.asarray(v, np.float64)).reshape(-1)
    return np.concatenate([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def _pm(v):
    v = np.atleast_1d(np.asarray(v, np.float64)).reshape(-1)
    return np.concatenate([v, -v])


def sincos_cases():
    rng = np.random.default_rng(20240501)
    c = {}
    for name, lim in (("uniform_8", 8.0), ("uniform_2000", 2000.0), ("uniform_1e5", 1e5), ("uniform_1e9", 1e9)):
        c[name] = rng.uniform(-lim, lim, N_UNIFORM)
    h32 = np.float32(rng.uniform(0.0, TWO_PI, 2000))
    c["fp32_headings"] = np.concatenate([h32, [np.float32(TWO_PI), np.float32(0.0), np.float32(np.pi)]]).astype(np.float64)
    k = np.arange(-64, 65, dtype=np.float64)
    c["half_pi_multiples"] = neighbours(k * (np.pi / 2))
    c["half_pi_60000"] = np.arange(60000, 64001, dtype=np.float64) * (np.pi / 2)
    c["quarter_pi_and_switch"] = neighbours(_pm([np.pi / 4, 0.78]))
    c["zeros_and_subnormal"] = np.array([0.0, -0.0, 5e-324, -5e-324, 1e-310])
    c["at_1e18"] = np.array([1e18, -1e18])
    c["non_finite"] = np.array([np.inf, -np.inf, np.nan])
    return c


# the largest |x| the header's "<= 1 ulp against libm" speaks of, and the largest |x| of the step kernel's own domain
SINCOS_CLAIM_LIMIT = 1e5
SINCOS_REDUCTION_LIMIT = 1e9


def small_angle_cases():
    """|x| <= pi/4: where the reduction's quotient is 0 and sincos_det_small promises sincos_det's bits; 0.78, the bound the
    steer variants test, lies just inside"""
    rng = np.random.default_rng(20240502)
    edge = neighbours(_pm([0.78, 0.5, 1e-3]))
    top = _pm([np.pi / 4, np.nextafter(np.pi / 4, 0.0)])
    return {"uniform_quarter_pi": rng.uniform(-np.pi / 4, np.pi / 4, N_UNIFORM),
            "log_spread": _pm(10.0 ** rng.uniform(-300, np.log10(0.78), 1000)),
            "edges": np.concatenate([edge, top, [0.0, -0.0, 5e-324, -5e-324]])}


def dense_cases(fn):
    """2^20 points for the table-against-literal comparison alone (both sides on the device, no reference to compute): one ulp
    in a low-order coefficient moves the last bit of a result once in ten thousand arguments or fewer, and a few thousand
    points do not see it"""
    rng = np.random.default_rng(20240510)
    n = 1 << 20
    if fn == "atan":
        return rng.uniform(-3.0, 3.0, n)
    x = rng.uniform(-8.0, 8.0, n)
    x[: n // 4] = rng.uniform(-np.pi / 4, np.pi / 4, n // 4)      # (whole waves of small angles: the steer shortcut)
    return x


def atan_cases():
    rng = np.random.default_rng(20240503)
    u = rng.uniform(-9.0, 17.0, 2000)
    return {"uniform_3": rng.uniform(-3.0, 3.0, N_UNIFORM),
            "cauchy": rng.standard_cauchy(N_UNIFORM),
            "powers_of_ten": _pm(10.0 ** u),
            "breakpoints": neighbours(_pm([0.4375, 0.6875, 1.1875, 2.4375])),
            "cutoffs": neighbours(_pm([7.45e-9, 7.450580596923828e-09, 1.8e16, 1.8014398509481984e16])),
            "zeros_and_subnormal": np.array([0.0, -0.0, 5e-324, -5e-324]),
            "non_finite": np.array([np.inf, -np.inf, np.nan])}


def atan2_cases():
    """name -> (y, x)"""
    rng = np.random.default_rng(20240504)
    n = N_UNIFORM
    sy, sx = rng.choice([-1.0, 1.0], n), rng.choice([-1.0, 1.0], n)
    c = {"unit_scale": (rng.uniform(-2.0, 2.0, n), rng.uniform(-2.0, 2.0, n)),
         "scales_1e300": (sy * 10.0 ** rng.uniform(-300, 300, n), sx * 10.0 ** rng.uniform(-300, 300, n)),
         "same_scale": (sy * 10.0 ** rng.uniform(-300, 300, n), None)}
    c["same_scale"] = (c["same_scale"][0], sx * np.abs(c["same_scale"][0]) * rng.uniform(0.1, 10.0, n))
    v = np.array([0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan])
    yy, xx = np.meshgrid(v, v, indexing="ij")
    c["specials"] = (yy.reshape(-1).copy(), xx.reshape(-1).copy())
    return c


def mod_two_pi_cases():
    rng = np.random.default_rng(20240505)
    k = np.concatenate([np.arange(-200, 201, dtype=np.float64), [1e6, 1e8, -1e8, 159154943.0]])
    return {"uniform_50": rng.uniform(-50.0, 50.0, N_UNIFORM),
            "uniform_1e5": rng.uniform(-1e5, 1e5, N_UNIFORM),
            "uniform_1e9": rng.uniform(-1e9, 1e9, N_UNIFORM),
            "fp32_20": np.float32(rng.uniform(-20.0, 20.0, N_UNIFORM)).astype(np.float64),
            "two_pi_multiples": neighbours(k * TWO_PI),
            "tiny": np.array([-1e-20, 1e-20, 5e-324, -5e-324, 0.0, -0.0, -1e-17]),
            "switch_1e9": np.concatenate([neighbours(_pm([1e9])), _pm([999999999.5, 1000000000.5, 1.5e9]),
                                          rng.uniform(0.999e9, 1.001e9, 500), -rng.uniform(0.999e9, 1.001e9, 500)]),
            # the largest multiples of fl(2 pi) below / above the switch, exact in fp64 or not: zero results on both paths
            "zero_results": np.concatenate([_pm(np.array([1.0, 2.0, 4.0, 1024.0, 2.0 ** 27, 2.0 ** 29]) * TWO_PI),
                                            _pm(np.array([2.0 ** 28, 2.0 ** 30, 2.0 ** 40, 2.0 ** 200]) * TWO_PI)]),
            "huge": _pm([1e12, 1e300, 1.7e308]),
            "non_finite": np.array([np.inf, -np.inf, np.nan])}


EXP_OVERFLOW = 709.782712893384
EXP_UNDERFLOW = -745.1332191019411


def exp_cases():
    rng = np.random.default_rng(20240506)
    return {"uniform_full": rng.uniform(-745.2, 709.8, N_UNIFORM),
            "uniform_1": rng.uniform(-1.0, 1.0, N_UNIFORM),
            "uniform_1e-8": rng.uniform(-1e-8, 1e-8, 1000),
            "cutoffs": np.concatenate([neighbours([EXP_OVERFLOW, EXP_UNDERFLOW]), [709.0, 710.0, -745.0, -746.0, 1e4, -1e4]]),
            "subnormal_results": np.concatenate([np.linspace(-745.13, -708.4, 3000), rng.uniform(-745.13, -708.4, 1000)]),
            "zeros_and_subnormal": np.array([0.0, -0.0, 5e-324, -5e-324]),
            "non_finite": np.array([np.inf, -np.inf, np.nan])}


def log_cases():
    """x > 0, finite: log_det's contract"""
    rng = np.random.default_rng(20240507)
    tiny = 2.2250738585072014e-308
    return {"powers_of_ten": 10.0 ** rng.uniform(-300.0, 300.0, N_UNIFORM),
            "uniform_half_2": rng.uniform(0.5, 2.0, N_UNIFORM),
            "near_one": np.concatenate([1.0 + rng.uniform(-1e-6, 1e-6, 1000), neighbours([1.0])]),
            "sqrt_half": neighbours([np.sqrt(0.5), 0.70710678118654752440, 2.0 * 0.70710678118654752440, 0.5, 2.0]),
            "smallest_normal": neighbours([tiny]),
            "subnormals": np.concatenate([5e-324 * 2.0 ** np.arange(0, 52), rng.uniform(5e-324, tiny, 500), [5e-324, 1e-323]]),
            "largest": np.array([1.7976931348623157e308, 1e308])}


POW_CHAIN_EXPONENTS = np.array([1, 2, 3, 4, 5, 6, 7, 8, 16, 33, 64], dtype=np.float64)


def pow_cases():
    """name -> (x, y)"""
    rng = np.random.default_rng(20240508)
    n = N_UNIFORM
    c = {"non_integer": (rng.uniform(0.0, 3.0, n), rng.uniform(0.5, 8.5, n))}
    ys = np.concatenate([POW_CHAIN_EXPONENTS, -POW_CHAIN_EXPONENTS])
    y = np.repeat(ys, 100)
    c["integer_chain"] = (rng.uniform(0.0, 3.0, y.size), y)
    c["integer_chain_negative_base"] = (-rng.uniform(0.0, 3.0, y.size), y)
    c["first_past_the_chain"] = (rng.uniform(0.05, 3.0, 400), np.repeat([65.0, -65.0, 64.5, 100.0], 100))
    c["negative_base_non_integer"] = (-rng.uniform(0.0, 3.0, 200), rng.uniform(0.5, 8.5, 200))
    c["negative_base_past_the_chain"] = (-rng.uniform(0.1, 3.0, 100), np.repeat([65.0, -65.0], 50))
    zy = np.array([0.5, 2.5, 3.0, 64.0, 65.0, -0.5, -2.5, -3.0, -64.0, -65.0])
    c["zero_base"] = (np.concatenate([np.zeros(zy.size), -np.zeros(zy.size)]), np.concatenate([zy, zy]))
    c["zero_exponent"] = (np.array([np.nan, 0.0, -0.0, 2.0, -2.0, np.inf, -np.inf, np.nan]),
                          np.array([0.0, 0.0, 0.0, 0.0, -0.0, 0.0, -0.0, -0.0]))
    c["nan"] = (np.array([np.nan, 2.0, np.nan, np.nan, -1.0, 0.0]), np.array([2.0, np.nan, np.nan, 2.5, np.nan, np.nan]))
    c["one"] = (np.concatenate([np.ones(5), rng.uniform(0.0, 3.0, 5)]), np.concatenate([[0.5, 2.5, 64.0, 65.0, -7.25], np.ones(5)]))
    return c


def steering_set():
    """(e) of tests/test_gpu_math.py: 4 096 steering angles with |x| <= 0.78 -- both ends of the range and their inner
    neighbours, zeros and a subnormal among them -- and the angles a wave's other lanes hold when it is NOT all-small."""
    rng = np.random.default_rng(20240509)
    fixed = np.concatenate([_pm([0.78, np.nextafter(0.78, 0.0), 0.7, 0.5]), [0.0, -0.0, 5e-324, 1e-9]])
    small = np.concatenate([fixed, rng.uniform(-0.78, 0.78, 4096 - fixed.size)])
    rng.shuffle(small)
    large_fixed = np.concatenate([_pm([np.nextafter(0.78, 1.0), np.pi / 4, 0.79, 1.0, np.pi / 2, 2.5, 1e5, 1e9]), [np.nan, np.inf, -np.inf]])
    return small, large_fixed


def large_angles(n, seed):
    """n angles with |x| > 0.78 (or not a number): the fixed ones of steering_set() first, then random ones"""
    rng = np.random.default_rng(seed)
    _, fixed = steering_set()
    r = rng.choice([-1.0, 1.0], n) * rng.uniform(0.7800001, 50.0, n)
    r[:min(n, fixed.size)] = fixed[:min(n, fixed.size)]
    rng.shuffle(r)
    return r


def place_in_waves(small, small_lanes_of_wave, seed):
    """Lay `small` out over waves of 64 lanes: wave w keeps its small angles in the lanes small_lanes_of_wave(w) (a sorted index
    array) and holds large ones everywhere else; the last wave ends with its last small angle.  Returns (array, index of
    every element of `small` in it)."""
    idx, w, at = [], 0, 0
    while at < small.size:
        lanes = np.asarray(small_lanes_of_wave(w))[: small.size - at]
        idx.append(64 * w + lanes)
        at += lanes.size
        w += 1
    idx = np.concatenate(idx)
    n = int(idx[-1]) + 1
    arr = large_angles(n, seed)
    arr[idx] = small
    return arr, idx
