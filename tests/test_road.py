"""The Fresnel integrals, Spiral and ParamPoly3 curves and plan-view reference lines WITHOUT a device: the specification
(tests/road_ref.py) against mpmath, against the fixture made by running the reference (tests/golden/road.npz), and -- the
build-defined clothoid -- against scipy's quadrature; the fixture's own preconditions; the committed coefficient table against
its generator; header, _ffi and layout against each other; the host-side refusals of the Python classes.

TOL is the project's 1e-9 of tests/test_dubins.py.  It is derived, not guessed: with |gamma| >= 1e-6 the spiral's scale
a = sqrt(pi / |gamma|) is at most 1773, so a Fresnel error of 5e-15 moves a point by under 1e-11 m; every other operation is an
IEEE + - * / sqrt in the reference's order, and sines and cosines agree within an ulp of values below 1e3."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import road_ref as R
from test_dubins import TOL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the Fresnel integrals -------------------------------------------------------------------------------------------------------
def fresnel_grid():
    """The committed, seeded grid: [0, 60] uniformly, densely around the branch points of fresnel_det (every interval edge, a
    few ulp and a few 1e-9 to either side), 0, +-tiny, the old library's saturation point 36974 and the threshold 2^53 from both
    sides.  Non-negative finite values; the sign is tested apart."""
    rng = np.random.default_rng(0)
    edges = np.repeat(R.AUX_X, 9) + np.tile([-1e-3, -1e-9, -4e-16, -2e-16, 0.0, 2e-16, 4e-16, 1e-9, 1e-3], len(R.AUX_X))
    around = np.concatenate([rng.uniform(x - 0.05, x + 0.05, 40) for x in R.AUX_X])
    return np.concatenate([rng.uniform(0.0, 60.0, 1204), edges, around, rng.uniform(0.0, 1.5, 200), rng.uniform(1.5, 5.0, 400),
                           [0.0, 5e-324, 1e-300, 1e-160, 1e-8, 36974.0, np.nextafter(R.SATURATE, 0.0), R.SATURATE, 2.0 * R.SATURATE]])


def mp_fresnel(x):
    import mpmath as mp
    with mp.workdps(40):
        return ([mp.fresnels(mp.mpf(float(v))) for v in x], [mp.fresnelc(mp.mpf(float(v))) for v in x])


def largest_error(values, exact):
    import mpmath as mp
    with mp.workdps(40):
        return max(float(abs(mp.mpf(float(v)) - e)) for v, e in zip(values, exact))


@pytest.fixture(scope="module")
def grid_exact():
    x = fresnel_grid()
    return x, mp_fresnel(x)


def test_the_specifications_fresnel_meets_twice_scipys_error_against_mpmath(grid_exact):
    import scipy.special
    x, (es, ec) = grid_exact
    S, C = R.fresnel(x)
    ss, sc = scipy.special.fresnel(x)
    in60 = x <= 60.0                                    # scipy's yardstick is its error on [0, 60]; ours covers the whole grid
    bound_s = 2.0 * largest_error(ss[in60], [e for e, k in zip(es, in60) if k])
    bound_c = 2.0 * largest_error(sc[in60], [e for e, k in zip(ec, in60) if k])
    err_s, err_c = largest_error(S, es), largest_error(C, ec)
    print(f"fresnel on {len(x)} points: largest error S {err_s:.3e} C {err_c:.3e}; twice scipy's on [0, 60]: S {bound_s:.3e} C {bound_c:.3e}")
    assert err_s <= bound_s and err_c <= bound_c


def test_fresnel_is_odd_saturates_and_propagates_nan():
    x = np.array([0.3, 1.49, 1.5, 2.0, 7.25, 59.0, 1e6, 1e15])
    S, C = R.fresnel(x)
    Sn, Cn = R.fresnel(-x)
    assert np.array_equal(Sn, -S) and np.array_equal(Cn, -C)
    S, C = R.fresnel(np.array([0.0, -0.0, np.inf, -np.inf, 2.0 ** 53, -2.0 ** 60, np.nan]))
    assert S[:6].tolist() == [0.0, -0.0, 0.5, -0.5, 0.5, -0.5] and C[:6].tolist() == S[:6].tolist()
    assert np.signbit(S[1]) and np.signbit(C[1]) and np.isnan(S[6]) and np.isnan(C[6])
    S, C = R.fresnel(np.array([1e-300, 5e-324]))
    assert C.tolist() == [1e-300, 5e-324] and S.tolist() == [0.0, 0.0]


def test_the_committed_table_is_what_its_generator_prints():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_fresnel_tables.py")], check=True, capture_output=True, text=True).stdout
    assert out == open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_fresnel_tab.h")).read()


# ---- the specification against the fixture ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    return R.fixture()


def test_fixture_preconditions_and_quirks(golden):
    z, spirals, pp3, roads = golden
    assert len(spirals) >= 100 and len(pp3) >= 40 and 30 <= len(roads) <= 48 and max(len(r["geoms"]) for r in roads) <= 6
    geoms = [g for r in roads for g in r["geoms"]]
    assert max(g["length"] for g in geoms) <= 40.0 and os.path.getsize(os.path.join(ROOT, "tests", "golden", "road.npz")) < 1 << 20
    # no discrete decision rests on the last ulp
    for r in roads:
        d = np.diff(r["raw"], axis=0)
        assert not np.any(np.abs(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) - 0.02) < 1e-6)
    for g in geoms:
        q = g["length"] / 0.1
        assert g["length"] <= 1e-6 or abs(q - round(q)) >= 1e-9, g
        assert g["kind"] != R.ARC or abs(abs(g["curvature"]) - 1e-9) >= 1e-12
    for par, _, _ in pp3:
        assert par[0] == 0.0 or abs(par[0] / 0.1 - round(par[0] / 0.1)) >= 1e-9
    assert np.all(np.abs(z["spiral_par"][:, 5][z["spiral_par"][:, 5] != 0]) >= 1e-6)          # what TOL's derivation assumes
    # every quirk is there on purpose
    par = z["spiral_par"]
    assert (par[:, 5] < 0).any() and ((par[:, 4] != 0) & (par[:, 5] != 0)).any() and ((par[:, 5] == 0) & (par[:, 4] != 0)).any()
    assert ((par[:, 5] == 0) & (par[:, 4] == 0)).any() and set(z["spiral_n"].tolist()) >= {1, 2, 63, 64, 65, 129}
    sp = [g for g in geoms if g["kind"] == R.SPIRAL and g["length"] >= 1e-6]
    assert any((g["curvEnd"] - g["curvStart"]) / g["length"] < 0 for g in sp) and any(g["curvStart"] != 0 for g in sp)
    short = [(r, i) for r in roads for i, g in enumerate(r["geoms"]) if g["kind"] == R.SPIRAL and 1e-6 <= g["length"] < 1.98 and len(r["geoms"]) > 1]
    assert short
    for r, i in short:                                   # ... and loses every point but its first
        first = int(np.sum(r["points"][:i]))
        assert r["keep"][first + 1:first + r["points"][i]].sum() == 0
    tiny = [(r, i) for r in roads for i, g in enumerate(r["geoms"]) if g["kind"] == R.LINE and g["length"] == 1e-17 and g["x"] == 1.0]
    assert tiny and all(r["popped"][i] and r["points"][i] == 1 for r, i in tiny) and z["geom_popped"].sum() == len(tiny)
    assert any(g["kind"] == R.ARC and abs(g["curvature"]) < 1e-9 for g in geoms) and any(g["kind"] == R.ARC and abs(g["curvature"]) >= 1e-9 for g in geoms)
    assert {g["pRange"] for g in geoms if g["kind"] == R.PARAM_POLY3} == {0, 1} and set(z["pp3_range"].tolist()) == {0, 1}
    seams = 0
    for r in roads:
        if r["count"]:
            first = np.cumsum(r["points"])[:-1]
            seams += sum(1 for k in first if k < len(r["raw"]) and np.array_equal(r["raw"][k], r["raw"][k - 1]) and not r["keep"][k])
    assert seams >= 10
    assert any(r["count"] == 0 for r in roads) and set(z["geom_kind"].tolist()) == {0, 1, 2, 3, 4}
    assert sorted(z["refusal_name"].tolist()) == ["spiral_negative_length", "spiral_negative_n_interpolation"]


def test_the_specification_equals_every_fixture_curve(golden):
    z, spirals, pp3, roads = golden
    worst = 0.0
    for par, n, xy in spirals:
        got = R.spiral(*par, n)
        assert got.shape == xy.shape
        worst = max(worst, float(np.abs(got - xy).max()))
    print("Spiral: largest deviation", worst)
    assert worst <= TOL
    worst = 0.0
    for par, p_range, xy in pp3:
        got = R.param_poly3(par[0], par[1], par[2], par[3], par[4:], p_range)
        assert got.shape == xy.shape, par[0]
        worst = max(worst, float(np.abs(got - xy).max()))
    print("ParamPoly3: largest deviation", worst)
    assert worst <= TOL


def test_the_specification_equals_every_fixture_road(golden):
    z, spirals, pp3, roads = golden
    worst = dict(xy=0.0, s=0.0, kappa=0.0, raw=0.0)
    for i, r in enumerate(roads):
        got = R.planview(r["geoms"])
        assert got["count"] == r["count"], i
        full = [len(R.sample_geometry(g)[0]) for g in r["geoms"]]
        assert full == r["points"].tolist() and [bool(R.sample_geometry(g)[2]) for g in r["geoms"]] == r["popped"].tolist(), i
        if not r["count"]:
            continue
        assert np.array_equal(got["keep"], r["keep"]) and np.array_equal(got["popped"], r["popped"]), i
        for k in worst:
            worst[k] = max(worst[k], float(np.abs(got[k] - r[k]).max()))
    print("roads: largest deviations", worst)
    assert max(worst.values()) <= TOL


def test_numpys_powers_are_what_the_specification_states():
    """p ** 2 of numpy is p * p; p ** 3 goes through pow and is within an ulp of the (p * p) * p the device and the
    specification compute (build-defined)"""
    p = np.random.default_rng(3).uniform(0.0, 40.0, 20000)
    assert np.array_equal(p ** 2, p * p)
    assert np.all(np.abs(p ** 3 - R.cube(p)) <= np.spacing(p ** 3))


def test_linspace_is_numpys():
    rng = np.random.default_rng(4)
    for n in (1, 2, 3, 64, 100, 387):
        for _ in range(20):
            a, b = rng.uniform(-50, 50, 2)
            assert np.array_equal(R.linspace(a, b, n), np.linspace(a, b, n)) and np.array_equal(R.linspace(0.0, b, n), np.linspace(0, b, n))


# ---- the build-defined clothoid -----------------------------------------------------------------------------------------------------
def test_the_standard_rule_is_the_clothoid_of_the_quadrature():
    from scipy.integrate import quad
    rng = np.random.default_rng(11)
    worst, signs = 0.0, set()
    for k in range(50):
        sk, sg = (1, 1, -1, -1)[k % 4], (1, -1, 1, -1)[k % 4]
        length, h = rng.uniform(5.0, 40.0), rng.uniform(-np.pi, np.pi)
        k0, gamma = sk * rng.uniform(0.005, 0.1), sg * rng.uniform(0.001, 0.02)
        x0, y0 = rng.uniform(-100, 100, 2)
        signs.add((sk, sg))
        got = R.spiral(length, x0, y0, h, k0, gamma, 12, R.STANDARD)
        s = R.linspace(0.0, length, 12)
        theta = lambda t: h + k0 * t + gamma * t * t / 2
        for j in range(12):
            qx = quad(lambda t: np.cos(theta(t)), 0.0, s[j], epsabs=1e-12, epsrel=1e-12, limit=200)[0]
            qy = quad(lambda t: np.sin(theta(t)), 0.0, s[j], epsabs=1e-12, epsrel=1e-12, limit=200)[0]
            worst = max(worst, abs(got[j, 0] - (x0 + qx)), abs(got[j, 1] - (y0 + qy)))
    print("standard rule against quad: largest deviation", worst)
    assert len(signs) == 4 and worst <= 1e-9
    # with k0 == 0 and gamma > 0 the two rules are one
    a, b = R.spiral(20.0, 1.0, 2.0, 0.3, 0.0, 0.01, 50, R.REFERENCE), R.spiral(20.0, 1.0, 2.0, 0.3, 0.0, 0.01, 50, R.STANDARD)
    assert np.array_equal(a, b)
    # the issue's table: where the reference ends, and where the clothoid does
    for k0, gamma, ref_end, std_end in ((0.0, -0.01, (9.807, 13.476), (15.704, -5.585)), (0.05, 0.01, (11.411, 12.149), (2.214, 13.031))):
        assert np.allclose(R.spiral(20.0, 0.0, 0.0, 0.3, k0, gamma, 100, R.REFERENCE)[-1], ref_end, atol=6e-4)
        assert np.allclose(R.spiral(20.0, 0.0, 0.0, 0.3, k0, gamma, 100, R.STANDARD)[-1], std_end, atol=6e-4)


def test_refusals_and_strides_of_the_specification():
    line = dict(kind=R.LINE, s=0.0, x=0.0, y=0.0, hdg=0.0, length=3.0)
    assert R.planview([line])["count"] == 31
    for bad in (dict(line, length=-1.0), dict(line, x=np.nan), dict(line, kind=7), dict(line, kind=R.ARC, curvature=np.inf),
                dict(line, length=(R.MAX_RAW + 5) * 0.1)):
        assert R.planview([line, bad])["count"] == 0
    assert R.planview([])["count"] == 0 and R.planview([line] * 3, max_geom=2)["count"] == 0
    assert R.planview([dict(line, kind=R.ARC, curvature=0.1, length=0.0)])["count"] == 0       # an arc of length 0 has no point
    xy = np.stack([np.arange(11.0), np.zeros(11)], 1)
    v, c = R.route_vertices(xy, 5, 8)
    assert c == 3 and v[:, 0].tolist() == [0, 5, 10, 10, 10, 10, 10, 10]
    v, c = R.route_vertices(xy, 4, 8)
    assert c == 4 and v[:, 0].tolist() == [0, 4, 8, 10, 10, 10, 10, 10]
    v, c = R.route_vertices(xy, 1, 8)
    assert c == 11 and v[:, 0].tolist() == list(range(8))
    assert R.route_vertices(xy[:1], 1, 8) == (None, 0)


# ---- header <-> _ffi <-> layout ---------------------------------------------------------------------------------------------------
def test_header_ffi_and_layout_agree():
    import ctypes as C

    from tactics2d_amd import _ffi, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for name in ("SPIRAL_REFERENCE", "SPIRAL_STANDARD", "GEOM_LINE", "GEOM_SPIRAL", "GEOM_ARC", "GEOM_POLY3", "GEOM_PARAM_POLY3",
                 "PLANVIEW_RECORD_BYTES", "PLANVIEW_MAX_GEOM", "PLANVIEW_MAX_RAW", "ROAD_CURVES_PER_BLOCK"):
        assert vals["T2D_" + name] == getattr(L, name), name
    assert int(re.search(r"enum \{ T2D_PROFILE_PLANVIEW_ROUTES = (\d+) \}", header).group(1)) == L.PROFILE_PLANVIEW_ROUTES == L.PROFILE_SPLINE_ROUTES + 1 == 19
    assert (R.REFERENCE, R.STANDARD) == (L.SPIRAL_REFERENCE, L.SPIRAL_STANDARD) and R.MAX_RAW == L.PLANVIEW_MAX_RAW
    assert (R.LINE, R.SPIRAL, R.ARC, R.POLY3, R.PARAM_POLY3) == (L.GEOM_LINE, L.GEOM_SPIRAL, L.GEOM_ARC, L.GEOM_POLY3, L.GEOM_PARAM_POLY3)
    assert L.PLANVIEW_RECORD_BYTES == 112 == 8 + 5 * 8 + 8 * 8
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for name in ("t2d_spiral_curves", "t2d_param_poly3_curves", "t2d_planview_lines", "t2d_planview_routes"):
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
        assert _ffi.SYMBOLS[name] == (C.c_int, want), name
    debug = open(os.path.join(ROOT, "include", "t2d_debug.h")).read()
    from tactics2d_amd import debug as D
    assert int(re.search(r"T2D_MATH_FRESNEL = (\d+)", debug).group(1)) == D.MATH_FUNCTIONS["fresnel"][0]


def test_the_library_exports_the_entry_points_and_no_fresnel_hook():
    import ctypes

    from tactics2d_amd import _ffi, build
    build.build()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    for name in ("t2d_spiral_curves", "t2d_param_poly3_curves", "t2d_planview_lines", "t2d_planview_routes"):
        assert hasattr(lib, name), name
    assert not hasattr(lib, "t2d_debug_math")


# ---- the Python classes without a device ------------------------------------------------------------------------------------------
def test_the_classes_refuse_what_the_reference_refuses(golden):
    from tactics2d_amd.interpolator import Spiral, pack_planview
    z = golden[0]
    message = dict(zip(z["refusal_name"].tolist(), z["refusal_message"].tolist()))
    with pytest.raises(ValueError) as ei:
        Spiral.get_curve(-1.0, [0.0, 0.0], 0.0, 0.0, 0.01)
    assert str(ei.value) == message["spiral_negative_length"]
    with pytest.raises(ValueError) as ei:
        Spiral.get_curve(np.array([1.0, -2.0]), np.zeros((2, 2)), 0.0, 0.0, 0.01)
    assert str(ei.value) == message["spiral_negative_length"]
    with pytest.raises(ValueError) as ei:
        Spiral.get_curve(1.0, [0.0, 0.0], 0.0, 0.0, 0.01, -1)
    assert str(ei.value) == message["spiral_negative_n_interpolation"]
    with pytest.raises(ValueError):
        Spiral.get_curve(1.0, [0.0, 0.0], 0.0, 0.0, 0.01, rule="euler")
    one = Spiral.get_curve(1.0, [0.0, 0.0], 0.0, 0.0, 0.01, 0)                    # nothing is launched: no device is needed
    assert isinstance(one, np.ndarray) and one.shape == (0, 2)
    many = Spiral.get_curve(np.ones(3), np.zeros((3, 2)), np.zeros(3), np.zeros(3), np.full(3, 0.01), 0)
    assert many.xy.shape == (3, 0, 2) and many.count.tolist() == [0, 0, 0]
    g = dict(s=0.0, x=1.0, y=2.0, hdg=0.5, length="3.5")
    rec, n_geom = pack_planview([[dict(g, line={}), dict(g, paramPoly3=dict(aU=0, bU=1, cU=2, dU=3, aV=4, bV=5, cV=6, dV=7, pRange="arcLength"))],
                                 [dict(g, type="arc", curvature=0.25)]])
    assert tuple(rec.shape) == (2, 2, 14) and n_geom.tolist() == [2, 1]
    r = rec.numpy()
    assert r.view(np.int32).reshape(2, 2, 28)[:, :, :2].tolist() == [[[0, 0], [4, 1]], [[2, 0], [0, 0]]]
    assert r[0, 1, 1:].tolist() == [0.0, 1.0, 2.0, 0.5, 3.5, 0, 1, 2, 3, 4, 5, 6, 7] and r[1, 0, 6] == 0.25
    for bad in ([[dict(g)]], [[dict(g, line={}, arc=dict(curvature=1))]], [[dict(g, type="clothoid")]], [[dict(g, arc={})]],
                [[dict(g, line={})] * 65], [[dict(x=1.0, line={})]]):
        with pytest.raises(ValueError):
            pack_planview(bad)
    with pytest.raises(ValueError):
        pack_planview([[dict(g, line={})] * 3], max_geom=2)
