"""Bezier, B-spline and cubic spline curves without a device: the specification (tests/spline_ref.py) against the fixture made by
running the reference's compiled module (tests/golden/splines.npz, tests/golden/make_splines.py) -- BIT FOR BIT, every operation
being IEEE + - * / in the reference's order --; the point counts, the unsampled B-spline end, the duplicated cubic knots and the
three-point not-a-knot polyline; header <-> _ffi <-> layout for the new constants and symbols; and the host-side refusals with
the reference's messages."""
import os
import re

import numpy as np
import pytest

import spline_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "splines.npz")))
        g["ctrl_off"] = np.concatenate([[0], np.cumsum(g["n_ctrl"])])
        g["xy_off"] = np.concatenate([[0], np.cumsum(g["count"])])
        n_knots = np.where(g["knot_kind"] >= 1, g["n_ctrl"] + g["degree"] + 1, 0)
        g["knot_off"] = np.concatenate([[0], np.cumsum(n_knots)])
        _CACHE["g"] = g
    return _CACHE["g"]


def fixture_curve(c):
    """(kind, ctrl [n, 2], n_interpolation, degree, knots or None, boundary, derivs, xy [count, 2]) of fixture curve c"""
    g = fixture()
    knots = g["knots"][g["knot_off"][c]:g["knot_off"][c + 1]] if g["knot_kind"][c] >= 1 else None
    return (int(g["kind"][c]), g["ctrl"][g["ctrl_off"][c]:g["ctrl_off"][c + 1]], int(g["n_interpolation"][c]), int(g["degree"][c]), knots,
            int(g["boundary"][c]), g["derivs"][c], g["xy"][g["xy_off"][c]:g["xy_off"][c + 1]])


def spec_curve(c):
    kind, ctrl, ni, degree, knots, boundary, derivs, _ = fixture_curve(c)
    return S.curve(kind, ctrl, ni, degree, knots, boundary, derivs)


def test_the_fixture_covers_what_it_says():
    g = fixture()
    bez, bsp, cub = (g["kind"] == k for k in (S.BEZIER, S.BSPLINE, S.CUBIC))
    assert {(int(n), int(i)) for n, i in zip(g["n_ctrl"][bez], g["n_interpolation"][bez])} == \
        {(n, i) for n in (2, 3, 4, 5, 8, 16, 32) for i in (2, 3, 50, 63, 64, 65)}
    assert {(int(d), int(k), int(i)) for d, k, i in zip(g["degree"][bsp], g["knot_kind"][bsp], g["n_interpolation"][bsp])} == \
        {(d, k, i) for d in range(6) for k in range(5) for i in (1, 2, 64, 65, 100)}
    for d in range(6):
        n = g["n_ctrl"][bsp & (g["degree"] == d)]
        assert n.min() == d + 1 and n.max() == 32, d
    assert {(int(b), int(n), int(i)) for b, n, i in zip(g["boundary"][cub], g["n_ctrl"][cub], g["n_interpolation"][cub])} >= \
        {(b, n, i) for b in (1, 2, 3) for n in (3, 4, 5, 9, 32) for i in (2, 3, 20, 64)}
    assert {(int(b), int(s)) for b, s in zip(g["boundary"][cub], g["spacing"][cub])} == {(b, s) for b in (1, 2, 3) for s in range(7)}
    assert (np.abs(g["derivs"][cub & (g["boundary"] == 2)]) > 0).all()
    assert g["ctrl"][np.repeat(cub, g["n_ctrl"]), 0].max() > 200.0      # abscissae of a few hundred metres
    assert np.isfinite(g["xy"]).all() and 200 <= len(g["kind"]) <= 500


def test_the_specification_equals_the_fixture_bit_for_bit():
    g = fixture()
    worst = {S.BEZIER: 0.0, S.BSPLINE: 0.0, S.CUBIC: 0.0}
    different = []
    for c in range(len(g["kind"])):
        want, got = fixture_curve(c)[-1], spec_curve(c)
        assert got is not None and got.shape == want.shape, c
        worst[int(g["kind"][c])] = max(worst[int(g["kind"][c])], float(np.abs(got - want).max()))
        if not np.array_equal(got, want):
            different.append(c)
    print("largest deviation of the specification from the reference, Bezier / B-spline / cubic:", [worst[k] for k in sorted(worst)])
    assert not different, different


def test_point_counts_and_the_shapes_of_the_three_families():
    g = fixture()
    for c in range(len(g["kind"])):
        kind, ctrl, ni, degree, knots, boundary, _, xy = fixture_curve(c)
        n = len(ctrl)
        assert len(xy) == ((n - 1) * ni + 1 if kind == S.CUBIC else ni), c
        if kind == S.BEZIER:     # t = 0 is the first control point exactly; t = (n - 1) * (1 / (n - 1)) need not be 1
            assert np.array_equal(xy[0], ctrl[0]) and np.abs(xy[-1] - ctrl[-1]).max() < 1e-9, c
        if kind == S.CUBIC:
            assert np.array_equal(xy[-1], ctrl[-1]), c
            starts = xy[np.arange(n - 1) * ni]
            assert np.array_equal(starts, ctrl[:-1]), c                           # every segment starts on its knot, exactly
            ends = xy[np.arange(1, n) * ni - 1, 0]                                # ... and ends on the ACCUMULATED abscissa
            assert np.abs(ends - ctrl[1:, 0]).max() < 1e-9, c
    # the accumulated abscissa misses the knot in the last bits somewhere: the near-duplicate vertex is not an exact duplicate
    cub = np.flatnonzero((g["kind"] == S.CUBIC) & (g["n_interpolation"] == 64))
    assert any((fixture_curve(c)[-1][np.arange(1, len(fixture_curve(c)[1])) * 64 - 1, 0] != fixture_curve(c)[1][1:, 0]).any() for c in cub)


def test_the_end_of_a_bspline_is_not_sampled():
    g = fixture()
    seen = 0
    for c in np.flatnonzero((g["kind"] == S.BSPLINE) & (g["knot_kind"] == 2) & (g["degree"] >= 1) & (g["n_interpolation"] >= 64)):
        _, ctrl, ni, degree, knots, _, _, xy = fixture_curve(c)
        # a clamped curve starts on the first control point and would end on the last one at u_end, where the half-open
        # degree-0 test makes every basis 0: the sampler stops one step short of it
        assert np.abs(xy[0] - ctrl[0]).max() < 1e-9, c
        assert np.abs(xy[-1] - ctrl[-1]).max() > 1e-6, c
        u_last = knots[degree] + (ni - 1) * ((knots[len(ctrl)] - knots[degree]) / ni)
        assert u_last < knots[len(ctrl)], c
        seen += 1
    assert seen >= 6
    every_basis_zero = np.flatnonzero((g["kind"] == S.BSPLINE) & (g["knot_kind"] == 4))
    assert len(every_basis_zero) and all((fixture_curve(c)[-1] == 0.0).all() for c in every_basis_zero)


def test_three_point_not_a_knot_is_the_polyline():
    g = fixture()
    rows = np.flatnonzero((g["kind"] == S.CUBIC) & (g["boundary"] == S.NOT_A_KNOT) & (g["n_ctrl"] == 3))
    assert len(rows) >= 7
    polylines, residue = 0, []
    for c in rows:
        _, ctrl, ni, _, _, _, _, xy = fixture_curve(c)
        a, b, cc, d, m = S.cubic_parameters(ctrl, (0.0, 0.0), S.NOT_A_KNOT)
        # Rows 0 and 2 of the matrix are equal.  Where the elimination cancels them exactly, BandedSolve meets a zero pivot column
        # and returns zeros: the polyline.  Where (x / p) * p != x leaves a residue of an ulp, that residue IS the last pivot and m
        # is whatever it gives -- the reference's curve all the same (the fixture holds it, and the bit-for-bit test covers it).
        if m != [0.0, 0.0, 0.0]:
            residue.append(int(c))
            continue
        assert cc == [0.0, 0.0] and d == [0.0, 0.0], c
        chord = np.interp(xy[:, 0], ctrl[:, 0], ctrl[:, 1])
        assert np.abs(xy[:, 1] - chord).max() < 1e-9, c
        polylines += 1
    print("three-point not-a-knot rows:", len(rows), "polylines:", polylines, "rows whose last pivot is a rounding residue:", residue)
    assert polylines >= 7 and len(residue) <= 2
    equal = [c for c in rows if g["spacing"][c] == 3]       # equal spacing cancels exactly: always the polyline
    assert equal and not set(equal) & set(residue)
    four = np.flatnonzero((g["kind"] == S.CUBIC) & (g["boundary"] == S.NOT_A_KNOT) & (g["n_ctrl"] >= 4))
    for c in four[:12]:     # from four points on it is the not-a-knot spline: a dense solve of the same system agrees
        _, ctrl, *_ = fixture_curve(c)
        x, y = ctrl[:, 0], ctrl[:, 1]
        h, n = np.diff(x), len(x) - 1
        A, B = np.zeros((n + 1, n + 1)), np.zeros(n + 1)
        for i in range(1, n):
            A[i, i - 1:i + 2] = h[i - 1], 2 * (h[i - 1] + h[i]), h[i]
            B[i] = 6 * ((y[i + 1] - y[i]) / h[i] - (y[i] - y[i - 1]) / h[i - 1])
        A[0, :3] = -h[1], h[0] + h[1], -h[0]
        A[n, n - 2:] = -h[n - 1], h[n - 2] + h[n - 1], -h[n - 2]
        m = S.cubic_parameters(ctrl, (0.0, 0.0), S.NOT_A_KNOT)[4]
        assert np.abs(np.linalg.solve(A, B) - m).max() <= 1e-9 * max(1.0, np.abs(m).max()), c


def test_rows_the_device_refuses():
    pts = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0], [4.0, 4.0]])
    bad = pts.copy()
    bad[2, 1] = np.nan
    assert S.bezier(pts[:1], 10) is None and S.bezier(bad, 10) is None and S.bezier(pts, 10) is not None
    assert S.bspline(pts, None, 4, 10) is None and S.bspline(bad, None, 2, 10) is None
    assert S.bspline(pts, [0, 1, 2, 3, 2.5, 4, 5.0], 2, 10) is None and S.bspline(pts, [0, 1, 2, np.inf, np.inf, np.inf, np.inf], 2, 10) is None
    assert S.cubic(pts[:2]) is None and S.cubic(pts[[0, 2, 1, 3]]) is None and S.cubic(bad) is None
    assert S.cubic(pts, (np.nan, 0.0), 10, S.CLAMPED) is None and S.cubic(pts, (np.nan, 0.0), 10, S.NATURAL) is not None


def test_default_knots_are_numpys_linspace():
    for n in range(1, 33):
        for d in range(6):
            if n >= d + 1:
                assert np.array_equal(S.default_knots(n, d), np.linspace(0, 1, n + d + 1)), (n, d)


# ---- header <-> _ffi <-> layout ---------------------------------------------------------------------------------------------------
def test_header_ffi_and_layout_agree():
    import ctypes as C

    from tactics2d_amd import _ffi, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for name in ("SPLINE_BEZIER", "SPLINE_BSPLINE", "SPLINE_CUBIC", "SPLINE_NATURAL", "SPLINE_CLAMPED", "SPLINE_NOT_A_KNOT",
                 "SPLINE_MAX_CTRL", "SPLINE_MAX_DEGREE", "SPLINE_CURVES_PER_BLOCK", "PROFILE_SPLINE_ROUTES"):
        assert vals["T2D_" + name] == getattr(L, name), name
    assert L.SPLINE_MAX_CTRL >= 32 and L.SPLINE_MAX_DEGREE >= 5
    assert L.PROFILE_SPLINE_ROUTES == L.PROFILE_CURVE_ROUTES + 1 == max(v for k, v in vals.items() if k.startswith("T2D_PROFILE_"))
    assert (S.BEZIER, S.BSPLINE, S.CUBIC) == (L.SPLINE_BEZIER, L.SPLINE_BSPLINE, L.SPLINE_CUBIC)
    assert (S.NATURAL, S.CLAMPED, S.NOT_A_KNOT) == (L.SPLINE_NATURAL, L.SPLINE_CLAMPED, L.SPLINE_NOT_A_KNOT)
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    for name in ("t2d_spline_curves", "t2d_spline_routes"):
        params = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text).group(1).split(",")
        want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
        assert _ffi.SYMBOLS[name] == (C.c_int, want), name
    assert vals["T2D_ABI_VERSION"] == L.ABI_VERSION        # additions only
    dev = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_spline_dev.h")).read()
    assert re.search(r"kSplineMaxCtrl = (\d+), kSplineMaxDegree = (\d+)", dev).groups() == (str(L.SPLINE_MAX_CTRL), str(L.SPLINE_MAX_DEGREE))


def test_the_library_exports_the_two_entry_points():
    import ctypes

    from tactics2d_amd import _ffi, build
    build.build()
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert hasattr(lib, "t2d_spline_curves") and hasattr(lib, "t2d_spline_routes")


# ---- the host-side refusals --------------------------------------------------------------------------------------------------------
def _refusal_calls():
    from tactics2d_amd.interpolator import Bezier, BSpline, CubicSpline
    pts = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0], [4.0, 4.0]])
    return {
        "bezier_shape": lambda: Bezier.get_curve(np.zeros((4, 3)), 10),
        "bezier_order_zero": lambda: Bezier.get_curve(pts, 10, order=0),
        "bezier_order_mismatch": lambda: Bezier.get_curve(pts, 10, order=2),
        "bezier_one_point": lambda: Bezier.get_curve(pts[:1], 10),
        "bezier_n_interpolation": lambda: Bezier.get_curve(pts, 1),
        "bspline_degree_negative": lambda: BSpline.get_curve(pts, degree=-1),
        "bspline_shape": lambda: BSpline.get_curve(np.zeros((4, 3)), degree=2),
        "bspline_knot_count": lambda: BSpline.get_curve(pts, np.linspace(0, 1, 5), degree=2),
        "bspline_knots_decreasing": lambda: BSpline.get_curve(pts, np.array([0, 1, 2, 3, 2.5, 4, 5.0]), degree=2),
        "bspline_too_few_control_points": lambda: BSpline.get_curve(pts, degree=4),
        "bspline_n_interpolation": lambda: BSpline.get_curve(pts, degree=2, n_interpolation=0),
        "cubic_boundary_type": lambda: CubicSpline.get_curve(pts, boundary_type=0),
        "cubic_shape": lambda: CubicSpline.get_curve(np.zeros((4, 3))),
        "cubic_too_few_control_points": lambda: CubicSpline.get_curve(pts[:2]),
        "cubic_x_not_increasing": lambda: CubicSpline.get_curve(pts[[0, 2, 1, 3]]),
        "cubic_n_interpolation": lambda: CubicSpline.get_curve(pts, n_interpolation=1),
    }


def test_host_side_refusals_carry_the_references_messages():
    g = fixture()
    calls = _refusal_calls()
    assert sorted(calls) == sorted(str(n) for n in g["refusal_name"])
    for name, message in zip(g["refusal_name"], g["refusal_message"]):
        with pytest.raises(ValueError) as ei:
            calls[str(name)]()
        assert str(ei.value) == str(message), name


def test_batched_refusals_and_the_caps():
    from tactics2d_amd import layout as L
    from tactics2d_amd.interpolator import Bezier, BSpline, CubicSpline, spline_check
    rng = np.random.default_rng(3)
    batch = np.stack([np.cumsum(rng.uniform(0.5, 2.0, (5, 6)), 1), rng.uniform(-1, 1, (5, 6))], 2)     # [5, 6, 2], x increasing
    assert spline_check("cubic", batch, n_interpolation=20)[:4] == (L.SPLINE_CUBIC, 5, 6, 20)
    assert spline_check("cubic", batch, n_interpolation=20, boundary_type=CubicSpline.BoundaryType.Clamped)[5] == L.SPLINE_CLAMPED
    assert spline_check("cubic", batch, n_interpolation=20)[6] == 5 * 20 + 1 and spline_check("bezier", batch, n_interpolation=7)[6] == 7
    wrong = batch.copy()
    wrong[3, 4, 0] = wrong[3, 3, 0]                               # one row of the batch repeats an abscissa ...
    with pytest.raises(ValueError, match="strictly increasing"):
        CubicSpline.get_curve(wrong)
    assert spline_check("cubic", wrong, n_ctrl=np.array([6, 6, 6, 4, 6]))[1] == 5     # ... past the points that row uses: no refusal
    knots = np.tile(np.linspace(0, 1, 6 + 3 + 1), (5, 1))
    knots[2, 8] = 0.1
    with pytest.raises(ValueError, match="non-decreasing"):
        BSpline.get_curve(batch, knots, degree=3)
    assert spline_check("bspline", batch, np.array([6, 6, 4, 6, 6]), 10, 3, knots)[4] == 3
    with pytest.raises(ValueError, match=r"Expected 10 knots, got 9\."):
        BSpline.get_curve(batch, knots[:, :9], degree=3)
    with pytest.raises(ValueError, match="device cap"):
        Bezier.get_curve(np.zeros((2, L.SPLINE_MAX_CTRL + 1, 2)), 10)
    with pytest.raises(ValueError, match="device cap"):
        BSpline.get_curve(np.zeros((2, 12, 2)), degree=L.SPLINE_MAX_DEGREE + 1)
    with pytest.raises(ValueError):
        Bezier.get_curve(batch, 10, n_ctrl=np.array([6, 6, 6]))
    with pytest.raises(ValueError):
        spline_check("hermite", batch)
    for ok in (1, 2, 3, CubicSpline.BoundaryType.Natural):
        spline_check("cubic", batch, boundary_type=ok)
    for bad in (0, 4, "NotAKnot"):
        with pytest.raises(ValueError, match="Invalid boundary type"):
            CubicSpline.get_curve(batch, boundary_type=bad)


def test_no_device_means_t2derror_not_a_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from tactics2d_amd import _ffi
    from tactics2d_amd.interpolator import Bezier, BSpline, CubicSpline
    pts = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0], [4.0, 4.0]])
    for call in (lambda: Bezier.get_curve(pts, 10), lambda: BSpline.get_curve(pts, degree=2), lambda: CubicSpline.get_curve(pts)):
        with pytest.raises(_ffi.T2DError) as ei:
            call()
        assert ei.value.code == _ffi.ERR_HIP
