"""The off-route detector without a device: the fp64 restatement (tests/route_ref.py, the kernel's operation order) against exact
rational arithmetic, the golden file made by running the reference's OffRoute class (tests/golden/make_off_route.py), the host
rules of traffic.OffRoute / routes_to_csr, the declared interface, and the bands of the GPU scene tests checked with the C
oracle's CPU rollouts (the table in tests/test_gpu_off_route.py comes from test_the_bands_of_the_gpu_scene_tests_hold_on_the_cpu).
"""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import helpers as H
import route_ref as R
import route_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ restatement vs exact
def test_known_answers_where_every_operation_is_exact():
    for name, route, (px, py), thr, off, d, seg in R.kats():
        got_d, got_off, got_seg = R.distance(route, px, py, thr)
        d2, ex_seg = R.exact_d2(route, px, py)
        assert d2 == Fraction(float(np.float32(d))) ** 2, name                     # the stated distance is the exact one
        assert (got_off, got_seg) == (off, seg) and got_d == np.float32(d), (name, got_d, got_off, got_seg)
        assert R.exact_off(d2, thr) == off and ex_seg == seg, name
        # the vectorised statement is the scalar one, bit for bit
        r = np.float32(route)
        vd, vo, vs = R.evaluate(r[None, :, 0], r[None, :, 1], [len(r)], [px], [py], [thr], [1])
        assert vd.view(np.uint32)[0] == np.float32(got_d).view(np.uint32) and bool(vo[0]) == off and vs[0] == seg, name


def test_restatement_against_exact_arithmetic_on_random_cases():
    """>= 20 000 seeded cases (the issue's recipe, route_ref.random_cases).  Verdicts must agree wherever the exact
    |d2 - thr^2| exceeds 2^-40 thr^2; the share left out by that margin is capped at 0.1 %."""
    n = off_count = left_out = disagree = 0
    worst = 0.0
    for route, px, py, thr in R.random_cases(20000, seed=7):
        n += 1
        d, off, seg = R.distance(route, px, py, thr)
        d2, ex_seg = R.exact_d2(route, px, py)
        t2 = Fraction(float(thr)) ** 2
        off_count += R.exact_off(d2, thr)
        if abs(d2 - t2) <= t2 / 2 ** 40:
            left_out += 1
        elif off != R.exact_off(d2, thr):
            disagree += 1
        r = route.astype(np.float64)
        fp = min(R.seg_d2(r[k, 0], r[k, 1], r[k + 1, 0], r[k + 1, 1], np.float64(px), np.float64(py)) for k in range(len(r) - 1))
        if d2 > 0:
            worst = max(worst, float(abs(Fraction(float(fp)) - d2) / d2))
    print(f"cases {n}, off-route {off_count}, left out {left_out}, disagreements {disagree}, largest relative error of d2 {worst:.2e}")
    assert n >= 20000 and disagree == 0
    assert left_out <= n // 1000, left_out
    assert 0.1 < off_count / n < 0.9      # (the recipe exercises both verdicts)
    assert worst < 1e-13


def test_build_defined_rows_of_the_restatement():
    r = np.float32([[0, 0], [4, 0]])
    VX, VY = np.repeat(r[None, :, 0], 6, 0), np.repeat(r[None, :, 1], 6, 0)
    x = np.float32([1, 1, np.nan, np.inf, 1, 1]); y = np.float32([3, 3, 0, 0, 3, 3])
    thr = np.float32([1, 1, 1, 1, np.nan, -1])
    d, off, seg = R.evaluate(VX, VY, [2, 2, 2, 2, 2, 2], x, y, thr, [1, 0, 1, 1, 1, 1])
    assert off.tolist() == [1, 0, 0, 0, 0, 1]           # inactive, NaN / inf position: 0; NaN threshold: never; negative: always
    assert np.isnan(d[[1, 2, 3]]).all() and d[0] == 3 and d[4] == 3 and d[5] == 3
    d, off, seg = R.evaluate(VX, VY, [2, 1, 0, 2, 2, 2], x, y, thr, np.ones(6))   # fewer than two vertices: no route
    assert off.tolist() == [1, 0, 0, 0, 0, 1] and np.isnan(d[[1, 2]]).all()


# ------------------------------------------------------------------------------------------------ the golden file
def test_golden_file_against_the_restatement_and_the_host_rules():
    """tests/golden/off_route.npz was made by RUNNING the reference's OffRoute (stand-in shapely with an exact distance): it
    pins the wiring -- centre point, strict >, list or LineString routes, the exceptions -- not GEOS."""
    from tactics2d_amd import traffic as T
    g = H.load_npz("off_route.npz")
    assert len(g["case_name"]) >= 40 and 0 < g["off"].sum() < len(g["off"])
    for c, name in enumerate(g["case_name"]):
        route = g["verts"][g["offsets"][c]:g["offsets"][c + 1]]
        px, py = g["point"][c]
        d, off, _ = R.distance(route, px, py, g["threshold"][c])
        assert int(off) == g["off"][c], name
        d2, _ = R.exact_d2(route, px, py)
        assert (str(d2.numerator), str(d2.denominator)) == (str(g["exact_d2_num"][c]), str(g["exact_d2_den"][c])), name
        # what reset() accepted, as_polyline accepts, with the same vertices -- a list of points and a LineString-like alike
        class LS:
            coords = [tuple(map(float, p)) for p in route]
        assert np.array_equal(T.as_polyline(LS() if g["as_linestring"][c] else route.tolist()), route), name
    names = {str(n) for n in g["case_name"]}
    assert {"at the threshold: not off", "one fp32 ulp further: off", "negative threshold: off at distance 0"} <= names
    # exceptions: update() before reset(), and every route reset() refused
    assert str(g["before_reset_exc"].reshape(-1)[0]) == "ValueError"
    with pytest.raises(ValueError):
        T.OffRoute(1.0).update()
    assert sorted(map(str, g["refused_name"])) == sorted(R.UNCOERCIBLE)
    for name, exc in zip(g["refused_name"], g["refused_exc"]):
        assert str(exc) == "TypeError", name
        with pytest.raises(TypeError):
            T.OffRoute(1.0).reset(R.UNCOERCIBLE[str(name)])
        with pytest.raises(TypeError):
            T.routes_to_csr([[R.UNCOERCIBLE[str(name)]]])


# ------------------------------------------------------------------------------------------------ host-side marshalling
def test_routes_to_csr():
    from tactics2d_amd.traffic import routes_to_csr
    so, vo, xy = routes_to_csr([[[(0, 0), (1, 0)], np.ones((3, 2))], [], [[(0, 0, 9), (1, 1, 9), (2, 2, 9)]]])
    assert so.tolist() == [0, 2, 2, 3] and vo.tolist() == [0, 2, 5, 8]
    assert so.dtype == vo.dtype == np.int32 and xy.dtype == np.float32 and xy.shape == (8, 2)
    assert xy[5:].tolist() == [[0, 0], [1, 1], [2, 2]]       # (z is dropped, as a LineString's distance ignores it)
    so, vo, xy = routes_to_csr([])
    assert so.tolist() == [0] and vo.tolist() == [0] and xy.shape == (0, 2)


def test_the_interface_is_there():
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.history import DeviceTrajectory, ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.traffic import BatchedScenarioManager, OffRoute, TrafficStatus
    vp = C.c_void_p
    assert _ffi.SYMBOLS["t2d_set_routes"] == (C.c_int, [vp, C.c_int32, vp, vp, vp, vp, vp, vp])
    assert _ffi.SYMBOLS["t2d_set_route_assignment"] == (C.c_int, [vp, vp, vp])
    assert _ffi.SYMBOLS["t2d_set_routes_from_traj"] == (C.c_int, [vp, vp, C.c_int32, vp, vp, vp, vp, vp])
    assert _ffi.SYMBOLS["t2d_off_route"] == (C.c_int, [vp, vp, vp, vp])
    assert _ffi.SYMBOLS["t2d_off_route_buffers"] == (C.c_int, [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_size_t)])
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    for name in ("t2d_set_routes", "t2d_set_route_assignment", "t2d_set_routes_from_traj", "t2d_off_route", "t2d_off_route_buffers"):
        assert re.search(r"\bint " + name + r"\(", header), name
    assert int(re.search(r"#define T2D_MAX_ROUTE_SET_VERTS (\d+)", header).group(1)) == L.MAX_ROUTE_SET_VERTS >= 4096
    assert int(re.search(r"#define T2D_ABI_VERSION (\d+)", header).group(1)) == L.ABI_VERSION == 13   # new symbols only
    assert re.search(r"9 = off-route \(t2d_off_route\)", header) and L.PROFILE_OFF_ROUTE == 9
    for name in ("set_routes", "set_route_assignment", "set_routes_from", "clear_routes", "off_route", "off_route_buffers",
                 "off_route_all", "off_route_host"):
        assert callable(getattr(ParticipantPool, name)), name
    for cls in (DeviceTrajectory, ReplaySource):
        assert callable(cls.traces) and callable(cls.set_routes_from)
    assert callable(OffRoute.update) and callable(OffRoute.distance) and callable(OffRoute.reset)
    assert TrafficStatus.OFF_ROUTE == 5
    assert "_after_step" in BatchedScenarioManager.__dict__


def test_no_new_field_or_flag_bit():
    """the detector is a launch of its own: the header gains no T2D_F_* field and no T2D_FLAG_* bit"""
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    assert int(re.search(r"T2D_F_COUNT = (\d+)", header).group(1)) == 24
    assert sorted(set(re.findall(r"#define (T2D_FLAG_\w+)", header))) == ["T2D_FLAG_COLLISION_DYNAMIC", "T2D_FLAG_COLLISION_STATIC",
                                                                        "T2D_FLAG_OFF_LANE", "T2D_FLAG_OUT_BOUND"]


# ------------------------------------------------------------------------------------------------ bands, on the CPU
def _shares(off, seg, routed):
    return float(off[routed].mean()), float((seg[routed] != 0).mean())


@pytest.mark.parametrize("name", ["highway", "intersection", "mixed"])
def test_the_bands_of_the_gpu_scene_tests_hold_on_the_cpu(oracle, name):
    """The restatement alone, fed with the C oracle's rollout of the scene (8 steps of the scene's random actions), meets the
    bands the GPU tests assert: off-route share of the active, routed participants strictly inside (0.02, 0.98) after every step
    and for every variant; nearest segment != 0 for at least a quarter where routes have many segments."""
    sc = RS.scene(name)
    states = RS.oracle_rollout(oracle, sc, 8, seed=21)
    for variant in ("shared", "per_env", "permuted"):
        sets, soe, ro, thr = RS.build(sc, variant)
        routed = (ro >= 0) & (sc.active != 0)
        assert routed.mean() > 0.85
        rows = []
        for st in states[1:]:
            _, off, seg = R.evaluate_sets(sets, soe, ro, sc.A, st[:, 0], st[:, 1], thr, sc.active)
            rows.append(_shares(off, seg, routed))
            assert 0.02 < rows[-1][0] < 0.98, (name, variant, rows)
            if name != "highway":
                assert rows[-1][1] >= 0.25, (name, variant, rows)
        print(name, variant, "off", " ".join(f"{a:.3f}" for a, _ in rows), "| segment != 0", " ".join(f"{b:.3f}" for _, b in rows))


def test_the_bands_of_the_gpu_trace_test_hold_on_the_cpu(oracle):
    """Trace routes: a 32-step oracle rollout is the recording; a second rollout from the same start with perturbed actions is
    evaluated against the recorded traces.  Over the 32 steps together the off-route share lies inside (0.02, 0.98) and the
    nearest segment is not segment 0 for at least a quarter."""
    from test_gpu_off_route import TRACE_THRESHOLD, perturb_actions, trace_scene
    sc = trace_scene()
    rec = RS.oracle_rollout(oracle, sc, 32, seed=5)
    run = RS.oracle_rollout(oracle, sc, 32, seed=5, perturb=perturb_actions)
    xy = np.stack([s[:, :2] for s in rec])
    first, last = np.zeros(sc.n, np.int32), np.full(sc.n, 32, np.int32)
    offs, segs = [], []
    for st in run[1:]:
        _, off, seg = R.evaluate_traces(xy, first, last, np.arange(sc.n_env), np.arange(sc.n) % sc.A, sc.A, st[:, 0], st[:, 1],
                                        np.full(sc.n, TRACE_THRESHOLD, np.float32), sc.active)
        offs.append(off.mean()); segs.append((seg != 0).mean())
    print("off per step", " ".join(f"{a:.3f}" for a in offs), "| overall", np.mean(offs), "| segment != 0 overall", np.mean(segs))
    assert 0.02 < np.mean(offs) < 0.98 and np.mean(segs) >= 0.25
