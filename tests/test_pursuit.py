"""The pure-pursuit and cruise / ACC controllers without a GPU: the numpy restatement (tests/pursuit_ref.py) and the host mirrors
(tactics2d_amd.controller.AccelerationController / PurePursuitController) against tests/golden/pursuit.npz -- recorded by
running the reference's own classes, tests/golden/make_pursuit.py --, the build-defined walk on known answers, header <-> Python
constants, and the closed-loop bands that tests/test_gpu_pursuit.py holds the device to.

Measured here: pursuit_ref equals the fixture BIT FOR BIT on all 3600 calls (cruise, ACC, the lateral law, step), NaN for NaN.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import pid_scenes as PS
import pursuit_ref as UR
import pursuit_scenes as US
import route_scenes as RS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _same(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


# ---------------------------------------------------------------------------------------------------- the laws
def test_ref_equals_the_fixture_bit_for_bit():
    f = US.fixture()
    c_in, a_in, l_in = f["c_in"], f["a_in"], f["l_in"]
    R = US.accel_rows(f["c_par"], 0)
    assert _same(UR.cruise(R, c_in[:, 0], c_in[:, 1], c_in[:, 2]), f["c_out"])
    R = US.accel_rows(f["a_par"], 1)
    assert _same(UR.acc(R, *[a_in[:, k] for k in range(8)]), f["a_out"])
    steer, _ = UR.lateral(l_in[:, 0], l_in[:, 1], l_in[:, 2], l_in[:, 3], l_in[:, 4], l_in[:, 5])
    assert _same(steer, f["l_out"])
    # step: the recorded d, the stand-in's point, then both laws
    s_in, par = f["s_in"], f["s_par"]
    R = US.accel_rows(par[:, 2:], 0, par[:, 0], par[:, 1], 1)
    d = UR.pre_aiming_distance(R, s_in[:, 3])
    assert _same(d, f["s_d"])
    pts = np.array([UR.interpolate(f["lines"][k][:f["line_nv"][k]], dk) for k, dk in zip(f["s_line"], d)])
    assert _same(pts, f["s_point"])
    steer, _ = UR.lateral(s_in[:, 0], s_in[:, 1], s_in[:, 2], pts[:, 0], pts[:, 1], s_in[:, 5])
    front = f["s_front"]
    has = ~np.isnan(front[:, 0])
    accel = np.where(has, UR.acc(R, s_in[:, 0], s_in[:, 1], s_in[:, 3], s_in[:, 4], front[:, 0], front[:, 1], front[:, 2], front[:, 3]),
                     UR.cruise(R, s_in[:, 3], s_in[:, 6], s_in[:, 4]))
    assert has.sum() > 200 and (~has).sum() > 200
    assert _same(steer, f["s_out"][:, 0]) and _same(accel, f["s_out"][:, 1])


def test_the_fixture_reaches_what_the_issue_lists():
    f = US.fixture()
    # cruise: each clip binds, and neither
    R, c_in = US.accel_rows(f["c_par"], 0), f["c_in"]
    raw = (c_in[:, 1] - c_in[:, 0]) / R[:, UR.KP]
    step = R[:, UR.ACCEL_CHANGE_RATE] * R[:, UR.DELTA_T]
    rate = (raw < c_in[:, 2] - step) | (raw > c_in[:, 2] + step)
    mid = np.clip(raw, c_in[:, 2] - step, c_in[:, 2] + step)
    limit = (mid < R[:, UR.MIN_ACCEL]) | (mid > R[:, UR.MAX_ACCEL])
    assert rate.sum() > 100 and limit.sum() > 50 and (~rate & ~limit).sum() > 100 and (rate & ~limit).sum() > 100
    assert (f["c_out"] == R[:, UR.MAX_ACCEL]).any() and (f["c_out"] == R[:, UR.MIN_ACCEL]).any()
    # ACC: distance_target at both clips and between, leaders faster and slower, leaders braking
    R, a_in = US.accel_rows(f["a_par"], 1), f["a_in"]
    target = a_in[:, 2] * R[:, UR.INTERVAL_LON] + 5.0
    assert (target < 7).sum() > 50 and (target > 80).sum() > 50 and ((target > 7) & (target < 80)).sum() > 50
    assert (a_in[:, 6] > a_in[:, 2]).sum() > 100 and (a_in[:, 6] < a_in[:, 2]).sum() > 100 and (a_in[:, 7] < -1).sum() > 100
    # the lateral law: ahead, abeam, behind, coincident (+-pi/2 and NaN)
    l_in, out = f["l_in"], f["l_out"]
    same = (l_in[:, 0] == l_in[:, 3]) & (l_in[:, 1] == l_in[:, 4])
    assert same.sum() > 100 and np.isnan(out[same]).sum() > 30 and (np.abs(out[same]) == np.pi / 2).sum() > 30
    assert (np.isnan(out) == (same & (l_in[:, 2] == 0))).all()
    bearing = np.arctan2(l_in[:, 4] - l_in[:, 1], l_in[:, 3] - l_in[:, 0]) - l_in[:, 2]
    c = np.cos(bearing[~same])
    assert (c > 0.9).sum() > 100 and (np.abs(c) < 0.1).sum() > 100 and (c < -0.9).sum() > 100
    # step: negative, zero and large speeds, d on both sides of the max
    v, grew = f["s_in"][:, 3], f["s_d"] > f["s_par"][:, 0]
    assert (v < 0).sum() > 100 and (v == 0).sum() > 100 and (v > 60).sum() > 100
    assert grew.sum() > 100 and (f["s_d"] == f["s_par"][:, 0]).sum() > 100 and (f["s_d"][v <= 0] == f["s_par"][v <= 0, 0]).all()
    # styles inside, at and beyond +-1; refusals by class
    s = f["y_style"]
    assert (np.abs(s) > 1).sum() >= 3 and (np.abs(s) == 1).sum() >= 2 and ((np.abs(s) < 1) & (s != 0)).sum() >= 4
    assert {"ValueError", "TypeError", "AttributeError", ""} == set(f["r_error"])
    assert os.path.getsize(US.GOLDEN) < 400 * 1024


# ---------------------------------------------------------------------------------------------------- the host mirrors
class _State:
    def __init__(self, x, y, heading, speed, accel):
        self.x, self.y, self.heading, self.speed, self.accel = x, y, heading, speed, accel


def _set(c, par):
    for k, v in zip(("kp", "accel_change_rate", "max_accel", "min_accel", "interval", "delta_t"), par):
        setattr(c, k, float(v))


def test_mirror_steps_equal_the_fixture():
    from tactics2d_amd.controller import AccelerationController, PurePursuitController, interpolate
    f = US.fixture()
    for i in range(0, 900, 3):
        sp, ts, last = f["c_in"][i]
        c = AccelerationController(ts)
        _set(c, f["c_par"][i])
        assert c.step(_State(0.0, 0.0, 0.0, sp, last)) == (0.0, f["c_out"][i])
        x, y, sp, last, fx, fy, fs, fa = f["a_in"][i + 1]
        c = AccelerationController()
        _set(c, f["a_par"][i + 1])
        assert c.step(_State(x, y, 0.0, sp, last), front_state=_State(fx, fy, 0.0, fs, fa)) == (0.0, f["a_out"][i + 1])
        x, y, h, px, py, wb = f["l_in"][i + 2]
        assert _same(PurePursuitController()._lateral_control(_State(x, y, h, 1.0, 0.0), (px, py), wb), f["l_out"][i + 2])
    for i in range(0, 900, 2):
        par, (x, y, h, sp, last, wb, ts) = f["s_par"][i], f["s_in"][i]
        c = PurePursuitController(par[0], ts)
        c.interval = par[1]
        _set(c._longitudinal_control, par[2:])
        line = f["lines"][f["s_line"][i]][:f["line_nv"][f["s_line"][i]]]
        assert c.pre_aiming_distance(sp) == f["s_d"][i] and _same(interpolate(line, f["s_d"][i]), f["s_point"][i])
        front = f["s_front"][i]
        kw = {} if np.isnan(front[0]) else dict(front_state=_State(front[0], front[1], 0.0, front[2], front[3]))
        assert _same(c.step(_State(x, y, h, sp, last), line, wb, **kw), f["s_out"][i])
    c = PurePursuitController()
    assert c.step(_State(0.0, 0.0, 0.0, 1.0, 0.0), [(0, 0), (20, 0)])[0] == c.step(_State(0.0, 0.0, 0.0, 1.0, 0.0), [(0, 0), (20, 0)], 2.637)[0]


def test_mirror_styles_defaults_and_refusals():
    from tactics2d_amd.controller import AccelerationController, PurePursuitController
    from tactics2d_amd import layout as L
    f = US.fixture()
    names = ("kp", "speed_factor", "accel_change_rate", "max_accel", "min_accel", "interval")
    for s, acc, pp in zip(f["y_style"], f["y_acc"], f["y_pp"]):
        for style in (float(s),) + ((int(s),) if s == int(s) else ()):
            c = PurePursuitController()
            c.update_driving_style(style)
            assert [getattr(c._longitudinal_control, k) for k in names] == list(acc) and c.interval == pp
            a = AccelerationController()
            a.update_driving_style(style)
            assert [getattr(a, k) for k in names] == list(acc)
    errors = {"": None, "ValueError": ValueError, "AttributeError": AttributeError, "TypeError": TypeError}
    calls = {"acc_ctor": lambda v: AccelerationController(v), "pp_ctor": lambda v: PurePursuitController(*v),
             "acc_style": lambda v: AccelerationController().update_driving_style(v),
             "pp_style": lambda v: PurePursuitController().update_driving_style(v),
             "acc_configure": lambda v: AccelerationController().configure(**v),
             "pp_configure": lambda v: PurePursuitController().configure(**v),
             "acc_front": lambda v: AccelerationController().step(_State(0.0, 0.0, 0.0, 3.0, 0.0), front_state=v),
             "pp_front": lambda v: PurePursuitController().step(_State(0.0, 0.0, 0.0, 3.0, 0.0), [(0, 0), (20, 0)], front_state=v)}
    assert sum(w.endswith("_front") and e == "TypeError" for (w, _), e in zip(f["r_calls"], f["r_error"])) == 3
    for (what, arg), want in zip(f["r_calls"], f["r_error"]):
        if errors[str(want)] is None:
            calls[what](arg)
        else:
            with pytest.raises(errors[str(want)]):
                calls[what](arg)
    a, p = AccelerationController(), PurePursuitController()
    assert (a.kp, a.speed_factor, a.accel_change_rate, a.max_accel, a.min_accel, a.interval, a.delta_t, a.target_speed) == \
        (3.5, 1.0, 3.0, 1.5, -4.0, 2.0, 0.05, 5.0)
    assert (p.interval, p.min_pre_aiming_distance, p.target_speed) == (1.0, 10.0, 5.0)
    r = p.row("acc")
    assert (r[:8] == [10.0, 1.0, 3.5, 3.0, 1.5, -4.0, 2.0, 0.05]).all() and r[L.PURSUIT_LAT_MODE] == 1 and r[L.PURSUIT_LON_MODE] == 1
    assert np.isnan(r[L.PURSUIT_WHEEL_BASE]) and r[L.PURSUIT_LANE_HALF_WIDTH] == 1.875 and r[L.PURSUIT_HORIZON] == np.inf
    assert a.row()[L.PURSUIT_LAT_MODE] == 0 and a.row("caller")[L.PURSUIT_LON_MODE] == 2 and len(r) == L.PURSUIT_COLS == UR.COLS
    a.update_driving_style(1.0)
    assert a.speed_factor == 1.2 and a.row()[L.PURSUIT_KP] == 2.5    # speed_factor: set, never read
    with pytest.raises(ValueError):
        a.row("idm")


# ---------------------------------------------------------------------------------------------------- the walk
def _la(route, x, y, d):
    la = UR.look_ahead(np.float32(route), x, y, d)
    return None if la is None else (float(la["point"][0]), float(la["point"][1]), la["segment"], la["target_segment"], la["events"])


def test_walk_known_answers():
    """Pins the REFERENCE, not the feature: hand-computed answers for the numpy restatement of the walk (tests/pursuit_ref.py, itself
    test infrastructure), so it passes with or without the product code.  tests/test_gpu_pursuit.py then holds the kernel to that
    restatement on the same cases."""
    assert _la([(0, 0), (16, 0)], 4, 1, 8) == (12.0, 0.0, 0, 0, 0)                               # a single segment
    L = [(0, 0), (8, 0), (8, 4), (20, 4), (20, -30)]
    assert _la(L, 4, -1, 4) == (8.0, 0.0, 0, 0, 0)                                              # exactly on a vertex
    assert _la(L, 4, 2, 8) == (8.0, 4.0, 0, 1, 0)
    assert _la(L, 2, 0, 6 + 4 + 12 + 5) == (20.0, -1.0, 0, 3, 0)                                # crossing three vertices
    Z = [(0, 0), (4, 0), (4, 0), (4, 0), (4, 8), (4, 8), (9, 8)]                                # zero-length segments inside the walk
    assert _la(Z, 1, 0, 3 + 8 + 2) == (6.0, 8.0, 0, 5, 0)
    assert _la(Z, 1, 0, 3) == (4.0, 0.0, 0, 0, 0) and _la(Z, 1, 0, 3.5) == (4.0, 0.5, 0, 3, 0)
    assert _la([(0, 0), (4, 0), (4, 3)], 1, 0, 10) == (4.0, 3.0, 0, 1, UR.ROUTE_END)            # shorter than the look-ahead
    assert _la([(0, 0), (4, 0), (4, 3), (4, 3)], 1, 0, 10) == (4.0, 3.0, 0, 2, UR.ROUTE_END)
    assert _la(L, -5, 3, 2) == (2.0, 0.0, 0, 0, 0)                                              # before the first vertex: from it
    assert _la(L, 25, -40, 2) == (20.0, -30.0, 3, 3, UR.ROUTE_END)                              # beyond the last: the last vertex
    assert _la([(2, 2), (2, 2), (2, 2)], 0, 0, 1) is None                                       # no route
    # the closed 24-gon at r = 14: over the seam, and a look-ahead longer than the lap
    ring = RS.roundabout_routes(40.0)[0]
    assert UR.is_closed(ring) and not UR.is_closed(L)
    side = 2 * 14.0 * np.sin(np.pi / 24)
    mid = 0.5 * (ring[22].astype(np.float64) + ring[23])
    x, y, seg, tseg, ev = _la(ring, np.float32(mid[0]), np.float32(mid[1]), 3.0 * side)
    assert (seg, tseg, ev) == (22, 1, UR.WRAPPED) and abs(np.hypot(x, y) - 14.0 * np.cos(np.pi / 24)) < 1e-5   # a side's midpoint again
    want = 0.5 * (ring[1].astype(np.float64) + ring[2])
    assert abs(x - want[0]) < 1e-5 and abs(y - want[1]) < 1e-5
    x, y, seg, tseg, ev = _la(ring, np.float32(mid[0]), np.float32(mid[1]), 0.25 * side)
    assert (seg, tseg, ev) == (22, 22, 0)
    x, y, seg, tseg, ev = _la(ring, np.float32(mid[0]), np.float32(mid[1]), 30 * side)
    assert (seg, tseg, ev) == (22, 21, UR.WRAPPED | UR.ROUTE_END) and (x, y) == (float(ring[22, 0]), float(ring[22, 1]))
    x, y, seg, tseg, ev = _la(ring, 14.0, 0.2, 30 * side)                                       # on segment 0: the whole lap, no seam
    assert (seg, tseg, ev) == (0, 23, UR.ROUTE_END) and (x, y) == (float(ring[0, 0]), float(ring[0, 1]))
    # the walk's length: along a straight route the point is d ahead of the projection
    for d in (0.5, 3.0, 17.25):
        x, y, _, _, ev = _la([(-50, 2), (-10, 2), (30, 2), (70, 2)], -20.5, 5, d)
        assert (x, y, ev) == (-20.5 + d, 2.0, 0)


# ---------------------------------------------------------------------------------------------------- header <-> Python
def test_header_layout_ffi_and_abi():
    from tactics2d_amd import _ffi, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {n: int(v) for n, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for body in re.findall(r"enum\s*\{(.*?)\};", header, re.S):
        vals.update({n: int(v) for n, v in re.findall(r"(T2D_\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))})
    assert vals["T2D_ABI_VERSION"] == 13 == L.ABI_VERSION
    assert vals["T2D_PROFILE_PURSUIT"] == 16 == L.PROFILE_PURSUIT and vals["T2D_PURSUIT_NONE"] == 255 == L.PURSUIT_NONE
    cols = ("MIN_PRE_AIMING", "INTERVAL_LAT", "KP", "ACCEL_CHANGE_RATE", "MAX_ACCEL", "MIN_ACCEL", "INTERVAL_LON", "DELTA_T", "LAT_MODE",
            "LON_MODE", "WHEEL_BASE", "LANE_HALF_WIDTH", "HORIZON", "COLS")
    for k, name in enumerate(cols):
        assert vals["T2D_PURSUIT_" + name] == k == getattr(L, "PURSUIT_" + name) == getattr(UR, name)
    for name in ("ROUTE_END", "NONFINITE", "WRAPPED", "NO_ROUTE", "NO_LEADER"):
        assert vals["T2D_PURSUIT_" + name] == getattr(L, "PURSUIT_" + name) == getattr(UR, name)
    assert (L.PURSUIT_LAT_NONE, L.PURSUIT_LAT_PURE_PURSUIT, L.PURSUIT_LON_CRUISE, L.PURSUIT_LON_ACC, L.PURSUIT_LON_CALLER) == (0, 1, 0, 1, 2)
    for name in ("t2d_set_pursuit", "t2d_pursuit_actions", "t2d_pursuit_buffers"):
        assert name in _ffi.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert len(_ffi.SYMBOLS["t2d_set_pursuit"][1]) == 6 and len(_ffi.SYMBOLS["t2d_pursuit_actions"][1]) == 5
    for name in ("t2d_pursuit_reset", "t2d_pursuit_state"):   # stateless: no such calls
        assert name not in _ffi.SYMBOLS and name not in header

    class Rec(ctypes.Structure):
        _fields_ = [("point", ctypes.c_double * 2), ("pre_aiming_distance", ctypes.c_double), ("distance", ctypes.c_double),
                    ("cross_track", ctypes.c_double), ("segment", ctypes.c_int32), ("target_segment", ctypes.c_int32),
                    ("leader", ctypes.c_int32), ("events", ctypes.c_uint32), ("action", ctypes.c_double * 2)]
    body = re.search(r"typedef struct t2d_pursuit_record \{(.*?)\} t2d_pursuit_record;", header, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[2\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in Rec._fields_]
    assert ctypes.sizeof(Rec) == 72 == L.PURSUIT_RECORD_BYTES and Rec.segment.offset == 40 and Rec.events.offset == 52
    assert Rec.action.offset == 56 and L.PURSUIT_RECORD_BYTES % 8 == 0
    from tactics2d_amd import build
    assert "t2d_pursuit.hip" in build.SOURCES


# ---------------------------------------------------------------------------------------------------- the closed loop
def test_closed_loop_bands_on_the_cpu(oracle):
    """pursuit_ref + the C oracle's kinematics, 8 x 16 cars on the two rings for 150 steps: the figures tests/test_gpu_pursuit.py
    holds the device to.  The reference law alone stays on the ring: no NO_ROUTE / NONFINITE / ROUTE_END event, every car within
    the OffRoute threshold throughout."""
    rows, cte, events, states = US.ring_rollout(oracle)
    sc, route_of, ts = PS.ring_scene()
    assert cte.shape == (US.RING_STEPS, 128) and np.isfinite(cte).all() and np.isfinite(rows).all()
    assert not (events & (UR.NO_ROUTE | UR.NONFINITE | UR.ROUTE_END | UR.NO_LEADER)).any() and (events & UR.WRAPPED).any()
    assert np.abs(cte).max() < PS.OFF_ROUTE_THRESHOLD
    for st in states[::10] + [states[-1]]:
        assert PS.ring_distance(st, route_of).max() < PS.OFF_ROUTE_THRESHOLD
    excess, signed, settled = US.ring_figures(cte)
    half = cte[US.RING_STEPS // 2:].mean(0)
    print("largest excess over the own start", excess, "largest |mean signed| of the second half", signed, "largest mean |offset|", settled,
          "signed means", half.min(), half.max(), "largest |steering|", np.abs(rows[:, :, 0]).max())
    assert abs(excess - US.RING_CPU_EXCESS) < 5e-4 and excess <= US.RING_MARGIN
    assert abs(signed - US.RING_CPU_SIGNED) < 5e-4 and abs(settled - US.RING_CPU_SETTLED) < 5e-4
    assert abs(half.min() - US.RING_CPU_INSIDE[0]) < 5e-4 and abs(half.max() - US.RING_CPU_INSIDE[1]) < 5e-4 and half.max() < 0   # inside
    assert US.RING_SIGNED == 1.5 * US.RING_CPU_SIGNED and US.RING_SETTLED == 1.5 * US.RING_CPU_SETTLED
    assert US.RING_CPU_SETTLED > PS.RING_CPU_SETTLED    # PID remains the tighter lane keeper
