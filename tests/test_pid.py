"""The lane-keeping PID controllers without a GPU: the numpy restatement (tests/pid_ref.py) and the host mirror
(tactics2d_amd.controller.PIDController) against tests/golden/pid.npz -- recorded by running the reference's own class,
tests/golden/make_pid.py -- the build-defined measurement on known answers, header <-> Python constants, and the closed-loop
bands that tests/test_gpu_pid.py holds the device to.

Measured here (teacher-forced, so nothing drifts): pid_ref equals the fixture BIT FOR BIT on all 2633 calls the device modes
express, outputs and state words, in all three lateral kinds -- the heading kind too, since both sides call numpy's sin / cos /
arctan2.  The asserted agreement is the issue's 1e-9 absolute, and exact equality where only + - * / and compares are involved.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import pid_ref as PR
import pid_scenes as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------------- the law
def test_ref_equals_the_fixture_teacher_forced():
    c = PS.fixture_calls()
    steer, accel, state, events, lat_err = PS.ref_on_calls(c)
    ok = ~c["raised"]
    assert len(ok) > 2500 and c["raised"].sum() > 10
    print("max |d steering|", np.abs(steer[ok] - c["out"][ok, 0]).max(), "max |d accel|", np.abs(accel[ok] - c["out"][ok, 1]).max(),
          "max |d state|", np.abs(state - c["after"]).max())
    assert np.abs(steer[ok] - c["out"][ok, 0]).max() <= 1e-9
    assert np.abs(accel[ok] - c["out"][ok, 1]).max() <= 1e-9
    assert np.abs(state - c["after"]).max() <= 1e-9          # (also where the reference raised: the state was updated first)
    exact = c["lat"] != 1                                        # cross-track and longitudinal: + - * / and compares only
    assert (steer[ok & exact] == c["out"][ok & exact, 0]).all() and (accel[ok] == c["out"][ok, 1]).all()
    assert (state[exact] == c["after"][exact]).all()
    # wheel_base <= 0: combined mode -> steering 0.0 with the lateral state updated; lateral mode -> the reference raised
    bad = (c["rows"][:, PR.WHEEL_BASE] <= 0) & (c["rows"][:, PR.LAT_MODE] == 2)
    assert (bad & (c["mode"] == 0)).sum() > 50 and (events[bad] & PR.BAD_WHEEL_BASE).all() and not (events[~bad] & PR.BAD_WHEEL_BASE).any()
    assert (steer[bad] == 0.0).all() and (c["out"][bad & (c["mode"] == 0), 0] == 0.0).all()
    assert (c["raised"] == (bad & (c["mode"] == 1))).all()
    assert (state[bad, :3] != c["before"][bad, :3]).any(1).all()


def test_ref_runs_the_sequences_on_its_own_state():
    """not teacher-forced: forty calls on the restatement's own state, reset() included"""
    f = PS.fixture()
    n_seq, n_call = f["q_th"].shape
    qp = f["q_params"].copy()
    styled = ~np.isnan(f["q_style"])
    for col, k in zip((1, 5, 4, 8, 9), range(5)):
        qp[styled, col] = f["q_styled"][styled, k]
    keep = (f["q_lat"] != 3) | (f["q_mode"] == 2)
    state = np.zeros((n_seq, 6))
    worst = 0.0
    for k in range(n_call):
        state[f["q_reset"] == k] = 0.0
        inp = f["q_in"][:, k]
        R = PS.fixture_rows(qp, f["q_mode"].astype(int), f["q_lat"].astype(int), inp[:, 6])
        steer, accel, state, _, _ = PR.law(R, state, inp[:, 0], inp[:, 1], inp[:, 2], np.ones(n_seq, bool), inp[:, 3], f["q_th"][:, k],
                                           np.full(n_seq, np.nan), np.zeros(n_seq))
        worst = max(worst, np.abs(np.stack([steer, accel], 1) - f["q_out"][:, k])[keep].max(), np.abs(state - f["q_after"][:, k])[keep].max())
    print("worst deviation over the sequences", worst)
    assert worst <= 1e-9


def test_the_fixture_reaches_what_the_issue_lists():
    f = PS.fixture()
    c = PS.fixture_calls()
    _, _, _, events, _ = PS.ref_on_calls(c)
    seq = slice(len(f["s_mode"]) - int(((f["s_lat"] == 3) & (f["s_mode"] != 2)).sum()), None)
    lon = c["rows"][seq, PR.LON_MODE] == 1
    sat = (events[seq] & PR.SATURATED) != 0
    out = c["out"][seq, 1]
    assert (sat & lon & (out == c["rows"][seq, PR.MAX_ACCEL])).any() and (sat & lon & (out == c["rows"][seq, PR.MIN_ACCEL])).any()
    assert (sat & (c["before"][seq, 3] != 0) & (c["after"][seq, 3] == c["before"][seq, 3] * 0.99)).any()      # the leaky branch
    at_limit = (out == c["rows"][seq, PR.MAX_ACCEL]) | (out == c["rows"][seq, PR.MIN_ACCEL])
    assert (~sat & lon & at_limit).any()                                                                         # the final clip alone
    assert set(f["q_mode"]) == {0, 1, 2} and (f["q_reset"] > 0).any()
    styles = f["q_style"][~np.isnan(f["q_style"])]
    assert len(set(styles)) >= 3 and (np.abs(styles) > 1).any()
    assert ((f["q_in"][:, :, 6] <= 0).all(1) & (f["q_mode"] == 0)).any()
    assert os.path.getsize(PS.GOLDEN) < 600 * 1024


# ---------------------------------------------------------------------------------------------------- the host mirror
class _State:
    def __init__(self, heading, speed):
        self.heading, self.speed = heading, speed


def _mirror_call(c, lat, inp, th):
    kw = dict(target_speed=float(inp[2]), wheel_base=float(inp[6]))
    if lat in (1, 3):
        kw["target_heading"] = float(th)
    if lat in (2, 3):
        kw["cross_track_error"] = float(inp[3])
    return c.step(_State(float(inp[0]), float(inp[1])), **kw)


def test_mirror_step_equals_the_fixture():
    from tactics2d_amd.controller import PIDController
    f = PS.fixture()
    modes = ("combined", "lateral", "longitudinal")
    worst = 0.0
    for i in range(0, len(f["s_mode"]), 3):   # (every third single call, every kind among them)
        c = PIDController(f["s_params"][i, 0], modes[f["s_mode"][i]], *f["s_params"][i, 1:])
        c.state = f["s_state"][i]
        if f["s_raised"][i]:
            with pytest.raises(ValueError):
                _mirror_call(c, f["s_lat"][i], f["s_in"][i], f["s_th"][i])
        else:
            out = _mirror_call(c, f["s_lat"][i], f["s_in"][i], f["s_th"][i])
            worst = max(worst, np.abs(np.float64(out) - f["s_out"][i]).max())
        worst = max(worst, np.abs(c.state - f["s_after"][i]).max())
    for s in range(len(f["q_mode"])):
        c = PIDController(f["q_params"][s, 0], modes[f["q_mode"][s]], *f["q_params"][s, 1:])
        if not np.isnan(f["q_style"][s]):
            c.update_driving_style(float(f["q_style"][s]))
            got = np.float64([c.kp_lat, c.kp_lon, c.max_steering, c.max_accel, c.min_accel])
            assert (got == f["q_styled"][s]).all(), (s, got, f["q_styled"][s])
        for k in range(f["q_th"].shape[1]):
            if k == f["q_reset"][s]:
                c.reset()
            out = _mirror_call(c, f["q_lat"][s], f["q_in"][s, k], f["q_th"][s, k])
            worst = max(worst, np.abs(np.float64(out) - f["q_out"][s, k]).max(), np.abs(c.state - f["q_after"][s, k]).max())
    print("worst deviation of the mirror", worst)
    assert worst <= 1e-9


def test_mirror_refuses_what_the_reference_refuses():
    from tactics2d_amd.controller import PIDController
    f = PS.fixture()
    errors = {"": None, "ValueError": ValueError, "AttributeError": AttributeError, "TypeError": TypeError}
    assert "ValueError" in set(f["r_ctor"]) and "AttributeError" in set(f["r_configure"]) and "" in set(f["r_ctor"])
    for kw, ctor, conf in zip(f["r_kwargs"], f["r_ctor"], f["r_configure"]):
        for want, call in ((str(ctor), lambda: PIDController(**kw)), (str(conf), lambda: PIDController().configure(**kw))):
            if errors[want] is None:
                call()
            else:
                with pytest.raises(errors[want]):
                    call()
    with pytest.raises(TypeError):
        PIDController().update_driving_style("brisk")
    c = PIDController(control_mode="lateral", lateral="heading", wheel_base=2.5)
    r = c.row()
    assert r[PR.LAT_MODE] == 1 and r[PR.LON_MODE] == 0 and r[PR.WHEEL_BASE] == 2.5 and np.isnan(PIDController().row()[PR.WHEEL_BASE])
    assert PIDController(longitudinal="idm").modes() == (2, 2) and PIDController(control_mode="longitudinal").modes() == (0, 1)
    assert (PIDController().row()[:11] == [0.05, 1.5, 0.2, 0.5, 0.5, 2.0, 0.3, 0.4, 3.0, -5.0, 0.1]).all()


# ---------------------------------------------------------------------------------------------------- the measurement
def _measure_one(route, px, py):
    import route_ref as RR
    VX, VY, nv = RR.pad_routes([np.float32(route)], np.array([0]))
    m, cte, th, seg, end = PR.measure(VX, VY, nv, np.float32([px]), np.float32([py]))
    return bool(m[0]), float(cte[0]), float(th[0]), int(seg[0]), bool(end[0])


def test_measurement_known_answers():
    L = [(0, 0), (8, 0), (8, 4)]   # east, then north
    assert _measure_one(L, 4, 0) == (True, 0.0, 0.0, 0, False)                      # on the route
    assert _measure_one(L, 4, -2) == (True, 2.0, 0.0, 0, False)                     # the route lies to the left: positive
    assert _measure_one(L, 4, 1) == (True, -1.0, 0.0, 0, False)                     # to the right: negative
    assert _measure_one(L, -3, 4)[:4] == (True, -5.0, 0.0, 0) and not _measure_one(L, -3, 4)[4]   # before the first vertex
    m, cte, th, seg, end = _measure_one(L, 11, 8)                                   # beyond the last vertex
    assert (m, cte, seg, end) == (True, 5.0, 1, True) and th == np.arctan2(4.0, 0.0)
    assert _measure_one(L, 8, 4) == (True, 0.0, np.arctan2(4.0, 0.0), 1, True)      # on the last vertex
    # zero-length segments are skipped: inside a route they change nothing but the index, a whole route of them is no route
    assert _measure_one([(0, 0), (4, 0), (4, 0), (4, 4)], 6, 1) == (True, 2.0, np.arctan2(4.0, 0.0), 2, False)
    assert _measure_one([(0, 0), (4, 0), (4, 0), (4, 4)], 6, 0) == (True, 0.0, 0.0, 0, False)   # collinear beyond a segment: c = 0
    assert _measure_one([(1, 1), (1, 1), (5, 1)], 1, 4) == (True, -3.0, 0.0, 1, False)
    assert _measure_one([(0, 0), (4, 0), (4, 4), (4, 4)], 4, 6)[3:] == (1, True)    # (the last NON-degenerate segment ends the route)
    assert _measure_one([(2, 2), (2, 2)], 0, 0)[0] is False and _measure_one([(2, 2), (2, 2), (2, 2)], 0, 0)[3] == -1
    # the distance is t2d_off_route's, bit for bit
    import route_ref as RR
    for k, (route, px, py, thr) in enumerate(RR.random_cases(300, seed=11)):
        d, _, seg = RR.distance(route, px, py, thr)
        m, cte, _, s2, _ = _measure_one(route, px, py)
        d64 = np.sqrt(min(RR.seg_d2(*np.float64(route[j]), *np.float64(route[j + 1]), np.float64(px), np.float64(py))
                          for j in range(len(route) - 1)))
        assert m and abs(cte) == d64 and np.float32(abs(cte)) == d
        assert s2 == seg or (route[seg] == route[seg + 1]).all()


# ---------------------------------------------------------------------------------------------------- header <-> Python
def test_header_layout_ffi_and_abi():
    from tactics2d_amd import _ffi, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {n: int(v) for n, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for body in re.findall(r"enum\s*\{(.*?)\};", header, re.S):
        vals.update({n: int(v) for n, v in re.findall(r"(T2D_\w+)\s*=\s*(\d+)", re.sub(r"/\*.*?\*/", "", body, flags=re.S))})
    assert vals["T2D_ABI_VERSION"] == 13 == L.ABI_VERSION
    assert vals["T2D_PROFILE_PID"] == 15 == L.PROFILE_PID and vals["T2D_PID_NONE"] == 255 == L.PID_NONE
    cols = ("DT", "KP_LAT", "KI_LAT", "KD_LAT", "MAX_STEERING", "KP_LON", "KI_LON", "KD_LON", "MAX_ACCEL", "MIN_ACCEL", "ALPHA",
            "LAT_MODE", "LON_MODE", "WHEEL_BASE", "COLS")
    for k, name in enumerate(cols):
        assert vals["T2D_PID_" + name] == k == getattr(L, "PID_" + name)
        assert name == "COLS" or getattr(PR, name) == k
    assert vals["T2D_PID_STATE_WORDS"] == 6 == L.PID_STATE_WORDS
    for name in ("ROUTE_END", "NONFINITE", "RESET", "NO_ROUTE", "BAD_WHEEL_BASE", "SATURATED"):
        assert vals["T2D_PID_" + name] == getattr(L, "PID_" + name) == getattr(PR, name)
    for name in ("t2d_set_pid", "t2d_pid_actions", "t2d_pid_reset", "t2d_pid_state", "t2d_pid_buffers"):
        assert name in _ffi.SYMBOLS and re.search(r"\bint\s+" + name + r"\s*\(", header)
    assert len(_ffi.SYMBOLS["t2d_set_pid"][1]) == 7 and len(_ffi.SYMBOLS["t2d_pid_actions"][1]) == 5
    # the record: 48 bytes, the fields where pool.pid_records() looks for them
    class Rec(ctypes.Structure):
        _fields_ = [("cross_track", ctypes.c_double), ("lat_error", ctypes.c_double), ("segment", ctypes.c_int32),
                    ("leader", ctypes.c_int32), ("events", ctypes.c_uint32), ("reserved", ctypes.c_uint32), ("action", ctypes.c_double * 2)]
    body = re.search(r"typedef struct t2d_pid_record \{(.*?)\} t2d_pid_record;", header, re.S).group(1)
    assert re.findall(r"(\w+)(?:\[2\])?;", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) == [n for n, _ in Rec._fields_]
    assert ctypes.sizeof(Rec) == 48 == L.PID_RECORD_BYTES and Rec.segment.offset == 16 and Rec.action.offset == 32


# ---------------------------------------------------------------------------------------------------- the closed loop
def test_closed_loop_bands_on_the_cpu(oracle):
    """pid_ref + the C oracle's kinematics, 8 x 16 cars on the two rings for 150 steps: the figures tests/test_gpu_pid.py tabulates"""
    rows, cte, states = PS.ring_rollout(oracle)
    sc, route_of, ts = PS.ring_scene()
    a = np.abs(cte)
    assert a.shape == (PS.RING_STEPS, 128) and np.isfinite(a).all()
    excess, settled = (a.max(0) - a[0]).max(), a[PS.RING_STEPS // 2:].mean(0).max()
    print("start: largest |error|", a[0].max(), "largest excess over the own start", excess, "settled (largest mean of the second half)",
          settled, "saturated steering share", (np.abs(rows[:, :, 0]) >= 0.5).mean())
    assert a[0].max() <= 0.65                                   # 0.5 m off the circle, measured to a polygon
    assert abs(excess - PS.RING_CPU_EXCESS) < 5e-4 and excess <= PS.RING_MARGIN
    assert abs(settled - PS.RING_CPU_SETTLED) < 5e-4 and PS.RING_SETTLED == 1.5 * PS.RING_CPU_SETTLED
    assert PS.ring_distance(states[-1], route_of).max() < 0.2
    # what the feature exists to change: the same start with steering 0.0 leaves the ring, every vehicle
    _, _, straight = PS.ring_rollout(oracle, steer=False)
    assert PS.ring_distance(straight[-1], route_of).min() > PS.OFF_ROUTE_THRESHOLD
