"""verify_states (physics_model_base.py:53-73) and device-resident trajectories, the parts that need no GPU: the fixture made by
running the reference (tests/golden/make_verify_states.py) and what it means, the host interval rule, the shared frame
bookkeeping of DeviceTrajectory, and the C ABI's declarations."""
import os
import re
import subprocess
import sys
import warnings

import numpy as np
import pytest

import helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("TACTICS2D_REFERENCE", "/root/reference")


def _cases():
    return H.load_npz("verify_states.npz")


def _traj(g, t):
    lo, hi = int(g["offsets"][t]), int(g["offsets"][t + 1])
    return g["stamp"][lo:hi], g["state"][lo:hi], g["interval"][lo:hi]


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "tactics2d")), reason="the reference tree is not present")
def test_generator_reproduces_the_fixture_bit_for_bit(tmp_path):
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_verify_states.py"), "--ref", REF,
                    "--out", str(tmp_path)], check=True, capture_output=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    with open(tmp_path / "verify_states.npz", "rb") as a, open(os.path.join(H.GOLD, "verify_states.npz"), "rb") as b:
        assert a.read() == b.read()


def test_fixture_covers_what_it_claims():
    g = _cases()
    assert len(g["valid"]) >= 2000 and 0.35 < g["valid"].mean() < 0.65
    assert sorted(set(g["type_id"].tolist())) == list(range(12))
    n = np.diff(g["offsets"])
    assert n.min() == 1 and n.max() <= 41 and (g["margin"] >= 1e-7).all()
    fps = g["fps"][g["stable"] == 1]
    assert {10.0, 20.0, 30.0, 7.0} <= set(fps.tolist())
    assert not g["valid"][g["kind"] == 5].any()       # stepped by the model itself: fails against frame 0
    assert g["valid"][g["kind"] == 6].any()           # jumps within one interval of frame 0: can pass
    assert g["valid"][g["kind"] == 4].all()           # one frame
    dup = [t for t in range(len(n)) if len(set(_traj(g, t)[0].tolist())) < n[t]]
    assert len(dup) > 100


def test_oracle_composition_against_frame_0_equals_the_reference_verdict(oracle):
    """verify_state frame by frame against FRAME 0 (the reference never advances last_state), AND-ed: the fixture's verdict,
    wherever every interval is an integer (what t2do_verify_state takes)"""
    g = _cases()
    rows = g["rows"]
    checked = 0
    for trig in (0, 1):
        for t in range(len(g["valid"])):
            stamps, st, iv = _traj(g, t)
            if not np.array_equal(iv, np.round(iv)):
                continue
            by = {int(f): k for k, f in enumerate(stamps)}          # (a repeated stamp resolves to its last state)
            last = st[by[int(stamps[0])]][None].astype(np.float64)
            ok = True
            for f, i in zip(stamps[1:], iv[1:]):
                cand = st[by[int(f)]][None, :4].astype(np.float64)
                ok &= bool(oracle.verify_state(rows, [int(g["type_id"][t])], last, cand, int(i), trig=trig)[0])
            assert ok == bool(g["valid"][t]), (trig, t)
            checked += 1
    assert checked > 2 * 1200


def _replay_reference_trajectory(g, t, cls=None):
    from tactics2d_amd.history import BatchedTrajectory
    from tactics2d_amd.physics import BatchedState
    stamps, st, _ = _traj(g, t)
    fps = None if np.isnan(g["fps"][t]) else int(g["fps"][t])
    tr = (cls or BatchedTrajectory)(id_=0, fps=fps, stable_freq=bool(g["kind"][t] != 7))   # (kind 7: stable_freq=False given)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for f, s in zip(stamps, st):
            tr.add_state(BatchedState(int(f), [s[0]], [s[1]], [s[2]], [s[4]], [s[5]], speed=[s[3]]))
    return tr


def test_host_interval_rule_reproduces_the_reference_intervals():
    from tactics2d_amd.history import BatchedTrajectory, verify_intervals
    g = _cases()
    for t in range(len(g["valid"])):
        tr = _replay_reference_trajectory(g, t)
        assert bool(tr.stable_freq) == bool(g["stable"][t]), t
        got = verify_intervals(tr)
        want = _traj(g, t)[2][1:]
        assert len(got) == len(want) and all(np.float64(a) == b for a, b in zip(got, want)), (t, got, want)
        assert all(isinstance(a, float) for a in got) if tr.stable_freq else all(isinstance(a, (int, np.integer)) for a in got)
    with pytest.raises(TypeError):   # 1000 / None
        verify_intervals(BatchedTrajectory(id_=0))
    with pytest.raises(IndexError):  # frames[0] of an empty trajectory
        verify_intervals(BatchedTrajectory(id_=0, fps=10))
    with pytest.raises(IndexError):
        verify_intervals(BatchedTrajectory(id_=0, stable_freq=False))


class HostSlots:
    """numpy stand-in of DeviceTrajectory's device buffer (same interface as history._TrajBuffer)"""

    def __init__(self, n, capacity):
        self.n, self.capacity = n, capacity
        self.data = np.full((6, capacity, n), np.nan, np.float32)
        self.grows = 0

    def write(self, slot, cols):
        assert 0 <= slot < self.capacity
        self.data[:, slot] = cols

    def read(self, slot):
        assert 0 <= slot < self.capacity
        return self.data[:, slot].copy()

    def rows(self, col, n_rows):
        return self.data[col, :n_rows].copy()

    def grown(self, capacity, n_slots, stream=None):
        new = HostSlots(self.n, capacity)
        new.data[:, :n_slots] = self.data[:, :n_slots]
        new.grows = self.grows + 1
        return new

    def close(self):
        pass


def replay_trajectory_kats(make):
    """tests/golden/trajectory_kats.json on the trajectory `make()` returns -- the checks of
    test_host.py::test_batched_trajectory_replays_the_reference_operation_by_operation"""
    from tactics2d_amd.physics import BatchedState
    seqs = H.load_json("trajectory_kats.json")
    n_ops = 0
    mk = lambda frame, x, y, speed: BatchedState(frame=frame, x=[x, x + 1.0], y=[y, y - 1.0], heading=[0.0, 0.0], speed=[speed, 2.0 * speed])
    for si, seq in enumerate(seqs):
        t = make()
        for oi, rec in enumerate(seq):
            op = rec["op"]; kind = op[0]; got = None; raised = None
            try:
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    if kind == "add":
                        t.add_state(mk(*op[1:]))
                    elif kind == "add_bad":
                        t.add_state("not a state")
                    elif kind == "get":
                        s = t.get_state(op[1])
                        got = None if s is None else dict(frame=s.frame, speed=float(s.speed[0]), x=float(s.x[0]))
                    elif kind == "has":
                        got = bool(t.has_state(op[1]))
                    elif kind == "trace":
                        tr = t.get_trace(None if op[1] is None else tuple(op[1]))
                        got = [[float(p[0][0]), float(p[1][0])] for p in tr]
                    elif kind == "reset":
                        t.reset(None if op[1] is None else mk(*op[1]), keep_history=op[2])
            except Exception as exc:   # noqa: BLE001 -- compared by type below
                raised = type(exc).__name__
            where = (si, oi, op)
            assert raised == rec.get("raises"), (where, raised, rec.get("raises"))
            if raised is None and kind in ("get", "has", "trace"):
                want = rec["result"]
                if kind == "get" and want is not None:
                    assert got["frame"] == want["frame"] and got["speed"] == np.float32(want["speed"]) and got["x"] == np.float32(want["x"]), (where, got, want)
                elif kind == "trace":
                    assert np.allclose(got, want, rtol=1e-6, atol=0) if want else got == [], (where, got, want)
                else:
                    assert got == want, (where, got, want)
            a = rec["after"]
            cur = t.get_state()
            assert list(t.frames) == a["frames"] and len(t) == a["n"] and bool(t.stable_freq) == a["stable_freq"], (where, list(t.frames), a)
            assert t.first_frame == a["first_frame"] and t.last_frame == a["last_frame"], where
            assert (None if cur is None else cur.frame) == a["current_frame"], (where, a)
            assert (None if t.initial_state is None else t.initial_state.frame) == a["initial_frame"], where
            assert (None if t.last_state is None else t.last_state.frame) == a["last_state_frame"], where
            if a["average_speed"] is not None and len(t):
                assert np.allclose(np.asarray(t.average_speed)[0], a["average_speed"], rtol=1e-6), (where, t.average_speed, a["average_speed"])
            n_ops += 1
    assert n_ops == 457


def test_device_trajectory_bookkeeping_answers_the_reference_kats_without_a_gpu():
    """DeviceTrajectory's frame -> slot bookkeeping (the pure-Python part, on a host stand-in of its buffer, capacity 2 so that it
    grows) answers tests/golden/trajectory_kats.json as BatchedTrajectory does"""
    from tactics2d_amd.history import DeviceTrajectory
    made = []

    def make():
        t = DeviceTrajectory(None, 3, _storage=HostSlots(2, 2))
        made.append(t)
        return t
    replay_trajectory_kats(make)
    assert max(t._buf.grows for t in made) >= 2
    for t in made:   # every referenced slot lies in the slots in use, and holds its frame
        assert all(0 <= s < t._n_used <= t.capacity for s in t._book.by_frame.values())


def test_device_trajectory_reuses_slots_as_documented():
    from tactics2d_amd.history import DeviceTrajectory
    from tactics2d_amd.physics import BatchedState
    t = DeviceTrajectory(None, 0, fps=10, _storage=HostSlots(3, 4))
    st = lambda f, x: BatchedState(f, [x] * 3, [0.0] * 3, [0.0] * 3, speed=[1.0] * 3)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for k in range(3):
            t.add_state(st(100 * k, float(k)))
        assert list(t.slots()) == [0, 1, 2]
        t.add_state(st(200, 9.0))                     # repeated frame: its slot again
        assert list(t.slots()) == [0, 1, 2, 2] and t._n_used == 3 and t.get_state(200).x[0] == 9.0
        with pytest.raises(KeyError):                 # early frame: overwritten, then raises
            t.add_state(st(100, 7.0))
        assert t.get_state(100).x[0] == 7.0 and t.get_state().frame == 200
        t.reset()                                     # history dropped: the initial state moves to slot 0
        assert list(t.slots()) == [0] and t._n_used == 1 and t.get_state().x[0] == 0.0
        for k in range(1, 6):                         # past capacity 4: grows to 8, contents intact
            t.add_state(st(100 * k, float(k)))
        assert t.capacity == 8 and [float(t.get_state(100 * k).x[0]) for k in range(6)] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]
        with pytest.raises(ValueError):
            t.add_state(BatchedState(700, [0.0] * 2))  # a batch of another size


def test_abi_declares_and_types_the_trajectory_calls():
    from tactics2d_amd import _ffi, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    names = ["t2d_traj_create", "t2d_traj_destroy", "t2d_traj_record", "t2d_traj_write", "t2d_traj_read", "t2d_traj_column",
             "t2d_traj_copy", "t2d_verify_states"]
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for n in names:
        assert re.search(r"\bint\s+" + n + r"\s*\(", text), n
        assert n in _ffi.SYMBOLS, n
    assert int(re.search(r"#define\s+T2D_ABI_VERSION\s+(\d+)", header).group(1)) == L.ABI_VERSION == 13
    assert int(re.search(r"#define\s+T2D_TRAJ_COLS\s+(\d+)", header).group(1)) == L.TRAJ_COLS
    assert len(_ffi.SYMBOLS["t2d_verify_states"][1]) == 6 and len(_ffi.SYMBOLS["t2d_traj_copy"][1]) == 4
