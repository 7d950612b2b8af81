"""Replayed participants, host side: `history.ReplaySource` answers `is_active` / `get_state(frame)` as the reference's
ParticipantBase does (participant/element/participant_base.py:166-203; tests/golden/replay.npz holds what the reference itself
answered, tests/golden/make_replay.py made it), the C header, the ctypes table and layout.py agree on the new names, and the
grid checks that need no device refuse what the device could not express."""
import os
import re

import numpy as np
import pytest

import helpers as H
from tactics2d_amd import _ffi, layout as L
from tactics2d_amd.history import BatchedTrajectory, ReplaySource
from tactics2d_amd.physics import BatchedState

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ("inside", "first", "last", "before", "after", "off_grid", "one_frame", "empty")


def _golden_source():
    g = H.load_npz("replay.npz")
    period = int(np.asarray(g["period"]).reshape(-1)[0])
    trajs = []
    for t in range(len(g["offsets"]) - 1):
        tr = BatchedTrajectory(t, fps=1000 / period)
        for k in range(g["offsets"][t], g["offsets"][t + 1]):
            x, y, h, v, vx, vy = g["state"][k]
            tr.add_state(BatchedState(int(g["stamp"][k]), x, y, h, vx, vy, speed=v))
        trajs.append(tr)
    return g, ReplaySource.from_trajectories(None, [trajs], 0, period)


def test_replay_source_answers_every_query_as_the_reference_does():
    g, src = _golden_source()
    counts = np.bincount(g["q_kind"], minlength=len(KINDS))
    assert len(counts) == len(KINDS) and (counts >= 20).all(), dict(zip(KINDS, counts))
    n_true = n_state = 0
    for q in range(len(g["q_traj"])):
        t, frame = int(g["q_traj"][q]), int(g["q_frame"][q])
        what = (KINDS[g["q_kind"][q]], t, frame)
        try:
            got, exc = int(bool(src.is_active(t, frame))), ""
        except Exception as e:
            got, exc = -1, type(e).__name__
        assert (got, exc) == (int(g["q_active"][q]), str(g["q_active_exc"][q])), what
        n_true += got == 1
        try:
            s = src.get_state(t, frame)
            st, exc = np.array([s.x[0], s.y[0], s.heading[0], s.speed[0], s.vx[0], s.vy[0]], np.float32), ""
            assert s.frame == frame
        except Exception as e:
            st, exc = None, type(e).__name__
        assert exc == str(g["q_state_exc"][q]), what
        if st is not None:
            assert st.tobytes() == g["q_state"][q].tobytes(), what
            n_state += 1
    # the fixture is not one-sided: active and inactive verdicts, states and both exceptions all occur
    assert n_true >= 100 and n_state >= 100
    assert (g["q_active"] == 0).sum() >= 100 and (g["q_active_exc"] == "TypeError").sum() >= 20
    assert (g["q_state_exc"] == "KeyError").sum() >= 100
    # the reference's quirk the fixture pins: off the grid but inside the window a participant IS active and has no state
    off = g["q_kind"] == KINDS.index("off_grid")
    assert (g["q_active"][off] == 1).all() and (g["q_state_exc"][off] == "KeyError").all()


def test_replay_source_windows_follow_the_trajectories():
    g, src = _golden_source()
    n = len(g["offsets"]) - 1
    assert src.n == n and src.n_src_env == 1
    for t in range(n):
        st = g["stamp"][g["offsets"][t]:g["offsets"][t + 1]]
        p = src.participant(t)
        if len(st) == 0:
            assert src.first_slot[t] > src.last_slot[t] and p.first_frame is None and p.last_frame is None
        else:
            assert (p.first_frame, p.last_frame) == (int(st[0]), int(st[-1]))
    # active_mask is the same rule for a whole env at once (what get_active_participants(frame) uses)
    for frame in (0, 40, 400, 1000, 4000):
        want = [len(st) > 0 and st[0] <= frame <= st[-1]
                for st in (g["stamp"][g["offsets"][t]:g["offsets"][t + 1]] for t in range(n))]
        assert src.active_mask(frame).reshape(-1).tolist() == want


def test_from_trajectories_raises_the_references_key_error_for_a_missing_stamp():
    tr = BatchedTrajectory(7)
    for f in (80, 120, 200):   # 160 is missing inside [80, 200]
        tr.add_state(BatchedState(f, 1.0, 2.0, 0.0, 0.0, 0.0, speed=0.0))
    with pytest.raises(KeyError, match="160"):
        ReplaySource.from_trajectories(None, [[tr]], 0, 40)
    with pytest.raises(ValueError, match="off the grid"):   # a window edge between two stamps
        ReplaySource.from_trajectories(None, [[tr]], 0, 60)
    with pytest.raises(ValueError, match="same number"):
        ReplaySource.from_trajectories(None, [[tr], [tr, tr]], 0, 40)


def test_grid_checks_that_need_no_device():
    st = np.zeros((4, 1, 2, 6), np.float32)
    with pytest.raises(ValueError, match="period_ms"):
        ReplaySource.from_arrays(None, st, t0_ms=0, period_ms=0)
    with pytest.raises(ValueError, match="not a multiple"):
        ReplaySource.from_arrays(None, st, t0_ms=30, period_ms=40)
    with pytest.raises(ValueError, match="outside"):
        ReplaySource.from_arrays(None, st, [0, 4], [3, 3], 0, 40)
    with pytest.raises(ValueError, match="outside"):
        ReplaySource.from_arrays(None, st, [0, 0], [3, -1], 0, 40)
    with pytest.raises(ValueError, match="windows of"):
        ReplaySource.from_arrays(None, st, [0], [3], 0, 40)
    with pytest.raises(ValueError, match="n_slots, n_src_env"):
        ReplaySource.from_arrays(None, st[0], t0_ms=0, period_ms=40)
    src = ReplaySource.from_arrays(None, st, [0, 2], [3, 1], 80, 40)   # first > last is legal: never present
    assert src.active_mask(80).tolist() == [[True, False]] and src.active_mask(40).tolist() == [[False, False]]
    assert src.slot_of([0, 79, 80, 119, 120]).tolist() == [-1, -1, 0, 0, 1]
    with pytest.raises(ValueError, match="upload"):
        src.device_buffer()


def test_header_ffi_and_layout_agree_on_replay():
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    assert re.search(r"#define\s+T2D_MODEL_REPLAY\s+5\b", header) and L.MODEL_REPLAY == 5
    assert re.search(r"#define\s+T2D_ABI_VERSION\s+13\b", header) and L.ABI_VERSION == 13
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name, n_args in (("t2d_replay_bind", 9), ("t2d_replay_apply", 2)):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)", text)
        assert m and len(m.group(1).split(",")) == n_args, name
        assert name in _ffi.SYMBOLS and len(_ffi.SYMBOLS[name][1]) == n_args
    from tactics2d_amd.pool import ParticipantPool
    for meth in ("replay_bind", "replay_apply", "replay_unbind"):
        assert callable(getattr(ParticipantPool, meth))


def test_replayed_rows_carry_shape_and_model_only():
    from tactics2d_amd import participant as P
    for name, shape, dims in (("medium_car", L.SHAPE_OBB, P.VEHICLE_TEMPLATE["medium_car"][:2]),
                              ("moped", L.SHAPE_OBB, P.CYCLIST_TEMPLATE["moped"][:2]),
                              ("adult_male", L.SHAPE_CIRCLE, P.PEDESTRIAN_TEMPLATE["adult_male"][:2])):
        r = P.replayed_row(name)
        assert r.shape == (L.PARAM_COLS,) and r[L.P_MODEL] == L.MODEL_REPLAY and r[L.P_SHAPE] == shape
        assert (r[L.P_LENGTH], r[L.P_WIDTH]) == dims
        assert r[L.P_RANGE_FLAGS] == 0 and r[L.P_MASS] == 0
    with pytest.raises(KeyError):
        P.replayed_row("hovercraft")
