"""The Reeds-Shepp path follower on the CPU: the specification (tests/rs_follow_ref.py) against the fixture made by executing
the tutorial's cells (tests/golden/rs_follow.npz), and the new names in the symbol table, the header and layout.py.  (The kernel
against both: tests/test_gpu_rs_follow.py.)"""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import rs_follow_cases as S
import rs_follow_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("TACTICS2D_REFERENCE", "/root/reference")


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "docs", "tutorial", "train_parking_demo.ipynb")),
                    reason="the reference tree is not present")
def test_generator_reproduces_the_fixture_byte_for_byte(tmp_path):
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_rs_follow.py"), "--ref", REF, "--out", str(tmp_path)],
                   check=True, capture_output=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    with open(tmp_path / "rs_follow.npz", "rb") as a, open(os.path.join(H.GOLD, "rs_follow.npz"), "rb") as b:
        assert a.read() == b.read()


def test_fixture_covers_what_it_claims():
    g = S.fixture()
    assert os.path.getsize(os.path.join(H.GOLD, "rs_follow.npz")) < 800 * 1024
    ev = g["events"]
    assert int(g["off"][S.N_LOOPS]) == 5529 and len(g["off"]) - 1 == S.N_LOOPS + 15
    for bit in (F.EV_POP_REACHED, F.EV_POP_RISING, F.EV_RESET):
        assert (ev & bit != 0).sum() >= 3, bit
    first = g["off"][S.N_LOOPS:-1]
    assert sum(ev[k] == F.EV_ADOPTED | F.EV_POP_REACHED for k in first) >= 3      # a first segment shorter than the reach radius
    assert (g["gains"] == 1).sum() >= 3 and g["head"].max() == 4
    pairs = {(int(s), int(np.sign(d))) for q in range(S.N_LOOPS) for s, d in zip(*S.plan_of(g, int(g["plan"][g["off"][q]])))}
    assert pairs == {(s, d) for s in (1, 0, -1) for d in (1, -1)}
    assert all(ev[g["off"][q + 1] - 1] & F.EV_FINISHED for q in range(S.N_LOOPS))


def test_specification_reproduces_every_call_and_has_no_knife_edge():
    g = S.fixture()
    worst, margin = 0.0, np.inf
    for q in range(len(g["off"]) - 1):
        f = F.Follower(S.params(g, int(g["gains"][q])))
        for k in S.sequence(g, q):
            r = f.call(g["state"][k], bool(g["ended"][k]), True, S.plan_of(g, int(g["plan"][k])), (0.25, -0.5))
            assert (r.executing, r.segment, r.events) == (g["left"][k], g["head"][k], g["events"][k]), (q, k, r)
            margin = min(margin, F.margin(r))
            if np.isnan(g["action"][k, 0]):   # the agent did not act: the policy's row, bit for bit
                assert np.isnan(r.action[0]) and r.row.tobytes() == np.float32([0.25, -0.5]).tobytes(), (q, k)
                continue
            worst = max(worst, np.abs(np.array(r.action) - g["action"][k]).max())
            assert r.row.tobytes() == g["row"][k].tobytes(), (q, k, r.row, g["row"][k])
    print("largest action deviation", worst, "smallest decision margin", margin)
    assert worst <= 1e-12 and margin >= 1e-7


def test_wrapper_stage_is_bit_exact():
    g = S.fixture()
    acted = ~np.isnan(g["action"][:, 0])
    got = np.array([F.wrap_action(a) for a in g["action"][acted]])
    assert got.dtype == np.float32 and got.tobytes() == g["row"][acted].tobytes()
    assert F.wrap_action((3.0, -7.0)).tolist() == [np.float32(0.524), -2.0]


def test_build_defined_rows_of_the_specification():
    g = S.fixture()
    plan = S.plan_of(g, int(g["plan"][0]))
    f = F.Follower(S.params(g))
    assert f.call(g["state"][0], active=False, plan=plan).events == 0 and not f.left          # (b) an inactive ego does not adopt
    assert f.call(g["state"][0], plan=plan).events == F.EV_ADOPTED
    r = f.call([np.nan, 0, 0, 0], policy_row=(0.1, 0.2))
    assert r.events == F.EV_DROPPED and r.executing == 0 and r.row.tolist() == [np.float32(0.1), np.float32(0.2)]
    f = F.Follower(S.params(g))   # the zero-length S segment as the head: 0 / 0, dropped, the controllers untouched
    r = f.call([0.0, 0.0, 0.0, 0.0], plan=([1, 0], [0.01, 0.0]))
    assert r.events == F.EV_ADOPTED | F.EV_POP_REACHED | F.EV_DROPPED and np.isnan(r.action[0]) and f.pid_s.integral == 0.0


def test_symbols_header_and_layout_agree():
    from tactics2d_amd import _ffi, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    for name in ("t2d_rs_follow_config", "t2d_rs_follow", "t2d_rs_follow_reset", "t2d_rs_follow_buffers"):
        assert name in _ffi.SYMBOLS and re.search(r"\b%s\s*\(" % name, header), name
    defs = dict(re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header))
    assert int(defs["T2D_PROFILE_RS_FOLLOW"]) == L.PROFILE_RS_FOLLOW == L.PROFILE_RS_PLAN + 1 and int(defs["T2D_ABI_VERSION"]) == 13
    for k, name in enumerate(("ADOPTED", "POP_REACHED", "POP_RISING", "FINISHED", "RESET", "DROPPED")):
        assert int(defs["T2D_RS_FOLLOW_" + name]) == getattr(L, "RS_FOLLOW_" + name) == 1 << k == getattr(F, "EV_" + name)
    body = re.search(r"typedef struct t2d_rs_follow_params \{(.*?)\} t2d_rs_follow_params;", header, re.S).group(1)
    fields = [n.strip() for decl in re.findall(r"double\s+([^;]+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S)) for n in decl.split(",")]
    assert fields == [n for n, _ in _ffi.RSFollowParams._fields_] == list(F.Params._fields)
    assert ctypes.sizeof(_ffi.RSFollowParams) == 8 * len(fields) and L.RS_FOLLOW_RECORD_BYTES == 48
    from tactics2d_amd.planner import rs_follow_params, rs_params
    p = rs_follow_params(rs_params("medium_car", steer_hi=0.524))
    assert F.Params(**p) == F.Params() and tuple(p) == F.Params._fields
    lib = _ffi.lib()
    assert all(hasattr(lib, n) for n in _ffi.SYMBOLS if n.startswith("t2d_rs_follow"))
