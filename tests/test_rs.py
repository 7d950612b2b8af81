"""Reeds-Shepp curves and the parking planner on the CPU: the specification (tests/rs_ref.py) against the fixture made by
running the reference (tests/golden/reeds_shepp.npz), the library's slot table against the same fixture, and the planner
scenes' conditions checked from the specification alone.  (The kernels against both: tests/test_gpu_rs.py.)"""
import os
import subprocess
import sys

import numpy as np
import pytest

import helpers as H
import rs_ref as R
import rs_scenes as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("TACTICS2D_REFERENCE", "/root/reference")
TOL = 1e-9   # three decades above the expected 1e-12 of ulp-level transcendentals, nine below a wrong formula


@pytest.mark.skipif(not os.path.isfile(os.path.join(REF, "tactics2d", "interpolator", "reeds_shepp.py")),
                    reason="the reference tree is not present")
def test_generator_reproduces_the_fixture_byte_for_byte(tmp_path):
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_rs.py"), "--ref", REF, "--out", str(tmp_path)],
                   check=True, capture_output=True, env=dict(os.environ, PYTHONDONTWRITEBYTECODE="1"))
    with open(tmp_path / "reeds_shepp.npz", "rb") as a, open(os.path.join(H.GOLD, "reeds_shepp.npz"), "rb") as b:
        assert a.read() == b.read()


def test_fixture_covers_what_it_claims():
    g = S.fixture()
    assert os.path.getsize(os.path.join(H.GOLD, "reeds_shepp.npz")) < 1 << 20
    assert len(g["stable"]) == 4000 and g["stable"].mean() >= 0.99
    counts = g["valid"].sum(0)
    print("valid per slot:", counts.tolist(), "stable share:", g["stable"].mean())
    assert (counts[:44] >= 5).all() and g["valid"].any(1).all()
    assert len(set(g["radius"].tolist())) == 2 and (np.hypot(g["start"][:, 0], g["start"][:, 1]) > 0).all()
    wide = (np.abs(g["start"][:, 2]) > np.pi) | (np.abs(g["goal"][:, 2]) > np.pi)
    assert 0.08 < wide.mean() < 0.12
    assert 25 <= len(g["deg_shortest"]) // 2 <= 35 and np.isfinite(g["deg_shortest"]).all()


def test_specification_candidates_agree_with_the_reference():
    g = S.fixture()
    valid, seg, length = R.all_paths(g["start"], g["goal"], g["radius_of"])
    st = g["stable"].astype(bool)
    assert np.array_equal(valid[st], g["valid"][st])
    both = valid & g["valid"]
    err_s, err_l = np.abs(seg - g["seg"])[both].max(), (np.abs(length[both] - g["length"][both]) / np.maximum(1.0, g["length"][both])).max()
    print("segments", err_s, "length", err_l)
    assert err_s <= TOL and err_l <= TOL
    last, first = R.shortest_slots(length)
    two = np.sort(g["length"], 1)[:, :2]
    clear = ~(two[:, 1] - two[:, 0] <= TOL)
    assert np.array_equal(last[clear & st], g["get_path"][clear & st]) and (first <= last).all()
    # (b): the shortest length at the degenerate goals
    _, _, dl = R.all_paths(g["deg_start"], g["deg_goal"], g["deg_radius"])
    assert np.abs(dl.min(1) - g["deg_shortest"]).max() <= TOL


def test_every_valid_word_of_the_fixture_integrates_to_the_goal():
    """reference-free: driving the word of a valid slot from the origin ends on the normalised goal pose"""
    g = S.fixture()
    x, y, phi = R.normalise(g["start"], g["goal"], g["radius_of"])
    worst = 0.0
    for s in range(48):
        k = g["valid"][:, s]
        if not k.any():
            continue
        ex, ey, eyaw = R.integrate(s, g["seg"][k, s])
        dyaw = np.abs((eyaw - phi[k] + np.pi) % (2 * np.pi) - np.pi)
        worst = max(worst, np.abs(ex - x[k]).max(), np.abs(ey - y[k]).max(), dyaw.max())
    print("worst end-pose error", worst)
    assert worst <= TOL


def test_the_library_slot_table_is_the_reference_s():
    from tactics2d_amd import layout as L
    from tactics2d_amd.interpolator import ReedsShepp
    g = S.fixture()
    letter = {1: "L", -1: "R", 0: "S"}
    words = tuple("".join(letter[int(v)] for v in g["letters"][s, :g["n_seg"][s]]) for s in range(48))
    assert ReedsShepp.WORDS == words and len(words) == L.RS_SLOTS
    assert ReedsShepp.CURVE_TYPES == tuple(("CSC", "CCC", "CCCC", "CCSC", "CCSCC")[c] for c in g["curve_type"])
    assert np.array_equal(ReedsShepp.SIGNS, g["signs"]) and np.array_equal(ReedsShepp.N_SEG, g["n_seg"])
    # ... and so is the specification's own
    assert tuple(R.WORDS) == words and np.array_equal(R.SIGNS, g["signs"])


def test_constructor_and_configuration_follow_the_reference():
    from tactics2d_amd.interpolator import ReedsShepp
    from tactics2d_amd.planner import rs_params
    for bad in (0, -1.0):
        with pytest.raises(ValueError):
            ReedsShepp(bad)
    assert ReedsShepp(4.0).radius == 4.0
    p = rs_params("medium_car", steer_hi=0.524)
    assert R.Params(**p) == S.PARAMS and R.Params._fields == tuple(p)
    from tactics2d_amd._ffi import RSParams
    assert tuple(n for n, _ in RSParams._fields_) == R.Params._fields
    assert p["radius"] == 2.637 / np.tan(0.524 * 0.98) and p["center_shift"] == 0.5 * 4.284 - 0.767 and p["threshold_distance"] == 15.0


def test_no_device_means_an_error_not_a_fallback():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from tactics2d_amd import _ffi
    from tactics2d_amd.interpolator import ReedsShepp
    with pytest.raises(_ffi.T2DError):
        ReedsShepp(4.0).get_all_path(np.zeros((1, 2)), np.zeros(1), np.ones((1, 2)), np.zeros(1))


def test_slot_info_and_paths_refuse_bad_arguments_without_a_device():
    import ctypes as C
    from tactics2d_amd import _ffi
    lib = _ffi.lib()
    buf = (C.c_int8 * 5)()
    n = C.c_int32()
    assert lib.t2d_rs_slot_info(48, buf, buf, C.byref(n), C.byref(n)) == _ffi.ERR_INVALID
    assert lib.t2d_rs_slot_info(-1, buf, buf, C.byref(n), C.byref(n)) == _ffi.ERR_INVALID
    one = C.c_void_p(8)   # never dereferenced: the arguments are refused first
    for radius in (0.0, -1.0, float("nan")):
        assert lib.t2d_rs_paths(0, 1, radius, one, one, one, one, one, one, None) == _ffi.ERR_INVALID
    assert lib.t2d_rs_paths(0, 1, 4.0, one, one, None, one, one, one, None) == _ffi.ERR_INVALID


@pytest.mark.parametrize("n_beams", [120, 24, 360])
def test_planner_scenes_show_every_outcome_and_few_knife_edges(n_beams):
    """from the specification alone, before any GPU run: each outcome occurs in >= 3 of the 65 envs, and at most 2 % of the envs
    change their decision when every scan value moves by +-1e-6 m (those are left out of the device comparison)"""
    plans = S.spec_plans(65, n_beams)
    cat = S.categories(plans)
    left_out = sum(not robust for _, robust in plans)
    print(n_beams, cat, "left out:", left_out, "of", len(plans))
    assert min(cat.values()) >= 3, cat
    assert left_out <= 0.02 * len(plans)
    for p, _ in plans:
        if p.status == R.FOUND:   # what the plan hands over: the word of its slot, driven, ends at the goal it was asked for
            assert p.n_seg == R.N_SEG[p.slot] and abs(np.abs(p.distance).sum() - p.length) <= TOL * max(1.0, p.length)
            assert p.length <= 2.0 * p.shortest and p.sorted_lengths[0] == p.shortest


def test_planner_rows_that_cannot_plan():
    c = S.planner_case(65, 120)
    p, e = c["params"], 0
    args = (c["target"][e], c["target_heading"][e])
    assert R.plan(p, S.LIDAR_RANGE, c["ego"][e], *args, c["scan"][e], active=False).status == R.NO_TARGET
    assert R.plan(p, S.LIDAR_RANGE, [np.nan, 0, 0], *args, c["scan"][e]).status == R.NO_TARGET
    bad = c["scan"][e].copy()
    bad[5] = np.nan
    assert R.plan(p, S.LIDAR_RANGE, c["ego"][e], *args, bad).status == R.UNCHECKED
    # +inf counts as the range (np.clip)
    a = R.plan(p, S.LIDAR_RANGE, c["ego"][e], *args, np.full(120, np.inf, np.float32))
    b = R.plan(p, S.LIDAR_RANGE, c["ego"][e], *args, np.full(120, S.LIDAR_RANGE, np.float32))
    assert a.status == b.status and a.slot == b.slot
