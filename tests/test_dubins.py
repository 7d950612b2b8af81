"""Dubins paths and sampled curve lines without a device: the specification (tests/curve_ref.py) against the fixture made by
running the reference's own classes (tests/golden/dubins_curves.npz, tests/golden/make_dubins.py), the properties the fixture
cannot give (word integration, the padding rule of t2d_curve_routes), and the agreement of header, ctypes table and layout.

TOL = 1e-9 is the project's figure for Reeds-Shepp outputs (tests/test_rs.py).  Here it also follows from the arithmetic:
coordinates stay below 64 m (ulp 1.4e-14), at most five chained segments, a sincos of a few ulp: an error around 1e-12.

Dubins._LRL (dubins.py:216-231) computes t = mod(-alpha + tmp + p / 2) where the family's form has -alpha - tmp + p / 2: slot 0's
curve misses the goal.  The fixture records it so, the specification keeps it for lrl="reference", and
test_the_reference_lrl_misses_the_goal states it."""
import ctypes
import functools
import os
import re

import numpy as np
import pytest

import curve_ref as CR
import helpers as H

TOL = 1e-9
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@functools.lru_cache(None)
def fixture():
    """dubins_curves.npz with the packed parts unpacked: valid bool [N, 6], seg [N, 6, 3], length [N, 6] (+inf for None)"""
    g = dict(H.load_npz("dubins_curves.npz"))
    n = len(g["valid"])
    valid = ((g["valid"][:, None] >> np.arange(6)) & 1).astype(bool)
    seg, length = np.zeros((n, 6, 3)), np.full((n, 6), np.inf)
    seg[valid], length[valid] = g["seg"], g["length"]
    g.update(valid_mask=g["valid"], valid=valid, seg=seg, length=length, start=g["start"].astype(np.float64),
             goal=g["goal"].astype(np.float64), c_start=g["c_start"].astype(np.float64), c_goal=g["c_goal"].astype(np.float64),
             c_first=np.concatenate([[0], np.cumsum(g["c_count"])]))
    return g


def spec_paths(which, lrl="reference"):
    g = fixture()
    rows = g["query_radius"] == which
    return rows, CR.all_paths(g["start"][rows], g["goal"][rows], float(g["radius"][which]), lrl)


def test_at_most_one_percent_of_the_fixture_is_unstable():
    g = fixture()
    assert 1 - g["stable"].mean() <= 0.01 and 1 - g["c_stable"].mean() <= 0.01
    assert len(g["stable"]) >= 1000 and len(g["c_stable"]) >= 200


@pytest.mark.parametrize("which", [0, 1])
def test_specification_paths_agree_with_the_reference(which):
    g = fixture()
    rows, (valid, seg, length) = spec_paths(which)
    st = g["stable"][rows].astype(bool)
    assert np.array_equal(valid[st], g["valid"][rows][st]) and np.array_equal(CR.mask_of(valid)[st], g["valid_mask"][rows][st])
    both = valid & g["valid"][rows]
    err_s, err_l = np.abs(seg - g["seg"][rows])[both].max(), np.abs(length[both] - g["length"][rows][both]).max()
    print("segments", err_s, "length", err_l)
    assert err_s <= TOL and err_l <= TOL
    last, first = CR.shortest_slots(length)
    two = np.sort(g["length"][rows], 1)[:, :2]
    clear = st & ~(two[:, 1] - two[:, 0] <= TOL)
    assert np.array_equal(last[clear], g["get_path"][rows][clear]) and clear.sum() > 0.9 * rows.sum()
    assert (first <= last).all() and (length[np.arange(len(last)), first] == length[np.arange(len(last)), last]).all()


def test_specification_words_and_defaults():
    g = fixture()
    assert np.array_equal(CR.LETTERS, g["letters"]) and CR.WORDS == ("LRL", "RLR", "LSL", "RSL", "RSR", "LSR")
    assert CR.DEFAULT_STEP == {CR.DUBINS: 0.1, CR.RS: 0.01}


def test_specification_at_the_degenerate_goals():
    g = fixture()
    for k in range(len(g["deg_radius"])):
        _, _, length = CR.all_paths(g["deg_start"][k], g["deg_goal"][k], float(g["deg_radius"][k]))
        last, _ = CR.shortest_slots(length)
        assert abs(length[0, last[0]] - g["deg_shortest"][k]) <= TOL and last[0] == g["deg_slot"][k], k
    # start == goal: every word has length 0 and get_path keeps the last one, LSR
    same = (g["deg_start"] == g["deg_goal"]).all(1)
    assert same.sum() >= 2 and (g["deg_shortest"][same] == 0).all() and (g["deg_slot"][same] == 5).all()


def spec_curve(g, k):
    n = int(g["c_n_seg"][k])
    return CR.curve_line(g["c_seg"][k, :n], g["c_letters"][k, :n], g["c_start"][k], float(g["radius"][g["c_radius"][k]]),
                         float(g["c_step"][k]), int(g["c_rule"][k]))


def test_specification_curves_agree_with_the_reference():
    g = fixture()
    worst_xy = worst_yaw = 0.0
    seen = set()
    for k in np.flatnonzero(g["c_stable"]):
        xy, yaw, end, counts = spec_curve(g, k)
        lo, hi = g["c_first"][k], g["c_first"][k + 1]
        assert len(xy) == g["c_count"][k] == hi - lo == sum(counts), k
        worst_xy = max(worst_xy, np.abs(xy - g["c_xy"][lo:hi]).max())
        worst_yaw = max(worst_yaw, np.abs(yaw - g["c_yaw"][lo:hi]).max())
        seen.add((int(g["c_rule"][k]), float(g["c_step"][k])))
    print("points", worst_xy, "yaw", worst_yaw)
    assert worst_xy <= TOL and worst_yaw <= TOL
    assert seen == {(0, 0.5), (0, 0.1), (1, 0.5), (1, 0.1)}
    # Reeds-Shepp curves of the fixture do reverse, Dubins words are all positive
    rs = g["c_rule"] == 1
    assert (g["c_seg"][rs] < 0).any() and (g["c_seg"][~rs] >= 0).all()


def test_tiny_segments_and_short_arcs():
    start, r = np.array([1.0, -2.0, 0.3]), 4.0
    for rule, step in ((CR.DUBINS, 0.1), (CR.RS, 0.01)):
        # |length| < 1e-15: the single point, the pose does not move
        xy, yaw, end, counts = CR.curve_line([1e-16, 0.5, 0.0], [1, 0, -1], start, r, step, rule)
        assert counts[0] == 1 and counts[2] == 1 and np.array_equal(xy[0], start[:2]) and yaw[0] == start[2]
        # an arc shorter than a step: one sampled point; Reeds-Shepp replaces it by [point, end_point] with yaw [h, h_end]
        xy, yaw, end, counts = CR.curve_line([0.5 * step / r], [1], start, r, step, rule)
        if rule == CR.RS:
            assert counts == [2] and np.array_equal(xy[1], end[:2]) and yaw[1] == end[2]
        else:
            assert counts == [1] and np.abs(xy[0] - start[:2]).max() <= 1e-12 and yaw[0] == start[2]   # (the circle's point at a0)
    # straights: max(1, ceil(L / step)) for Dubins, max(2, ...) for Reeds-Shepp, the end point included
    assert CR.curve_line([0.01], [0], start, r, 0.1, CR.DUBINS)[3] == [1] and CR.curve_line([0.01], [0], start, r, 0.1, CR.RS)[3] == [2]
    xy, _, end, _ = CR.curve_line([1.0], [0], start, r, 0.1, CR.DUBINS)
    assert len(xy) == 40 and np.array_equal(xy[-1], end[:2])
    # arcs omit their end point, the yaw reaches the end heading
    xy, yaw, end, _ = CR.curve_line([1.0], [-1], start, r, 0.1, CR.DUBINS)
    assert len(xy) == 40 and np.abs(xy[-1] - end[:2]).max() > 0.05 and yaw[-1] == end[2] == start[2] - 1.0
    # build-defined: no segments or non-finite input: an empty curve
    assert len(CR.curve_line([], [], start, r, 0.1, CR.DUBINS)[0]) == 0
    assert len(CR.curve_line([np.nan], [1], start, r, 0.1, CR.DUBINS)[0]) == 0
    assert len(CR.curve_line([1.0], [1], [np.inf, 0, 0], r, 0.1, CR.RS)[0]) == 0


def test_the_dubins_rule_reads_the_magnitude_of_a_segment():
    """DubinsPath.get_curve_line takes abs(segment) for arcs and straights alike (dubins.py:94-98): a caller-made word with a
    negative length gives the curve of its magnitudes; under the Reeds-Shepp rule the sign is `forward`."""
    start, r = np.array([1.0, -2.0, 0.3]), 4.0
    pos = CR.curve_line([0.7, 1.1, 0.4], [1, 0, -1], start, r, 0.1, CR.DUBINS)
    neg = CR.curve_line([-0.7, -1.1, 0.4], [1, 0, -1], start, r, 0.1, CR.DUBINS)
    assert np.array_equal(pos[0], neg[0]) and np.array_equal(pos[1], neg[1]) and np.array_equal(pos[2], neg[2])
    back = CR.curve_line([-0.7, -1.1, 0.4], [1, 0, -1], start, r, 0.1, CR.RS)
    assert np.abs(back[2][:2] - pos[2][:2]).max() > 1.0


def test_the_reference_lrl_misses_the_goal():
    """From the fixture alone: the last sampled point of slot 0 (LRL) lies farther than one step from the goal in almost every
    valid case; the other five words always end within one step of it, at the goal's heading or within one step's turn of it."""
    g = fixture()
    q, s = g["last_query"], g["last_slot"]
    miss = np.hypot(*(g["last"][:, :2] - g["goal"][q, :2]).T)
    dyaw = np.abs((g["last"][:, 2] - g["goal"][q, 2] + np.pi) % (2 * np.pi) - np.pi)
    step = 0.1
    lrl = s == 0
    share = (miss[lrl] > step).mean()
    print("LRL: valid", int(lrl.sum()), "miss the goal", share, "by up to", miss[lrl].max(), "others: worst", miss[~lrl].max())
    assert lrl.sum() >= 300 and share >= 0.9 and miss[lrl].max() > 5.0
    # (the heading: np.linspace reaches the end heading unless the last arc is a single point, less than a step long)
    turn = step / g["radius"][g["query_radius"][q]]
    assert (miss[~lrl] <= step).all() and (dyaw[~lrl] <= turn[~lrl] + TOL).all() and (dyaw[~lrl] <= TOL).mean() >= 0.95
    # get_path does pick LRL, and the curve fixture holds such curves
    assert (g["get_path"] == 0).sum() >= 10
    # the same from the specification: the word driven from the start ends away from the goal as written, on it when corrected
    for lrl_rule, on_goal in (("reference", False), ("standard", True)):
        for which in (0, 1):
            rows, (valid, seg, _) = spec_paths(which, lrl_rule)
            k = np.flatnonzero(valid[:, 0])
            end = np.array([CR.integrate(seg[i, 0], CR.LETTERS[0], g["start"][rows][i], float(g["radius"][which])) for i in k])
            off = np.hypot(*(end[:, :2] - g["goal"][rows][k, :2]).T)
            assert (off <= TOL).all() if on_goal else (off > step).mean() >= 0.9, (lrl_rule, which, off.max())


@pytest.mark.parametrize("which", [0, 1])
def test_valid_words_integrate_to_the_goal(which):
    """Driving a valid word from the start ends on the goal to 1e-9: the five sound words, and LRL under lrl="standard"."""
    g = fixture()
    radius = float(g["radius"][which])
    rows, (valid, seg, length) = spec_paths(which, "standard")
    start, goal = g["start"][rows], g["goal"][rows]
    worst = 0.0
    for s in range(6):
        for i in np.flatnonzero(valid[:, s]):
            end = CR.integrate(seg[i, s], CR.LETTERS[s], start[i], radius)
            dyaw = abs((end[2] - goal[i, 2] + np.pi) % (2 * np.pi) - np.pi)
            worst = max(worst, np.abs(end[:2] - goal[i, :2]).max(), dyaw)
    print("worst end-pose error", worst)
    assert worst <= TOL
    # the two rules differ in slot 0's t and q alone
    _, (valid_r, seg_r, _) = spec_paths(which, "reference")
    assert np.array_equal(valid, valid_r) and np.array_equal(seg[:, 1:], seg_r[:, 1:]) and np.array_equal(seg[:, 0, 1], seg_r[:, 0, 1])
    assert (seg[:, 0, 0] != seg_r[:, 0, 0]).any()
    # the sampled curve of a sound word ends on the goal too: its `end` is the word's end pose
    for i in range(20):
        s = int(CR.shortest_slots(length[i:i + 1])[0][0])
        _, _, end, _ = CR.curve_line(seg[i, s], CR.LETTERS[s], start[i], radius, 0.1, CR.DUBINS)
        assert np.abs(end[:2] - goal[i, :2]).max() <= TOL


def test_route_padding_rule():
    g = fixture()
    k = int(np.flatnonzero((g["c_rule"] == 0) & (g["c_step"] == 0.5))[0])
    xy, _, end, _ = spec_curve(g, k)
    c = len(xy)
    before = np.arange(2 * (c + 7), dtype=np.float32).reshape(-1, 2)
    v = CR.route_vertices(xy, end, c + 7, before)          # count <= capacity: the points, then the end point
    assert v.dtype == np.float32 and np.array_equal(v[:c], xy.astype(np.float32))
    assert (v[c:] == end[:2].astype(np.float32)).all() and len(v) == c + 7
    v = CR.route_vertices(xy, end, c, before[:c])          # count == capacity: no padding
    assert np.array_equal(v, xy.astype(np.float32))
    v = CR.route_vertices(xy, end, c - 3, before[:c - 3])  # count > capacity: the first `capacity` points
    assert np.array_equal(v, xy[:c - 3].astype(np.float32))
    v = CR.route_vertices(np.zeros((0, 2)), np.full(3, np.nan), 5, before[:5])   # no curve: the route stays
    assert np.array_equal(v, before[:5])


def test_radius_must_be_positive():
    from tactics2d_amd.interpolator import Dubins
    for bad in (0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            Dubins(bad)
    with pytest.raises(ValueError):
        Dubins(1.0, lrl="other")
    assert Dubins(2.5).radius == 2.5 and Dubins(2.5).lrl == "reference" and Dubins(2.5, lrl="standard").lrl == "standard"


def test_header_ffi_and_layout_agree():
    from tactics2d_amd import _ffi, build, layout as L
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    assert vals["T2D_DUBINS_SLOTS"] == 6 == L.DUBINS_SLOTS and vals["T2D_CURVE_WORD_BYTES"] == 48 == L.CURVE_WORD_BYTES
    assert (vals["T2D_CURVE_DUBINS"], vals["T2D_CURVE_RS"]) == (0, 1) == (L.CURVE_DUBINS, L.CURVE_RS) == (CR.DUBINS, CR.RS)
    assert vals["T2D_PROFILE_CURVE_ROUTES"] == 17 == L.PROFILE_CURVE_ROUTES == L.PROFILE_PURSUIT + 1
    assert vals["T2D_ABI_VERSION"] == 13 == L.ABI_VERSION
    assert L.CURVE_WORD_BYTES == 8 * L.RS_MAX_SEGMENTS + L.RS_MAX_SEGMENTS + 1 + 2
    for name, n_args in (("t2d_dubins_slot_info", 2), ("t2d_dubins_paths", 11), ("t2d_curve_lines", 13), ("t2d_curve_routes", 9),
                         ("t2d_route_vertices", 3)):
        assert len(_ffi.SYMBOLS[name][1]) == n_args, name
        decl = re.search(r"\bint " + name + r"\((.*?)\);", header, re.S).group(1)
        assert len(decl.split(",")) == n_args, name
    assert "t2d_curve.hip" in build.SOURCES and "t2d_curve_dev.h" in build.HEADERS
    # the library's own slot table, read without a device
    build.build()
    from tactics2d_amd.interpolator import Dubins, dubins_slot_table
    assert np.array_equal(dubins_slot_table(), CR.LETTERS) and Dubins.WORDS == CR.WORDS
    lib = ctypes.CDLL(_ffi.LIB_PATH)
    assert lib.t2d_dubins_slot_info(6, np.zeros(3, np.int8).ctypes.data_as(ctypes.c_void_p)) == _ffi.ERR_INVALID
    assert lib.t2d_dubins_slot_info(0, None) == _ffi.ERR_INVALID


def test_pack_words_layout():
    w = CR.pack_words(np.arange(10.0).reshape(2, 5), np.int8([[1, 0, -1, 1, -1], [0, 0, 1, 0, 0]]), [5, 3])
    raw = w.view(np.int8).reshape(2, 48)
    assert np.array_equal(w[:, :5], np.arange(10.0).reshape(2, 5))
    assert raw[0, 40:46].tolist() == [1, 0, -1, 1, -1, 5] and raw[1, 40:46].tolist() == [0, 0, 1, 0, 0, 3] and not raw[:, 46:].any()
