"""t2d_dubins_paths on the device: against the fixture made by running the reference (tests/golden/dubins_curves.npz), against
the specification (tests/curve_ref.py) on fresh seeded queries under both LRL rules, at the launch's edges (a workgroup takes
256 queries), on queries that are not finite, and on every error path.  TOL: see tests/test_dubins.py."""
import ctypes as C

import numpy as np
import pytest

import curve_ref as CR
from test_dubins import TOL, fixture

pytestmark = pytest.mark.gpu
BLOCK = 256   # queries of one workgroup (t2d_curve.hip kPathBlock)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _run(torch, radius, start, goal, lrl="reference"):
    from tactics2d_amd.interpolator import Dubins
    r = Dubins(radius, lrl).get_all_path(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2])
    torch.cuda.synchronize()
    return dict(valid=r.valid.cpu().numpy(), seg=r.segments.cpu().numpy(), length=r.length.cpu().numpy(),
                shortest=r.shortest.cpu().numpy(), first=r.shortest_first.cpu().numpy(), mask=r.mask.cpu().numpy())


def _fresh(n, seed=4711):
    rng = np.random.default_rng(seed)
    start = np.concatenate([rng.uniform(-25, 25, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(-14, 14, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    return start, goal


@pytest.fixture(scope="module")
def fresh_paths(torch):
    """4000 fresh queries at radius 3.3 under both rules, one launch each, and the specification's answers"""
    start, goal = _fresh(4000)
    out = {}
    for lrl in ("reference", "standard"):
        out[lrl] = (_run(torch, 3.3, start, goal, lrl), CR.all_paths(start, goal, 3.3, lrl), CR.stable_mask(start, goal, 3.3, lrl))
    return start, goal, out


def _compare(d, valid, seg, length, stable, what):
    assert np.array_equal(d["valid"][stable], valid[stable]) and np.array_equal(d["mask"][stable], CR.mask_of(valid)[stable]), what
    both = d["valid"] & valid
    err_s, err_l = np.abs(d["seg"] - seg)[both].max(), np.abs(d["length"][both] - length[both]).max()
    print(what, "segments", err_s, "length", err_l, "unstable", int((~stable).sum()))
    assert err_s <= TOL and err_l <= TOL, what
    # None: zero segments, +inf length
    assert (d["seg"][~d["valid"]] == 0).all() and np.isinf(d["length"][~d["valid"]]).all() and np.isfinite(d["length"][d["valid"]]).all()
    # the two tie rules, from the device's own lengths
    last, first = CR.shortest_slots(d["length"])
    assert np.array_equal(d["shortest"], last) and np.array_equal(d["first"], first), what


@pytest.mark.parametrize("which", [0, 1])
def test_paths_agree_with_the_reference(torch, which):
    g = fixture()
    rows = g["query_radius"] == which
    d = _run(torch, float(g["radius"][which]), g["start"][rows], g["goal"][rows])
    st = g["stable"][rows].astype(bool)
    _compare(d, g["valid"][rows], g["seg"][rows], g["length"][rows], st, f"fixture radius {which}")
    two = np.sort(g["length"][rows], 1)[:, :2]
    clear = st & ~(two[:, 1] - two[:, 0] <= TOL)
    assert np.array_equal(d["shortest"][clear], g["get_path"][rows][clear]) and clear.sum() > 0.9 * rows.sum()


@pytest.mark.parametrize("lrl", ["reference", "standard"])
def test_paths_agree_with_the_specification_on_fresh_queries(fresh_paths, lrl):
    _, _, out = fresh_paths
    d, (valid, seg, length), stable = out[lrl]
    assert stable.mean() >= 0.99
    _compare(d, valid, seg, length, stable, f"fresh {lrl}")
    last, _ = CR.shortest_slots(length)
    two = np.sort(length, 1)[:, :2]
    clear = stable & ~(two[:, 1] - two[:, 0] <= TOL)
    assert np.array_equal(d["shortest"][clear], last[clear])


def test_the_two_lrl_rules_differ_in_slot_0_alone(fresh_paths):
    _, _, out = fresh_paths
    a, b = out["reference"][0], out["standard"][0]
    assert np.array_equal(a["mask"], b["mask"]) and np.array_equal(a["seg"][:, 1:], b["seg"][:, 1:])
    assert np.array_equal(a["seg"][:, 0, 1], b["seg"][:, 0, 1]) and np.array_equal(a["length"][:, 1:], b["length"][:, 1:])
    assert (a["seg"][:, 0, 0] != b["seg"][:, 0, 0]).any()


def test_words_integrate_to_the_goal_on_fresh_inputs(fresh_paths):
    """the device's own segments, driven from the start: on the goal for the five sound words and for lrl="standard"; the
    reference's LRL is away from it"""
    start, goal, out = fresh_paths
    d = out["standard"][0]
    worst = 0.0
    for s in range(6):
        for i in np.flatnonzero(d["valid"][:1000, s]):
            end = CR.integrate(d["seg"][i, s], CR.LETTERS[s], start[i], 3.3)
            dyaw = abs((end[2] - goal[i, 2] + np.pi) % (2 * np.pi) - np.pi)
            worst = max(worst, np.abs(end[:2] - goal[i, :2]).max(), dyaw)
    print("worst end-pose error", worst)
    assert worst <= TOL
    r = out["reference"][0]
    k = np.flatnonzero(r["valid"][:1000, 0])
    off = np.array([np.abs(CR.integrate(r["seg"][i, 0], CR.LETTERS[0], start[i], 3.3)[:2] - goal[i, :2]).max() for i in k])
    assert (off > 0.1).mean() >= 0.9


@pytest.mark.parametrize("n", [1, BLOCK - 1, BLOCK + 1])
def test_block_edges(torch, fresh_paths, n):
    start, goal, out = fresh_paths
    d = _run(torch, 3.3, start[:n], goal[:n])
    for k in ("mask", "seg", "length", "shortest", "first"):
        assert d[k].shape[0] == n and np.array_equal(d[k], out["reference"][0][k][:n]), k


def test_shortest_at_the_degenerate_goals(torch):
    g = fixture()
    for r in g["radius"]:
        k = g["deg_radius"] == r
        d = _run(torch, float(r), g["deg_start"][k], g["deg_goal"][k])
        err = np.abs(d["length"][np.arange(k.sum()), d["shortest"]] - g["deg_shortest"][k]).max()
        print("radius", r, "shortest length error", err)
        assert err <= TOL
        exact = (g["deg_start"][k] == g["deg_goal"][k]).all(1)   # start == goal: all six lengths 0, get_path keeps LSR
        assert (d["shortest"][exact] == 5).all() and (d["first"][exact] == 0).all() and (d["length"][exact] == 0).all()


def test_queries_that_are_not_finite_touch_only_their_own_rows(torch, fresh_paths):
    start, goal, out = fresh_paths
    n = BLOCK + 40
    s, e = start[:n].copy(), goal[:n].copy()
    bad = np.array([0, 7, 63, 64, BLOCK - 1, BLOCK, n - 1])
    for j, i in enumerate(bad):
        (s if j % 2 else e)[i, j % 3] = (np.nan, np.inf, -np.inf)[j % 3]
    d = _run(torch, 3.3, s, e)
    good = np.setdiff1d(np.arange(n), bad)
    for k in ("mask", "seg", "length", "shortest", "first"):
        assert np.array_equal(d[k][good], out["reference"][0][k][good]), k
    assert (d["mask"][bad] == 0).all() and (d["shortest"][bad] == -1).all() and (d["first"][bad] == -1).all()
    assert (d["seg"][bad] == 0).all() and np.isinf(d["length"][bad]).all()


def test_get_path_and_numpy_or_tensor_inputs(torch):
    from tactics2d_amd.interpolator import Dubins
    g = fixture()
    db = Dubins(float(g["radius"][0]))
    s, e = g["start"][:100], g["goal"][:100]
    a = db.get_path(s[:, :2], s[:, 2], e[:, :2], e[:, 2])
    t = lambda v: torch.as_tensor(v, device="cuda")
    b = db.get_path(t(s[:, :2].copy()), t(s[:, 2].copy()), t(e[:, :2].copy()), t(e[:, 2].copy()))
    for k in ("slot", "segments", "steer", "n_seg", "length"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    ps, pe = t(s.copy()), t(e.copy())   # packed float64 [n, 3] poses are read in place
    c = db.get_all_path(ps, None, pe, None)
    assert c._inputs[0].data_ptr() == ps.data_ptr() and c._inputs[1].data_ptr() == pe.data_ptr()
    assert torch.equal(c.shortest, a.slot) and torch.equal(c.length[torch.arange(100), a.slot.long()], a.length)
    slot = a.slot.cpu().numpy()
    assert np.array_equal(a.steer.cpu().numpy(), CR.LETTERS[slot]) and (a.n_seg.cpu().numpy() == 3).all()
    assert Dubins.WORDS == CR.WORDS and c.WORDS == CR.WORDS
    with pytest.raises(ValueError):
        db.get_all_path(s[:, :2], s[:, 2], e[:50, :2], e[:50, 2])


def test_error_paths(torch):
    from tactics2d_amd import _ffi
    lib = _ffi.lib()
    n = 4
    start, goal = torch.zeros((n, 3), dtype=torch.float64, device="cuda"), torch.ones((n, 3), dtype=torch.float64, device="cuda")
    mask = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    seg = torch.full((n, 6, 3), 77.0, dtype=torch.float64, device="cuda")
    length = torch.full((n, 6), 77.0, dtype=torch.float64, device="cuda")
    short = torch.full((n, 2), 77, dtype=torch.int32, device="cuda")
    ptrs = [start.data_ptr(), goal.data_ptr(), mask.data_ptr(), seg.data_ptr(), length.data_ptr(), short.data_ptr()]

    def call(n_=n, radius=2.0, rule=0, null=None):
        p = [None if k == null else v for k, v in enumerate(ptrs)]
        return lib.t2d_dubins_paths(0, n_, radius, p[0], p[1], rule, p[2], p[3], p[4], p[5], None)

    for rc in (call(radius=0.0), call(radius=-1.0), call(radius=float("nan")), call(radius=float("inf")), call(n_=-1), call(rule=2),
               call(rule=-1)) + tuple(call(null=k) for k in range(6)):
        assert rc == _ffi.ERR_INVALID
    assert call(n_=0) == _ffi.OK
    torch.cuda.synchronize()
    assert (mask == 77).all() and (seg == 77).all() and (length == 77).all() and (short == 77).all()   # nothing was launched
    assert call() == _ffi.OK
    torch.cuda.synchronize()
    assert (mask != 77).all() and (short != 77).all()
