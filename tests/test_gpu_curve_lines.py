"""t2d_curve_lines and t2d_curve_routes on the device: the sampled curve lines against the fixture made by running the reference
(tests/golden/dubins_curves.npz) and against the specification (tests/curve_ref.py) on fresh seeded queries; counts around the
256 lanes of a curve's workgroup; truncation with a guard region; empty and non-finite words; every error path; curves written
into the route sets against the specification and against a twin pool that got the same vertices from the host; and
RSPlanner.write_routes on the planner scenes of tests/rs_scenes.py.  TOL: see tests/test_dubins.py.

Route vertices are fp32: the device's fp64 point and the specification's differ by less than TOL, so their fp32 roundings are
equal or neighbours -- the vertex tests allow one fp32 ulp (2^-17 m below 64 m) and print how many vertices are bit-equal."""
import numpy as np
import pytest

import curve_ref as CR
import pid_scenes as PS
import pursuit_scenes as US
import rs_scenes as S
from route_writers import A, N_ENV, placeholder, route_pool as _route_pool
from test_dubins import TOL, fixture, spec_curve

pytestmark = pytest.mark.gpu
LANES = 256          # lanes of a curve's workgroup (t2d_curve.hip kCurveBlock)
ULP32 = 2.0 ** -17   # one fp32 ulp of a coordinate in [32, 64) m
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _lines(torch, words, starts, radius, step, rule, max_points):
    """one t2d_curve_lines over numpy inputs -> numpy outputs"""
    from tactics2d_amd.interpolator import curve_lines
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")
    r = curve_lines(t(words), t(starts), radius, step, rule, max_points)
    torch.cuda.synchronize()
    return dict(xy=r.xy.cpu().numpy(), yaw=r.yaw.cpu().numpy(), count=r.count.cpu().numpy(), end=r.end.cpu().numpy())


def _against_spec(d, seg, letters, n_seg, starts, radius, step, rule, stable=None, what=""):
    """device rows against curve_ref.curve_line, curve by curve; returns the largest deviation"""
    worst = 0.0
    for k in range(len(seg)):
        if stable is not None and not stable[k]:
            continue
        n = int(n_seg[k])
        xy, yaw, end, _ = CR.curve_line(seg[k, :n], letters[k, :n], starts[k], radius, step, rule)
        assert d["count"][k] == len(xy), (what, k, d["count"][k], len(xy))
        c = min(len(xy), d["xy"].shape[1])
        if c:
            worst = max(worst, np.abs(d["xy"][k, :c] - xy[:c]).max(), np.abs(d["yaw"][k, :c] - yaw[:c]).max())
        if len(xy):
            worst = max(worst, np.abs(d["end"][k] - end).max())
    return worst


def test_curves_agree_with_the_reference(torch):
    g = fixture()
    worst = 0.0
    for ri in (0, 1):
        for step in (0.5, 0.1):
            for rule in (CR.DUBINS, CR.RS):
                k = np.flatnonzero((g["c_radius"] == ri) & (g["c_step"] == step) & (g["c_rule"] == rule))
                cap = int(g["c_count"][k].max())
                d = _lines(torch, CR.pack_words(g["c_seg"][k], g["c_letters"][k], g["c_n_seg"][k]), g["c_start"][k],
                           float(g["radius"][ri]), step, rule, cap)
                for j, kk in enumerate(k):
                    if not g["c_stable"][kk]:
                        continue
                    lo, hi = g["c_first"][kk], g["c_first"][kk + 1]
                    assert d["count"][j] == hi - lo, (kk, d["count"][j], hi - lo)
                    worst = max(worst, np.abs(d["xy"][j, :hi - lo] - g["c_xy"][lo:hi]).max(),
                                np.abs(d["yaw"][j, :hi - lo] - g["c_yaw"][lo:hi]).max())
                    worst = max(worst, np.abs(d["end"][j] - spec_curve(g, kk)[2]).max())
    print("largest deviation from the reference's points, yaws and the specification's end poses:", worst)
    assert worst <= TOL


@pytest.fixture(scope="module")
def fresh_curves(torch):
    """get_curve of 1500 fresh queries per family at step 0.5 (the device's own paths), downloaded"""
    from tactics2d_amd.interpolator import Dubins, ReedsShepp
    rng = np.random.default_rng(2718)
    n, radius = 1500, 3.3
    start = np.concatenate([rng.uniform(-25, 25, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(-14, 14, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    out = {}
    for name, planner, rule in (("dubins", Dubins(radius), CR.DUBINS), ("dubins_standard", Dubins(radius, "standard"), CR.DUBINS),
                                ("rs", ReedsShepp(radius), CR.RS)):
        path = planner.get_path(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2])
        r = planner.get_curve(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2], step_size=0.5, max_points=160)
        torch.cuda.synchronize()
        seg = path.segments.cpu().numpy()
        seg = np.concatenate([seg, np.zeros((n, 5 - seg.shape[1]))], 1)
        letters = path.steer.cpu().numpy().astype(np.int8)
        letters = np.concatenate([letters, np.zeros((n, 5 - letters.shape[1]), np.int8)], 1)
        out[name] = dict(xy=r.xy.cpu().numpy(), yaw=r.yaw.cpu().numpy(), count=r.count.cpu().numpy(), end=r.end.cpu().numpy(),
                         slot=r.slot.cpu().numpy(), seg=seg, letters=letters, n_seg=path.n_seg.cpu().numpy(), rule=rule)
    return start, goal, radius, out


@pytest.mark.parametrize("family", ["dubins", "rs"])
def test_curves_agree_with_the_specification_on_fresh_queries(fresh_curves, family):
    start, goal, radius, out = fresh_curves
    d = out[family]
    stable = np.array([CR.stable_count(d["seg"][k, :d["n_seg"][k]], d["letters"][k], start[k], radius, 0.5, d["rule"])
                       for k in range(len(start))])
    assert stable.mean() >= 0.99 and (d["count"] <= 160).all() and (d["count"] > 0).all()
    worst = _against_spec(d, d["seg"], d["letters"], d["n_seg"], start, radius, 0.5, d["rule"], stable, family)
    print(family, "largest deviation from the specification:", worst, "unstable", int((~stable).sum()))
    assert worst <= TOL
    if family == "rs":
        assert (d["seg"] < 0).any() and (d["n_seg"] >= 4).any()


def test_end_is_the_goal_except_for_the_reference_lrl(fresh_curves):
    start, goal, radius, out = fresh_curves

    def miss(d):
        dyaw = np.abs((d["end"][:, 2] - goal[:, 2] + np.pi) % (2 * np.pi) - np.pi)
        return np.maximum(np.abs(d["end"][:, :2] - goal[:, :2]).max(1), dyaw)

    ref, std, rs = out["dubins"], out["dubins_standard"], out["rs"]
    lrl = ref["slot"] == 0
    print("reference rule: LRL chosen", int(lrl.sum()), "worst miss of the others", miss(ref)[~lrl].max(), "of LRL", miss(ref)[lrl].max(),
          "standard rule:", miss(std).max(), "Reeds-Shepp:", miss(rs).max())
    assert lrl.sum() >= 10 and (miss(ref)[~lrl] <= TOL).all() and (miss(ref)[lrl] > 0.1).mean() >= 0.9
    assert (miss(std) <= TOL).all() and (std["slot"] == 0).sum() >= 10 and (miss(rs) <= TOL).all()


def _edge_words(radius, step):
    """single-segment Dubins words whose counts sit around the lane count: straights and arcs of 255, 256, 257 and 513 points, and
    a three-segment word whose second segment starts on the last lane"""
    seg, letters, n_seg = [], [], []
    for c in (LANES - 1, LANES, LANES + 1, 2 * LANES + 1):
        for l in (0, 1, -1):
            seg.append([(c - 0.5) * step / radius, 0, 0, 0, 0]); letters.append([l, 0, 0, 0, 0]); n_seg.append(1)
    seg.append([(LANES - 1.5) * step / radius, 3.5 * step / radius, 2.5 * step / radius, 0, 0]); letters.append([1, 0, -1, 0, 0]); n_seg.append(3)
    return np.array(seg), np.array(letters, np.int8), np.array(n_seg)


def test_counts_around_the_lane_count(torch):
    radius, step = 4.0, 0.25
    seg, letters, n_seg = _edge_words(radius, step)
    starts = np.tile([1.0, -2.0, 0.7], (len(seg), 1))
    d = _lines(torch, CR.pack_words(seg, letters, n_seg), starts, radius, step, CR.DUBINS, 600)
    assert d["count"][:12].tolist() == [c for c in (255, 256, 257, 513) for _ in range(3)] and d["count"][12] == 255 + 4 + 3
    worst = _against_spec(d, seg, letters, n_seg, starts, radius, step, CR.DUBINS)
    print("largest deviation:", worst)
    assert worst <= TOL


def test_tiny_segments_short_arcs_and_negative_lengths_on_the_device(torch):
    """the branches a path of get_path seldom takes, sent on purpose under both rules: |length| < 1e-15 (the single point), an arc
    shorter than a step (Dubins: one point; Reeds-Shepp: [point, end_point]), an arc of zero sampled points, a straight shorter
    than a step, and negative lengths (Reeds-Shepp: backwards; Dubins: the magnitude is read)"""
    radius = 4.0
    seg = np.array([[1e-16, 0.5, 0.0, 0, 0], [0.5, 1e-16, 0.3, 0, 0], [0.5 * 0.1 / radius, 0, 0, 0, 0], [0.3, 0.5 * 0.1 / radius, 0.2, 0, 0],
                    [2e-15, 0, 0, 0, 0], [0.002, 0, 0, 0, 0], [-0.7, -1.1, 0.4, 0, 0], [0.6, -0.5 * 0.1 / radius, -0.4, 0.2, -1e-16]])
    letters = np.int8([[1, 0, -1, 0, 0], [-1, 1, 0, 0, 0], [1, 0, 0, 0, 0], [0, -1, 1, 0, 0],
                       [-1, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 0, -1, 0, 0], [1, -1, 0, 1, -1]])
    n_seg = np.array([3, 3, 1, 3, 1, 1, 3, 5])
    starts = np.tile([1.0, -2.0, 0.3], (len(seg), 1))
    for rule, step in ((CR.DUBINS, 0.1), (CR.RS, 0.1), (CR.RS, 0.01)):
        d = _lines(torch, CR.pack_words(seg, letters, n_seg), starts, radius, step, rule, 400)
        worst = _against_spec(d, seg, letters, n_seg, starts, radius, step, rule, None, f"rule {rule} step {step}")
        print("rule", rule, "step", step, "counts", d["count"].tolist(), "largest deviation", worst)
        assert worst <= TOL
        if step == 0.1:   # the sub-step arc alone, the near-zero arc and the short straight: 1 point each for Dubins, 2 for Reeds-Shepp
            assert d["count"][[2, 4, 5]].tolist() == ([1, 1, 1] if rule == CR.DUBINS else [2, 2, 2])
            assert np.array_equal(d["xy"][0, 0], starts[0, :2]) and d["yaw"][0, 0] == starts[0, 2]        # the tiny segment IS the start pose
    # Dubins reads |seg|: word 6 gives the bits of its all-positive twin
    twin = seg.copy()
    twin[6] = np.abs(twin[6])
    a = _lines(torch, CR.pack_words(seg[6:7], letters[6:7], n_seg[6:7]), starts[6:7], radius, 0.1, CR.DUBINS, 400)
    b = _lines(torch, CR.pack_words(twin[6:7], letters[6:7], n_seg[6:7]), starts[6:7], radius, 0.1, CR.DUBINS, 400)
    c = int(a["count"][0])
    assert c == b["count"][0] and np.array_equal(a["xy"][0, :c], b["xy"][0, :c]) and np.array_equal(a["end"], b["end"])


def test_get_curve_on_a_side_stream_and_with_its_defaults(torch):
    """everything get_curve enqueues -- both launches and the gather between them -- goes to the stream it is given: the answer
    on a side stream is the default stream's, bit for bit; and the reference's default steps with the default point budget"""
    from tactics2d_amd.interpolator import Dubins, ReedsShepp, default_max_points
    rng = np.random.default_rng(5)
    n, radius = 20000, 3.3
    start = np.concatenate([rng.uniform(-25, 25, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(-14, 14, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    ps, pg = torch.as_tensor(start, device="cuda"), torch.as_tensor(goal, device="cuda")
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for planner in (Dubins(radius, "standard"), ReedsShepp(radius)):
        want = planner.get_curve(ps, None, pg, None, step_size=0.5, max_points=128)
        torch.cuda.synchronize()
        for _ in range(3):
            got = planner.get_curve(ps, None, pg, None, step_size=0.5, max_points=128, stream=side)
            side.synchronize()
            assert torch.equal(got.count, want.count) and torch.equal(got.slot, want.slot) and torch.equal(got.end, want.end)
            k = torch.arange(128, device="cuda")[None] < want.count[:, None]
            assert torch.equal(got.xy[k], want.xy[k]) and torch.equal(got.yaw[k], want.yaw[k])
        path = planner.get_path(ps, None, pg, None, stream=side)
        side.synchronize()
        assert torch.equal(path.slot, want.slot)
    # defaults: step 0.1 (Dubins) and 0.01 (Reeds-Shepp), max_points = default_max_points(radius, step, 64 m)
    for planner, rule in ((Dubins(radius, "standard"), CR.DUBINS), (ReedsShepp(radius), CR.RS)):
        r = planner.get_curve(start[:3, :2], start[:3, 2], goal[:3, :2], goal[:3, 2])
        path = planner.get_path(start[:3, :2], start[:3, 2], goal[:3, :2], goal[:3, 2])
        torch.cuda.synchronize()
        step = CR.DEFAULT_STEP[rule]
        assert r.xy.shape == (3, default_max_points(radius, step, 64.0), 2)
        seg, letters, n_seg = path.segments.cpu().numpy(), path.steer.cpu().numpy(), path.n_seg.cpu().numpy()
        d = dict(xy=r.xy.cpu().numpy(), yaw=r.yaw.cpu().numpy(), count=r.count.cpu().numpy(), end=r.end.cpu().numpy())
        stable = [CR.stable_count(seg[k, :n_seg[k]], letters[k], start[k], radius, step, rule) for k in range(3)]
        worst = _against_spec(d, seg, letters, n_seg, start[:3], radius, step, rule, stable, "defaults")
        print("rule", rule, "default step", step, "counts", d["count"].tolist(), "largest deviation", worst)
        dyaw = np.abs((d["end"][:, 2] - goal[:3, 2] + np.pi) % (2 * np.pi) - np.pi)
        assert worst <= TOL and (d["count"] < r.xy.shape[1]).all() and np.abs(d["end"][:, :2] - goal[:3, :2]).max() <= TOL and dyaw.max() <= TOL


def _raw(torch, words, starts, radius, step, rule, max_points, guard=64):
    """t2d_curve_lines through the C interface into sentinel-filled buffers with a guard region behind them"""
    from tactics2d_amd import _ffi
    n = len(words)
    t = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")
    w, s = t(words), t(starts)
    xy = torch.full((n * max(max_points, 1) + guard, 2), SENTINEL, dtype=torch.float64, device="cuda")
    yaw = torch.full((n * max(max_points, 1) + guard,), SENTINEL, dtype=torch.float64, device="cuda")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    end = torch.full((n, 3), SENTINEL, dtype=torch.float64, device="cuda")
    rc = _ffi.lib().t2d_curve_lines(0, n, w.data_ptr(), s.data_ptr(), radius, step, rule, max_points, xy.data_ptr(), yaw.data_ptr(),
                                    count.data_ptr(), end.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, xy.cpu().numpy(), yaw.cpu().numpy(), count.cpu().numpy(), end.cpu().numpy()


def test_truncation_reports_the_full_count_and_writes_nothing_past_max_points(torch):
    radius, step = 4.0, 0.25
    seg, letters, n_seg = _edge_words(radius, step)
    seg, letters, n_seg = seg[[3, 4, 12]], letters[[3, 4, 12]], n_seg[[3, 4, 12]]   # counts 256 (a straight), 256 (an arc), 262
    starts = np.tile([1.0, -2.0, 0.7], (3, 1))
    words = CR.pack_words(seg, letters, n_seg)
    full = _lines(torch, words, starts, radius, step, CR.DUBINS, 300)
    for max_points in (1, 255, 256, 262, 261):
        rc, xy, yaw, count, end = _raw(torch, words, starts, radius, step, CR.DUBINS, max_points)
        assert rc == 0 and count.tolist() == [256, 256, 262], max_points
        for k in range(3):
            c = min(int(count[k]), max_points)
            row = slice(k * max_points, k * max_points + c)
            assert np.array_equal(xy[row], full["xy"][k, :c]) and np.array_equal(yaw[row], full["yaw"][k, :c]), (max_points, k)
            rest = slice(k * max_points + c, (k + 1) * max_points)
            assert (xy[rest] == SENTINEL).all() and (yaw[rest] == SENTINEL).all(), (max_points, k)
        assert (xy[3 * max_points:] == SENTINEL).all() and (yaw[3 * max_points:] == SENTINEL).all(), max_points   # the guard
        assert np.array_equal(end, full["end"])


def test_empty_and_non_finite_words_touch_only_their_own_rows(torch):
    g = fixture()
    k = np.flatnonzero((g["c_radius"] == 0) & (g["c_step"] == 0.5) & (g["c_rule"] == CR.RS))[:12]
    seg, letters, n_seg, starts = g["c_seg"][k].copy(), g["c_letters"][k], g["c_n_seg"][k].copy(), g["c_start"][k].copy()
    radius, cap = float(g["radius"][0]), int(g["c_count"][k].max())
    _, xy0, yaw0, count0, end0 = _raw(torch, CR.pack_words(seg, letters, n_seg), starts, radius, 0.5, CR.RS, cap)
    n_seg[1] = 0                    # a word of 0 segments
    seg[4, 0] = np.nan              # segments and starts that are not finite
    seg[5, 1] = np.inf
    starts[7, 0] = np.nan
    starts[8, 2] = -np.inf
    n_seg[10] = 6                   # more segments than a word holds
    bad = [1, 4, 5, 7, 8, 10]
    rc, xy, yaw, count, end = _raw(torch, CR.pack_words(seg, letters, n_seg), starts, radius, 0.5, CR.RS, cap)
    assert rc == 0
    for j in range(12):
        row = slice(j * cap, (j + 1) * cap)
        if j in bad:
            assert count[j] == 0 and (xy[row] == SENTINEL).all() and (yaw[row] == SENTINEL).all() and (end[j] == SENTINEL).all(), j
        else:
            assert count[j] == count0[j] and np.array_equal(xy[row], xy0[row]) and np.array_equal(yaw[row], yaw0[row]), j
            assert np.array_equal(end[j], end0[j]), j


def test_curve_lines_error_paths(torch):
    from tactics2d_amd import _ffi
    from tactics2d_amd.interpolator import curve_lines
    words = CR.pack_words([[1.0, 0, 0, 0, 0]], np.int8([[1, 0, 0, 0, 0]]), [1])
    starts = np.zeros((1, 3))
    for kw in (dict(radius=0.0), dict(radius=-1.0), dict(radius=float("nan")), dict(step=0.0), dict(step=-0.1), dict(step=float("inf")),
               dict(max_points=0), dict(max_points=-3), dict(rule=2), dict(rule=-1)):
        a = dict(radius=2.0, step=0.1, rule=0, max_points=8)
        a.update(kw)
        rc, xy, yaw, count, end = _raw(torch, words, starts, a["radius"], a["step"], a["rule"], a["max_points"])
        assert rc == _ffi.ERR_INVALID, kw
        assert (xy == SENTINEL).all() and (count == -7).all() and (end == SENTINEL).all(), kw   # nothing was launched
    lib = _ffi.lib()
    t = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = t.data_ptr()
    for null in range(6):
        a = [None if k == null else p for k in range(6)]
        assert lib.t2d_curve_lines(0, 1, a[0], a[1], 2.0, 0.1, 0, 2, a[2], a[3], a[4], a[5], None) == _ffi.ERR_INVALID, null
    assert lib.t2d_curve_lines(0, -1, p, p, 2.0, 0.1, 0, 2, p, p, p, p, None) == _ffi.ERR_INVALID
    assert lib.t2d_curve_lines(0, 1, p, p, 2.0, 0.1, 0, 2, p + 8, p, p, p, None) == _ffi.ERR_INVALID   # xy not 16-byte aligned
    assert lib.t2d_curve_lines(0, 1, p + 4, p, 2.0, 0.1, 0, 2, p, p, p, p, None) == _ffi.ERR_INVALID   # words not 8-byte aligned
    assert lib.t2d_curve_lines(0, 0, p, p, 2.0, 0.1, 0, 2, p, p, p, p, None) == _ffi.OK
    with pytest.raises(ValueError):
        curve_lines(torch.zeros((2, 5), dtype=torch.float64, device="cuda"), torch.zeros((2, 3), dtype=torch.float64, device="cuda"),
                    2.0, 0.1, "dubins", 8)
    with pytest.raises(_ffi.T2DError):
        curve_lines(torch.zeros((2, 6), dtype=torch.float64, device="cuda"), torch.zeros((2, 3), dtype=torch.float64, device="cuda"),
                    2.0, 0.1, "dubins", 0)


# ---- curves as routes ------------------------------------------------------------------------------------------------------------
CAP = 96


def _placeholder(e, cap=CAP):
    return placeholder(cap, e, 200.0)


def _consumers(torch, pool):
    """off_route, pid_actions and pursuit_actions of the pool's current state -> the bytes of everything they write"""
    from tactics2d_amd import layout as L
    n = pool.n
    dist, _ = pool.off_route_host()
    out = {"off_route": dist.copy(), "off": pool.off_route_all()[1].copy()}
    for name, call, nbytes in (("pid", pool.pid_actions, L.PID_RECORD_BYTES), ("pursuit", pool.pursuit_actions, L.PURSUIT_RECORD_BYTES)):
        rows = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")
        rec = torch.zeros((n, nbytes // 8), dtype=torch.float64, device="cuda")
        call(None, rows.data_ptr(), rec.data_ptr())
        pool.sync()
        out[name + "_rows"], out[name + "_rec"] = rows.cpu().numpy().view(np.uint32), rec.cpu().numpy().view(np.uint64)
    return out


def test_curve_routes_against_the_specification_and_a_twin_pool(torch):
    from tactics2d_amd.interpolator import Dubins, pack_words
    rng = np.random.default_rng(99)
    radius, step = 4.0, 0.5
    start = np.concatenate([rng.uniform(-10, 10, (N_ENV, 2)), rng.uniform(-3, 3, (N_ENV, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(-12, 12, (N_ENV, 2)), rng.uniform(-3, 3, (N_ENV, 1))], 1)
    goal[2, :2] = start[2, :2] + [40.0, 30.0]          # env 2: 50 m and more, over 96 points at step 0.5
    path = Dubins(radius, "standard").get_path(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2])
    n_seg = path.n_seg.clone()
    n_seg[5] = 0                                       # env 5: a word of 0 segments
    pad = torch.zeros((N_ENV, 2), dtype=torch.float64, device="cuda")
    words = pack_words(torch.cat([path.segments, pad], 1), torch.cat([path.steer, pad.to(torch.int8)], 1), n_seg)
    starts = torch.as_tensor(start, device="cuda")
    # participants: spread along each env's chord from start to goal, a little off it
    f = np.repeat(np.linspace(0.1, 0.9, A)[None], N_ENV, 0)
    x = (start[:, None, 0] + f * (goal[:, None, 0] - start[:, None, 0]) + rng.uniform(-1, 1, (N_ENV, A))).astype(np.float32).ravel()
    y = (start[:, None, 1] + f * (goal[:, None, 1] - start[:, None, 1]) + rng.uniform(-1, 1, (N_ENV, A))).astype(np.float32).ravel()
    heading = rng.uniform(-3, 3, N_ENV * A).astype(np.float32)
    speed = rng.uniform(2, 6, N_ENV * A).astype(np.float32)
    sets = [[_placeholder(e)] for e in range(N_ENV)]

    def controllers(pool):   # (a participant has one controller: agents 0 and 1 of every env follow by PID, 2 and 3 by pure pursuit)
        from tactics2d_amd import layout as L
        agent = np.tile(np.arange(A), N_ENV)
        pool.set_pid(PS.ring_controller().row()[None], np.where(agent < 2, 0, L.PID_NONE).astype(np.uint8), speed)
        pool.set_pursuit(US.ring_controller().row()[None], np.where(agent >= 2, 0, L.PURSUIT_NONE).astype(np.uint8), speed)

    pool = _route_pool(x, y, heading, speed)
    pool.set_routes(sets, np.arange(N_ENV), 0, 1.5)
    controllers(pool)
    before = pool.route_vertices().cpu().numpy().copy()
    assert before.shape == (N_ENV * CAP, 2) and np.array_equal(before, np.concatenate([s[0] for s in sets]))
    pool.profile_enable(True)
    count = pool.curve_routes(words, starts, radius, step, "dubins", 0)
    pool.sync()
    from tactics2d_amd import layout as L
    assert pool.profile_read(L.PROFILE_CURVE_ROUTES)[1] == 1
    pool.profile_enable(False)
    count = count.cpu().numpy()
    verts = pool.route_vertices().cpu().numpy().reshape(N_ENV, CAP, 2)
    seg, letters = path.segments.cpu().numpy(), path.steer.cpu().numpy()
    want, bit_equal, total = np.zeros_like(verts), 0, 0
    for e in range(N_ENV):
        xy, _, end, _ = CR.curve_line(seg[e] if e != 5 else [], letters[e], start[e], radius, step, CR.DUBINS)
        assert count[e] == len(xy), e
        want[e] = CR.route_vertices(xy, end, CAP, before.reshape(N_ENV, CAP, 2)[e])
        if 0 < len(xy) <= CAP:    # the route reaches the goal although the arcs omit it
            assert np.abs(verts[e, -1] - goal[e, :2].astype(np.float32)).max() <= ULP32, e
    assert count[2] > CAP and count[5] == 0 and ((count > 0) & (count < CAP)).sum() >= 5
    assert np.array_equal(verts[5], before.reshape(N_ENV, CAP, 2)[5])       # the 0-segment word's route is unchanged, bit for bit
    bit_equal, total = int((verts == want).sum()), verts.size
    print("vertices bit-equal to the fp32 rounding of the specification:", bit_equal, "of", total,
          "largest difference", np.abs(verts.astype(np.float64) - want).max())
    assert np.abs(verts.astype(np.float64) - want.astype(np.float64)).max() <= ULP32 and bit_equal >= 0.99 * total
    got = _consumers(torch, pool)
    # a twin pool that gets the SAME vertices from the host
    twin = _route_pool(x, y, heading, speed)
    twin.set_routes([[verts[e]] for e in range(N_ENV)], np.arange(N_ENV), 0, 1.5)
    controllers(twin)
    ref = _consumers(torch, twin)
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    assert np.isfinite(got["off_route"]).all() and (got["off_route"].reshape(N_ENV, A)[[0, 1, 3, 4, 6, 7]] < 8.0).all()
    pool.close()
    twin.close()


def test_curve_routes_error_paths(torch):
    from tactics2d_amd import _ffi
    from tactics2d_amd.interpolator import pack_words
    z = np.zeros(N_ENV * A, np.float32)
    pool = _route_pool(z, z, z, z)
    words = pack_words(torch.ones((N_ENV, 5), dtype=torch.float64, device="cuda"), torch.ones((N_ENV, 5), dtype=torch.int8, device="cuda"),
                       torch.full((N_ENV,), 3, dtype=torch.int32, device="cuda"))
    starts = torch.zeros((N_ENV, 3), dtype=torch.float64, device="cuda")

    def state_error(**kw):
        a = dict(radius=4.0, step_size=0.5, rule="dubins", route=0)
        a.update(kw)
        with pytest.raises(_ffi.T2DError) as ei:
            pool.curve_routes(words, starts, a["radius"], a["step_size"], a["rule"], a["route"])
        return ei.value.code

    assert state_error() == _ffi.ERR_STATE                                           # no routes installed
    with pytest.raises(_ffi.T2DError) as ei:
        pool.route_vertices()
    assert ei.value.code == _ffi.ERR_STATE
    pool.set_routes([[_placeholder(0)]], None, 0, 1.0)                               # one set shared by every env
    assert state_error() == _ffi.ERR_STATE
    sets = [[_placeholder(e)] + ([_placeholder(e)[:4]] if e != 3 else []) for e in range(N_ENV)]
    pool.set_routes(sets, np.arange(N_ENV), 0, 1.0)
    before = pool.route_vertices().cpu().numpy().copy()
    assert state_error(route=1) == _ffi.ERR_STATE                                    # env 3's set has no route 1
    assert state_error(route=2) == _ffi.ERR_STATE
    for kw in (dict(radius=0.0), dict(radius=float("nan")), dict(step_size=0.0), dict(step_size=-1.0), dict(rule=2), dict(route=-1)):
        assert state_error(**kw) == _ffi.ERR_INVALID, kw
    lib = _ffi.lib()
    assert lib.t2d_curve_routes(pool._h, None, starts.data_ptr(), 4.0, 0.5, 0, 0, None, None) == _ffi.ERR_INVALID
    assert lib.t2d_curve_routes(pool._h, words.data_ptr(), None, 4.0, 0.5, 0, 0, None, None) == _ffi.ERR_INVALID
    assert lib.t2d_curve_routes(None, words.data_ptr(), starts.data_ptr(), 4.0, 0.5, 0, 0, None, None) == _ffi.ERR_INVALID
    assert lib.t2d_curve_routes(pool._h, words.data_ptr() + 4, starts.data_ptr(), 4.0, 0.5, 0, 0, None, None) == _ffi.ERR_INVALID   # misaligned
    import ctypes as C
    ptr, nv = C.c_void_p(), C.c_size_t()
    assert lib.t2d_route_vertices(pool._h, None, C.byref(nv)) == _ffi.ERR_INVALID
    assert lib.t2d_route_vertices(pool._h, C.byref(ptr), None) == _ffi.ERR_INVALID
    assert lib.t2d_route_vertices(None, C.byref(ptr), C.byref(nv)) == _ffi.ERR_INVALID
    assert lib.t2d_route_vertices(pool._h, C.byref(ptr), C.byref(nv)) == _ffi.OK and nv.value == N_ENV * CAP + 4 * (N_ENV - 1)
    with pytest.raises(ValueError):
        pool.curve_routes(words[:4], starts, 4.0, 0.5, "dubins")
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before)               # nothing was launched
    count = pool.curve_routes(words, starts, 4.0, 0.5, "dubins", 0)                  # a NULL count pointer is allowed in C; here a new tensor
    assert lib.t2d_curve_routes(pool._h, words.data_ptr(), starts.data_ptr(), 4.0, 0.5, 0, 0, None, None) == _ffi.OK
    pool.sync()
    after = pool.route_vertices().cpu().numpy()
    assert (count.cpu().numpy() > 0).all() and not np.array_equal(after, before)
    # route 1 of the sets (4 vertices each, where it exists) was not touched by writing route 0
    off = 0
    for e in range(N_ENV):
        off += CAP
        if e != 3:
            assert np.array_equal(after[off:off + 4], before[off:off + 4]), e
            off += 4
    pool.clear_routes()
    assert state_error() == _ffi.ERR_STATE
    pool.close()


def test_curve_routes_into_a_route_wider_than_the_workgroup(torch):
    """A route of 300 vertices takes the 256 lanes of a curve's workgroup a second round: straight words whose points end in the
    first round (201: the padding crosses the round's boundary), in the second (280), on the capacity (300) and past it (401),
    a word of 0 segments and three Dubins paths.  The straights run along the diagonal from (-53, -53), so every vertex stays
    below 64 m and the tolerance is the one fp32 ulp of the module's docstring."""
    from tactics2d_amd.interpolator import Dubins, pack_words
    n_env, cap, radius, step = 8, 300, 4.0, 0.5
    lengths, points = (100.1, 139.9, 149.9, 200.1), (201, 280, 300, 401)
    rng = np.random.default_rng(7)
    start = np.concatenate([rng.uniform(-10, 10, (n_env, 2)), rng.uniform(-3, 3, (n_env, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(-12, 12, (n_env, 2)), rng.uniform(-3, 3, (n_env, 1))], 1)
    start[:4] = [-53.0, -53.0, np.pi / 4]
    path = Dubins(radius, "standard").get_path(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2])
    seg, letters, n_seg = path.segments.cpu().numpy().copy(), path.steer.cpu().numpy().copy(), path.n_seg.cpu().numpy().copy()
    for e, length in enumerate(lengths):                          # envs 0 .. 3: one straight segment
        seg[e], letters[e], n_seg[e] = [length / radius, 0.0, 0.0], 0, 1
    n_seg[4] = 0                                                  # env 4: a word of 0 segments; envs 5 .. 7: Dubins paths
    pad = np.zeros((n_env, 2))
    t = lambda a, dt: torch.as_tensor(np.ascontiguousarray(a, dt), device="cuda")
    words = pack_words(t(np.concatenate([seg, pad], 1), np.float64), t(np.concatenate([letters, pad], 1), np.int8), t(n_seg, np.int32))
    z = np.zeros(n_env, np.float32)
    pool = _route_pool(z, z, z, z, n_env, 1)
    pool.set_routes([[_placeholder(e, cap)] for e in range(n_env)], np.arange(n_env), 0, 1.5)
    before = pool.route_vertices().cpu().numpy().copy().reshape(n_env, cap, 2)
    count = pool.curve_routes(words, t(start, np.float64), radius, step, "dubins", 0)
    pool.sync()
    count = count.cpu().numpy()
    verts = pool.route_vertices().cpu().numpy().reshape(n_env, cap, 2)
    want = np.zeros_like(verts)
    for e in range(n_env):
        word = (seg[e, :n_seg[e]], letters[e, :n_seg[e]], start[e], radius, step, CR.DUBINS)
        xy, _, end, _ = CR.curve_line(*word)
        assert n_seg[e] == 0 or CR.stable_count(*word), e
        assert count[e] == len(xy), e
        want[e] = CR.route_vertices(xy, end, cap, before[e])
    assert tuple(count[:4]) == points and count[4] == 0 and ((count[5:] > 0) & (count[5:] < cap)).all()
    assert np.abs(np.delete(want, 4, 0)).max() < 64.0
    assert np.array_equal(verts[4], before[4])                    # the 0-segment word's route is unchanged, bit for bit
    bit_equal, total = int((verts == want).sum()), verts.size
    print("vertices bit-equal to the fp32 rounding of the specification:", bit_equal, "of", total,
          "largest difference", np.abs(verts.astype(np.float64) - want).max())
    assert np.abs(verts.astype(np.float64) - want.astype(np.float64)).max() <= ULP32 and bit_equal >= 0.99 * total
    pool.close()


# ---- RSPlanner.write_routes ------------------------------------------------------------------------------------------------------
def test_write_routes_on_the_planner_scenes(torch):
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    from tactics2d_amd.planner import RSPlanner
    from tactics2d_amd.pool import ParticipantPool
    n_env, n_beams, cap, step = 16, 120, 160, 0.2
    case = S.planner_case(n_env, n_beams)

    def make():
        pool = ParticipantPool(n_env, 1)
        ego = vehicle_model("medium_car", "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0), steer_range=(-0.524, 0.524))
        pool.set_param_table(ego.param_row(L.SHAPE_OBB, *VEHICLE_TEMPLATE["medium_car"][:2])[None])
        pool.set_status_config()
        pool.set_target_areas(case["target"])
        pool.set_target_headings(case["target_heading"])
        z = np.zeros(n_env, np.float32)
        pool.reset(case["ego"][:, 0], case["ego"][:, 1], case["ego"][:, 2], z, np.zeros(n_env, np.int32))
        pool.lidar_config(n_beams, S.LIDAR_RANGE)
        t = np.linspace(0.0, 1.0, cap, dtype=np.float32)
        sets = [[np.stack([500.0 + 50.0 * t, 100.0 + 7.0 * e + 0.0 * t], 1).astype(np.float32)] for e in range(n_env)]
        pool.set_routes(sets, np.arange(n_env), 0, 1.0)
        planner = RSPlanner(pool, "medium_car", steer_hi=0.524)
        plan = planner.plan(torch.as_tensor(np.ascontiguousarray(case["scan"], np.float32), device="cuda"))
        return pool, planner, plan, np.concatenate([s[0] for s in sets]).reshape(n_env, cap, 2)

    def outputs(pool, planner):
        pool.sync()
        out = {f: pool.download(f).copy() for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_STATUS, L.F_REWARD)}
        out["plan"] = planner._out.cpu().numpy().view(np.uint64).copy()
        return out

    pool, planner, plan, placeholder = make()
    count = planner.write_routes(route=0, step_size=step).cpu().numpy()
    got = outputs(pool, planner)
    verts = pool.route_vertices().cpu().numpy().reshape(n_env, cap, 2)
    dist_got, _ = pool.off_route_host()
    twin, twin_planner, _, _ = make()          # the same run without the call
    ref = outputs(twin, twin_planner)
    dist_ref, _ = twin.off_route_host()
    for k in got:
        assert np.array_equal(got[k], ref[k]), k
    rec = {k: v.cpu().numpy() for k, v in plan.items()}
    found = rec["status"] == L.RS_FOUND
    kinds = np.arange(n_env) % 4
    assert found[kinds == 0].any() and found.sum() >= 4 and (~found).sum() >= 2, rec["status"]
    p = case["params"]
    worst = 0.0
    for e in range(n_env):
        if not found[e]:
            assert count[e] == 0 and np.array_equal(verts[e], placeholder[e]) and dist_got[e, 0] == dist_ref[e, 0], e
            continue
        n = int(rec["n_seg"][e])
        h = float(np.float32(case["ego"][e, 2]))
        start = np.array([float(np.float32(case["ego"][e, 0])) - p.center_shift * np.cos(h),
                          float(np.float32(case["ego"][e, 1])) - p.center_shift * np.sin(h), h])
        xy, _, end, _ = CR.curve_line(rec["distance"][e, :n] / p.radius, rec["steer"][e, :n], start, p.radius, step, CR.RS)
        assert count[e] == len(xy) and 0 < count[e], (e, count[e], len(xy))
        want = CR.route_vertices(xy, end, cap, placeholder[e])
        worst = max(worst, np.abs(verts[e].astype(np.float64) - want).max())
        assert dist_got[e, 0] < 0.5 * p.center_shift + 2.0     # the ego stands at the start of its own plan: centre_shift from the rear axle
    print("largest vertex difference from the specification:", worst, "found", int(found.sum()), "counts", count.tolist())
    assert worst <= ULP32
    pool.close()
    twin.close()
