"""t2d_spline_curves and t2d_spline_routes on the device: EVERY curve of the fixture made by running the reference
(tests/golden/splines.npz) and fresh seeded batches against the specification (tests/spline_ref.py); batch sizes around the
curves of a workgroup and point counts around the 64 lanes of a curve's wave; ragged batches; truncation with a guard region;
bad rows; every error path; a side stream; and curves written into the route sets against the specification, against a twin
pool that got the same vertices from the host, and through the profile counter.

TOL is the project's 1e-9 of tests/test_dubins.py; every operation is IEEE + - * / in the reference's order, so the expectation
is bit equality, and each test prints the largest deviation it saw.  Route vertices are the fp32 roundings of those points."""
import numpy as np
import pytest

import spline_ref as S
from route_writers import A, N_ENV, off_route as _off_route, placeholder, route_pool as _route_pool
from test_dubins import TOL
from test_splines import fixture, fixture_curve

pytestmark = pytest.mark.gpu
LANES = 64
SENTINEL = -12345.0
NAMES = {S.BEZIER: "Bezier", S.BSPLINE: "B-spline", S.CUBIC: "cubic"}


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _pad(rows, width):
    """rows of different lengths -> [n, width(, 2)] padded with a value the kernels must not read"""
    out = np.full((len(rows), width) + np.shape(rows[0])[1:], 7.0e30)
    for k, r in enumerate(rows):
        out[k, :len(r)] = r
    return out


def _raw(torch, kind, ctrl, n_ctrl, ni, degree=0, knots=None, boundary=S.NOT_A_KNOT, derivs=None, max_points=None, guard=64,
         stream=None):
    """t2d_spline_curves through the C interface into sentinel-filled buffers with a guard region behind them ->
    (rc, xy [n * max_points + guard, 2], count [n])"""
    from tactics2d_amd import _ffi
    n, m = ctrl.shape[:2]
    t = lambda v, dt=np.float64: None if v is None else torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    c, nc, kn, dv = t(ctrl), t(n_ctrl, np.int32), t(knots), t(derivs)
    rows = max(max_points, 1)
    xy = torch.full((n * rows + guard, 2), SENTINEL, dtype=torch.float64, device="cuda")
    count = torch.full((n,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = _ffi.lib().t2d_spline_curves(0, n, kind, c.data_ptr(), nc.data_ptr(), m, ni, degree, None if kn is None else kn.data_ptr(),
                                      boundary, None if dv is None else dv.data_ptr(), max_points, xy.data_ptr(), count.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, xy.cpu().numpy(), count.cpu().numpy()


def _check(xy, count, want, max_points, what):
    """device rows against the expected curves (None: count 0, nothing written); the guard untouched; -> largest deviation"""
    worst = 0.0
    for k, w in enumerate(want):
        row = xy[k * max_points:(k + 1) * max_points]
        full = 0 if w is None else len(w)
        assert count[k] == full, (what, k, count[k], full)
        c = min(full, max_points)
        if c:
            worst = max(worst, float(np.abs(row[:c] - w[:c]).max()))
        assert (row[c:] == SENTINEL).all(), (what, k)
    assert (xy[len(want) * max_points:] == SENTINEL).all(), what
    return worst


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def _fixture_launches():
    """the fixture's curves grouped into launches: one per (family, n_interpolation, degree, default knots?, boundary)"""
    g = fixture()
    groups = {}
    for c in range(len(g["kind"])):
        key = (int(g["kind"][c]), int(g["n_interpolation"][c]), int(g["degree"][c]), int(g["knot_kind"][c]) == 0, int(g["boundary"][c]))
        groups.setdefault(key, []).append(c)
    return groups


@pytest.fixture(scope="module")
def fixture_deviation(torch):
    """runs every fixture curve once; per family the largest deviation, the curves that are not bit-equal and the curves seen"""
    worst, different, seen = {k: 0.0 for k in NAMES}, {k: [] for k in NAMES}, set()
    for (kind, ni, degree, default_knots, boundary), rows in _fixture_launches().items():
        cur = [fixture_curve(c) for c in rows]
        ctrl = _pad([v[1] for v in cur], max(len(v[1]) for v in cur))
        n_ctrl = [len(v[1]) for v in cur]
        knots = None
        if kind == S.BSPLINE and not default_knots:
            knots = _pad([v[4] for v in cur], ctrl.shape[1] + degree + 1)
        derivs = np.array([v[6] for v in cur]) if kind == S.CUBIC else None
        max_points = max(len(v[7]) for v in cur)
        rc, xy, count = _raw(torch, kind, ctrl, n_ctrl, ni, degree, knots, boundary, derivs, max_points)
        assert rc == 0
        for k, c in enumerate(rows):
            want = cur[k][7]
            row = xy[k * max_points:k * max_points + len(want)]
            assert count[k] == len(want), (c, count[k], len(want))
            worst[kind] = max(worst[kind], float(np.abs(row - want).max()))
            if not np.array_equal(row, want):
                different[kind].append(c)
            assert (xy[k * max_points + len(want):(k + 1) * max_points] == SENTINEL).all(), c
            seen.add(c)
    return worst, different, seen


def test_every_fixture_curve_agrees_with_the_reference(fixture_deviation):
    worst, different, seen = fixture_deviation
    assert seen == set(range(len(fixture()["kind"])))        # none left out
    for kind in NAMES:
        print(f"{NAMES[kind]}: largest deviation from the reference {worst[kind]:.3e}, curves not bit-equal: {different[kind]}")
    assert max(worst.values()) <= TOL


def test_the_fixture_curves_are_bit_equal(fixture_deviation):
    """the expectation behind the bound: the same IEEE operations in the same order"""
    assert not any(fixture_deviation[1].values()), fixture_deviation[1]


# ---- fresh batches against the specification ---------------------------------------------------------------------------------------
def _fresh(rng, kind, n, m_lo, m_hi, degree=0):
    """n random control polygons of m_lo .. m_hi points (a cubic row's x increasing) -> (list of [m, 2], padded, n_ctrl)"""
    rows = []
    for _ in range(n):
        m = int(rng.integers(m_lo, m_hi + 1))
        p = rng.uniform(-50.0, 50.0, (m, 2))
        if kind == S.CUBIC:
            p[:, 0] = rng.uniform(-100.0, 100.0) + np.cumsum(rng.uniform(0.3, 9.0, m))
        rows.append(p)
    return rows, _pad(rows, m_hi), [len(r) for r in rows]


@pytest.mark.parametrize("kind", [S.BEZIER, S.BSPLINE, S.CUBIC], ids=["bezier", "bspline", "cubic"])
def test_fresh_ragged_batches_agree_with_the_specification(torch, kind):
    """ragged n_ctrl in one launch; batch sizes 1 and one below / one above the curves of a workgroup, and a few workgroups"""
    from tactics2d_amd import layout as L
    rng = np.random.default_rng(1000 + kind)
    per = L.SPLINE_CURVES_PER_BLOCK
    worst = 0.0
    for n in (1, per - 1, per + 1, 3 * per + 2):
        for variant in range(3):
            degree = (3, 5, 1)[variant] if kind == S.BSPLINE else 0
            boundary = (S.NOT_A_KNOT, S.NATURAL, S.CLAMPED)[variant]
            ni = (37, 64, 5)[variant]
            lo = {S.BEZIER: 2, S.BSPLINE: degree + 1, S.CUBIC: 3}[kind]
            rows, ctrl, n_ctrl = _fresh(rng, kind, n, lo, (12, 32, 7)[variant], degree)
            knots = derivs = None
            klist = [None] * n
            if kind == S.BSPLINE and variant != 1:
                klist = [np.sort(rng.uniform(0.0, 4.0, len(r) + degree + 1)) for r in rows]
                knots = _pad(klist, ctrl.shape[1] + degree + 1)
            if kind == S.CUBIC and variant != 0:
                derivs = rng.uniform(-2.0, 2.0, (n, 2))
            want = [S.curve(kind, rows[k], ni, degree, klist[k], boundary, (0.0, 0.0) if derivs is None else derivs[k]) for k in range(n)]
            max_points = max(len(w) for w in want)
            rc, xy, count = _raw(torch, kind, ctrl, n_ctrl, ni, degree, knots, boundary, derivs, max_points)
            assert rc == 0
            worst = max(worst, _check(xy, count, want, max_points, (n, variant)))
    print(f"{NAMES[kind]}: largest deviation from the specification on fresh batches {worst:.3e}")
    assert worst <= TOL


def test_point_counts_around_the_lane_count(torch):
    rng = np.random.default_rng(5)
    worst = 0.0
    for ni in (LANES - 1, LANES, LANES + 1, 2 * LANES, 2 * LANES + 1):
        for kind in (S.BEZIER, S.BSPLINE):
            rows, ctrl, n_ctrl = _fresh(rng, kind, 3, 6, 6)
            want = [S.curve(kind, r, ni, 3) for r in rows]
            rc, xy, count = _raw(torch, kind, ctrl, n_ctrl, ni, 3, max_points=ni)
            assert rc == 0 and count.tolist() == [ni] * 3
            worst = max(worst, _check(xy, count, want, ni, (kind, ni)))
    for ni, m in ((31, 3), (32, 3), (21, 4), (63, 2 + 1), (64, 3), (9, 8)):      # cubic counts 63, 65, 64, 127, 129, 64
        rows, ctrl, n_ctrl = _fresh(rng, S.CUBIC, 3, m, m)
        want = [S.curve(S.CUBIC, r, ni, boundary=S.NATURAL) for r in rows]
        total = (m - 1) * ni + 1
        rc, xy, count = _raw(torch, S.CUBIC, ctrl, n_ctrl, ni, boundary=S.NATURAL, max_points=total)
        assert rc == 0 and count.tolist() == [total] * 3
        worst = max(worst, _check(xy, count, want, total, ("cubic", ni, m)))
    assert worst <= TOL


def test_truncation_reports_the_full_count_and_leaves_the_tail_untouched(torch):
    rng = np.random.default_rng(6)
    for kind, ni, full in ((S.BEZIER, 70, 70), (S.BSPLINE, 70, 70), (S.CUBIC, 23, 70)):
        rows, ctrl, n_ctrl = _fresh(rng, kind, 3, 4, 4)
        want = [S.curve(kind, r, ni, 2) for r in rows]
        assert all(len(w) == full for w in want)
        for max_points in (1, 63, 64, 65, 69, 70, 90):
            rc, xy, count = _raw(torch, kind, ctrl, n_ctrl, ni, 2, max_points=max_points)
            assert rc == 0 and count.tolist() == [full] * 3, (kind, max_points)
            assert _check(xy, count, want, max_points, (kind, max_points)) <= TOL


def test_bad_rows_touch_only_their_own_outputs(torch):
    rng = np.random.default_rng(7)
    n, m = 10, 8
    for kind, degree, lo in ((S.BEZIER, 0, 2), (S.BSPLINE, 3, 4), (S.CUBIC, 0, 3)):
        rows, ctrl, n_ctrl = _fresh(rng, kind, n, m, m)
        n_ctrl = np.array(n_ctrl)
        knots = np.sort(rng.uniform(0.0, 4.0, (n, m + degree + 1)), 1) if kind == S.BSPLINE else None
        derivs = rng.uniform(-1.0, 1.0, (n, 2)) if kind == S.CUBIC else None
        boundary = S.CLAMPED
        rc, xy0, count0 = _raw(torch, kind, ctrl, n_ctrl, 20, degree, knots, boundary, derivs, 200)
        assert rc == 0 and (count0 > 0).all()
        bad = [0, 2, 3, 5, 9]
        n_ctrl[0] = lo - 1                 # below the family's minimum
        n_ctrl[2] = m + 1                  # above max_ctrl
        ctrl[3, 1, 1] = np.nan             # a control point that is not finite
        ctrl[5, 4, 0] = -np.inf
        if kind == S.BEZIER:
            n_ctrl[9] = 0
        elif kind == S.BSPLINE:
            knots[9, 5] = knots[9, 4] - 0.5    # knots that decrease
            knots[7, 2] = np.inf               # a knot that is not finite
            bad.append(7)
        else:
            ctrl[9, 6, 0] = ctrl[9, 5, 0]      # x that does not increase (a tie)
            derivs[7, 1] = np.nan              # a clamped derivative that is not finite
            bad.append(7)
        rc, xy, count = _raw(torch, kind, ctrl, n_ctrl, 20, degree, knots, boundary, derivs, 200)
        assert rc == 0
        for k in range(n):
            row = slice(k * 200, (k + 1) * 200)
            if k in bad:
                assert count[k] == 0 and (xy[row] == SENTINEL).all(), (kind, k)
            else:
                assert count[k] == count0[k] and np.array_equal(xy[row], xy0[row]), (kind, k)
        assert (xy[n * 200:] == SENTINEL).all()
    # a short row reads nothing past its own points: the padding of a ragged batch may hold anything
    rows, ctrl, n_ctrl = _fresh(rng, S.CUBIC, 4, 3, 9)
    ctrl[np.arange(9)[None, :] >= np.array(n_ctrl)[:, None]] = np.nan
    rc, xy, count = _raw(torch, S.CUBIC, ctrl, n_ctrl, 10, max_points=100)
    assert rc == 0 and _check(xy, count, [S.cubic(r, n_interpolation=10) for r in rows], 100, "padding") <= TOL
    # derivatives are read under Clamped only
    d = np.full((4, 2), np.nan)
    rc, xy2, count2 = _raw(torch, S.CUBIC, ctrl, n_ctrl, 10, derivs=d, max_points=100)
    assert rc == 0 and np.array_equal(count2, count) and np.array_equal(xy2, xy)


def test_every_invalid_launch_is_refused_and_launches_nothing(torch):
    from tactics2d_amd import _ffi, layout as L
    ctrl = np.cumsum(np.ones((2, 6, 2)), 1)
    ok = dict(kind=S.CUBIC, ni=10, degree=0, boundary=S.NATURAL, max_points=64)
    for kw in (dict(kind=3), dict(kind=-1), dict(kind=S.BEZIER, ni=1), dict(kind=S.BSPLINE, ni=0), dict(kind=S.CUBIC, ni=1),
               dict(kind=S.CUBIC, boundary=0), dict(kind=S.CUBIC, boundary=4), dict(kind=S.BSPLINE, degree=-1),
               dict(kind=S.BSPLINE, degree=L.SPLINE_MAX_DEGREE + 1), dict(max_points=0), dict(max_points=-5)):
        a = dict(ok)
        a.update(kw)
        rc, xy, count = _raw(torch, a["kind"], ctrl, [6, 6], a["ni"], a["degree"], None, a["boundary"], None, a["max_points"])
        assert rc == _ffi.ERR_INVALID, kw
        assert (xy == SENTINEL).all() and (count == -7).all(), kw          # nothing was launched
    rc, xy, count = _raw(torch, S.BEZIER, np.zeros((1, L.SPLINE_MAX_CTRL + 1, 2)), [4], 10, max_points=16)     # max_ctrl above the cap
    assert rc == _ffi.ERR_INVALID and (xy == SENTINEL).all()
    lib = _ffi.lib()
    buf = torch.zeros(256, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    call = lambda n=1, kind=S.BSPLINE, c=p, nc=p, m=4, kn=p, dv=p, xy=p, cnt=p: \
        lib.t2d_spline_curves(0, n, kind, c, nc, m, 10, 2, kn, S.CLAMPED, dv, 16, xy, cnt, None)
    assert call(n=-1) == _ffi.ERR_INVALID and call(m=0) == _ffi.ERR_INVALID
    for null in ("c", "nc", "xy", "cnt"):
        assert call(**{null: None}) == _ffi.ERR_INVALID, null
    assert call(c=p + 8) == _ffi.ERR_INVALID and call(xy=p + 8) == _ffi.ERR_INVALID           # 16-byte alignment
    assert call(nc=p + 2) == _ffi.ERR_INVALID and call(cnt=p + 2) == _ffi.ERR_INVALID         # 4-byte alignment
    assert call(kn=p + 4) == _ffi.ERR_INVALID and call(kind=S.CUBIC, dv=p + 4) == _ffi.ERR_INVALID
    assert call(n=0) == _ffi.OK
    torch.cuda.synchronize()
    assert (buf == 0).all()


def test_the_classes_on_a_side_stream_and_with_their_defaults(torch):
    from tactics2d_amd.interpolator import Bezier, BSpline, CubicSpline
    rng = np.random.default_rng(8)
    rows, ctrl, n_ctrl = _fresh(rng, S.CUBIC, 5, 6, 6)
    side = torch.cuda.Stream()
    dev = torch.as_tensor(ctrl, device="cuda")
    torch.cuda.synchronize()
    b = Bezier.get_curve(dev, 50, stream=side)                                  # a CUDA tensor, read in place
    assert b._inputs[0].data_ptr() == dev.data_ptr()
    s = BSpline.get_curve(ctrl, degree=3, stream=side)                          # numpy, the default knots, 100 points
    c = CubicSpline.get_curve(dev, stream=side)                                 # not-a-knot, 100 per segment
    k = CubicSpline.get_curve(ctrl, (0.5, -0.25), 20, CubicSpline.BoundaryType.Clamped, n_ctrl=np.array([6, 5, 4, 3, 6]), stream=side)
    one = Bezier.get_curve(ctrl[0], 11)                                         # [m, 2]: a batch of one, the current stream
    side.synchronize()
    torch.cuda.synchronize()
    assert tuple(b.xy.shape) == (5, 50, 2) and tuple(s.xy.shape) == (5, 100, 2) and tuple(c.xy.shape) == (5, 501, 2)
    assert tuple(one.xy.shape) == (1, 11, 2) and one.count.tolist() == [11] and k.count.tolist() == [101, 81, 61, 41, 101]
    worst = 0.0
    for e in range(5):
        worst = max(worst, np.abs(b.xy[e].cpu().numpy() - S.bezier(rows[e], 50)).max(),
                    np.abs(s.xy[e].cpu().numpy() - S.bspline(rows[e], None, 3, 100)).max(),
                    np.abs(c.xy[e].cpu().numpy() - S.cubic(rows[e], (0.0, 0.0), 100, S.NOT_A_KNOT)).max())
        want = S.cubic(rows[e][:(6, 5, 4, 3, 6)[e]], (0.5, -0.25), 20, S.CLAMPED)
        worst = max(worst, np.abs(k.xy[e, :len(want)].cpu().numpy() - want).max())
    assert worst <= TOL and np.abs(one.xy[0].cpu().numpy() - S.bezier(rows[0], 11)).max() <= TOL
    # device tensors: the data-dependent refusals become count 0
    bad = dev.clone()
    bad[2, 3, 0] = bad[2, 2, 0]
    assert CubicSpline.get_curve(bad, n_interpolation=5).count.tolist() == [26, 26, 0, 26, 26]
    knots = torch.linspace(0, 1, 10, dtype=torch.float64, device="cuda").repeat(5, 1)
    knots[4, 7] = 0.0
    assert BSpline.get_curve(dev, knots, 3, 9).count.tolist() == [9, 9, 9, 9, 0]


# ---- curves as routes --------------------------------------------------------------------------------------------------------------
CAPS = (40, 61, 61, 90, 61, 61, 33, 120)     # route capacities below, equal to and above the 61 points of a curve


def _routes_against_the_specification_and_a_twin_pool(kind, caps, no_curve):
    """one curve per env of a pool of len(caps) envs into routes of these capacities; env `no_curve` (None: no env) has no curve"""
    from tactics2d_amd import layout as L
    n_env = len(caps)
    rng = np.random.default_rng(40 + kind)
    m = 5
    ni = 15 if kind == S.CUBIC else 61                                    # 61 points per curve either way
    rows, ctrl, n_ctrl = _fresh(rng, kind, n_env, m, m)
    for r in rows:                                                        # roads of some tens of metres near the origin
        r[:, 0] = np.linspace(-20.0, 20.0, m) + rng.uniform(-2.0, 2.0, m)
        r[:, 1] = rng.uniform(-6.0, 6.0, m)
    ctrl = np.stack(rows)
    n_ctrl = np.full(n_env, m, np.int32)
    if no_curve is not None:
        n_ctrl[no_curve] = 1 if kind != S.BSPLINE else 2
    live = [e for e in range(n_env) if e != no_curve]
    kw = dict(n_interpolation=ni, degree=3, boundary_type=S.CLAMPED, first_derivatives=np.tile([0.3, -0.2], (n_env, 1)))
    want_xy = [None if e == no_curve else S.curve(kind, rows[e], ni, 3, None, S.CLAMPED, (0.3, -0.2)) for e in range(n_env)]
    x = np.repeat(np.linspace(-15.0, 15.0, A)[None], n_env, 0).astype(np.float32).ravel()
    y = rng.uniform(-5.0, 5.0, n_env * A).astype(np.float32)
    z = np.zeros(n_env * A, np.float32)
    sets = [[placeholder(caps[e], e)] for e in range(n_env)]
    pool = _route_pool(x, y, z, z, n_env)
    pool.set_routes(sets, np.arange(n_env), 0, 1.5)
    before = pool.route_vertices().cpu().numpy().copy()
    pool.profile_enable(True)
    count = pool.spline_routes(kind, ctrl, n_ctrl, route=0, **kw)
    pool.sync()
    assert pool.profile_read(L.PROFILE_SPLINE_ROUTES)[1] == 1 and pool.profile_read(L.PROFILE_CURVE_ROUTES)[1] == 0
    pool.profile_enable(False)
    count = count.cpu().numpy()
    verts = pool.route_vertices().cpu().numpy()
    off = np.concatenate([[0], np.cumsum(caps)])
    equal = total = 0
    for e in range(n_env):
        got = verts[off[e]:off[e + 1]]
        if e == no_curve:
            assert count[e] == 0 and np.array_equal(got, before[off[e]:off[e + 1]])         # untouched, bit for bit
            continue
        assert count[e] == 61, e
        want = S.route_vertices(want_xy[e], caps[e])
        equal, total = equal + int((got == want).sum()), total + got.size
        assert np.abs(got.astype(np.float64) - want).max() <= 2.0 ** -18, e               # one fp32 ulp below 32 m
        if caps[e] > 61:                                                                  # the padding rule: the last written point
            assert (got[61:] == got[60]).all(), e
    print(f"{NAMES[kind]}: route vertices bit-equal to the fp32 rounding of the specification: {equal} of {total}")
    assert equal == total
    got = _off_route(pool)
    twin = _route_pool(x, y, z, z, n_env)
    twin.set_routes([[verts[off[e]:off[e + 1]]] for e in range(n_env)], np.arange(n_env), 0, 1.5)
    ref = _off_route(twin)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1])
    d = got[0].reshape(n_env, A)
    assert np.isfinite(d).all() and (d[live] < 30.0).all() and (no_curve is None or (d[no_curve] > 100.0).all())
    pool.close()
    twin.close()


@pytest.mark.parametrize("kind", [S.BEZIER, S.BSPLINE, S.CUBIC], ids=["bezier", "bspline", "cubic"])
def test_spline_routes_against_the_specification_and_a_twin_pool(torch, kind):
    _routes_against_the_specification_and_a_twin_pool(kind, CAPS, 5)


@pytest.mark.parametrize("no_curve", [None, 4], ids=["env4_alone", "no_writer"])
@pytest.mark.parametrize("kind", [S.BEZIER, S.BSPLINE, S.CUBIC], ids=["bezier", "bspline", "cubic"])
def test_spline_routes_of_a_pool_that_ends_inside_a_workgroup(torch, kind, no_curve):
    """5 envs, four curves to a workgroup: env 4 is the only live wave of the last workgroup, whose three idle waves keep the
    barriers; without a curve in env 4 that workgroup has no writer at all"""
    _routes_against_the_specification_and_a_twin_pool(kind, (40, 61, 90, 33, 120), no_curve)


def test_spline_routes_error_paths(torch):
    from tactics2d_amd import _ffi
    z = np.zeros(N_ENV * A, np.float32)
    pool = _route_pool(z, z, z, z)
    ctrl = torch.as_tensor(np.cumsum(np.ones((N_ENV, 4, 2)), 1), device="cuda")
    n_ctrl = torch.full((N_ENV,), 4, dtype=torch.int32, device="cuda")
    lib = _ffi.lib()

    def code(kind=S.CUBIC, ni=10, degree=0, boundary=S.NATURAL, route=0, c=ctrl.data_ptr(), nc=n_ctrl.data_ptr(), m=4, h=pool._h):
        return lib.t2d_spline_routes(h, kind, c, nc, m, ni, degree, None, boundary, None, route, None, None)

    assert code() == _ffi.ERR_STATE                                                   # no routes installed
    pool.set_routes([[placeholder(CAPS[0], 0)]], None, 0, 1.0)                        # one set shared by every env
    assert code() == _ffi.ERR_STATE
    sets = [[placeholder(CAPS[e], e)] + ([placeholder(CAPS[e], e)[:4]] if e != 3 else []) for e in range(N_ENV)]
    pool.set_routes(sets, np.arange(N_ENV), 0, 1.0)
    before = pool.route_vertices().cpu().numpy().copy()
    assert code(route=1) == _ffi.ERR_STATE and code(route=2) == _ffi.ERR_STATE        # env 3's set has no route 1
    for kw in (dict(kind=5), dict(ni=1), dict(kind=S.BSPLINE, ni=0), dict(kind=S.BEZIER, ni=1), dict(boundary=0), dict(kind=S.BSPLINE, degree=-1),
               dict(kind=S.BSPLINE, degree=6), dict(route=-1), dict(m=0), dict(m=33), dict(c=None), dict(nc=None),
               dict(c=ctrl.data_ptr() + 8), dict(h=None)):
        assert code(**kw) == _ffi.ERR_INVALID, kw
    with pytest.raises(_ffi.T2DError) as ei:
        pool.spline_routes("cubic", ctrl, route=1)
    assert ei.value.code == _ffi.ERR_STATE
    with pytest.raises(ValueError):
        pool.spline_routes("cubic", ctrl[:4])
    with pytest.raises(ValueError):
        pool.spline_routes("cubic", ctrl, count=torch.zeros(3, dtype=torch.int32, device="cuda"))
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before)                # nothing was launched
    assert code() == _ffi.OK                                                          # a NULL count pointer is allowed
    count = pool.spline_routes("bezier", ctrl, n_interpolation=30)
    pool.sync()
    after = pool.route_vertices().cpu().numpy()
    assert count.tolist() == [30] * N_ENV and not np.array_equal(after, before)
    off = 0
    for e in range(N_ENV):                                                            # route 1 of the sets was not touched
        off += CAPS[e]
        if e != 3:
            assert np.array_equal(after[off:off + 4], before[off:off + 4]), e
            off += 4
    pool.clear_routes()
    assert code() == _ffi.ERR_STATE
    pool.close()
