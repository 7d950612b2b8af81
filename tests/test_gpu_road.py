"""fresnel_det, t2d_spiral_curves, t2d_param_poly3_curves, t2d_planview_lines and t2d_planview_routes on the device: the Fresnel
integrals through the debug hook against the specification (tests/road_ref.py) and mpmath; EVERY curve and road of the fixture
made by running the reference (tests/golden/road.npz); fresh seeded batches against the specification at the shapes where the
kernels can go wrong -- point counts around the 64 lanes of a wave, batch sizes around the curves of a workgroup, roads of 1, 2
and T2D_PLANVIEW_MAX_GEOM geometries, a seam duplicate on lane 0 and on lane 63 of a pass, a line that crosses max_points with a
guard region behind every buffer --; bad rows between good ones; every error path; a side stream; and roads written into the
route sets against the specification, against a twin pool that got the same vertices from the host, through the profile counter
and under pure-pursuit cars in closed loop.

TOL is the project's 1e-9 of tests/test_dubins.py (derived in tests/test_road.py).  The device outputs the kept points, not the
keep mask: equal counts and kept points within TOL of the fixture's raw[keep] ARE the equal mask, because the fixture keeps every
raw distance 1e-6 away from the filter's 0.02."""
import numpy as np
import pytest

import road_ref as R
from route_writers import A, N_ENV, off_route as _off_route, placeholder as _placeholder, route_pool as _route_pool
from test_dubins import TOL
from test_road import fresnel_grid, largest_error, mp_fresnel

pytestmark = pytest.mark.gpu
SENTINEL = -12345.0
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def golden():
    return R.fixture()


# ---- the Fresnel integrals -------------------------------------------------------------------------------------------------------
def test_fresnel_det_equals_the_specification_and_meets_the_mpmath_bound():
    import scipy.special
    from tactics2d_amd import debug as dev
    x = fresnel_grid()
    es, ec = mp_fresnel(x)
    S, C = dev.math("fresnel", x)
    rs, rc = R.fresnel(x)
    ulps = max(float((np.abs(S - rs) / np.spacing(np.abs(rs))).max()), float((np.abs(C - rc) / np.spacing(np.abs(rc))).max()))
    ss, sc = scipy.special.fresnel(x)
    in60 = x <= 60.0
    bound_s = 2.0 * largest_error(ss[in60], [e for e, k in zip(es, in60) if k])
    bound_c = 2.0 * largest_error(sc[in60], [e for e, k in zip(ec, in60) if k])
    err_s, err_c = largest_error(S, es), largest_error(C, ec)
    print(f"fresnel_det on {len(x)} points: largest deviation from the specification {ulps} ulp; largest error S {err_s:.3e} C {err_c:.3e}; "
          f"twice scipy's on [0, 60]: S {bound_s:.3e} C {bound_c:.3e}")
    assert ulps <= 2.0 and err_s <= bound_s and err_c <= bound_c
    # odd, saturating, NaN for NaN; negative arguments share waves with positive ones
    y = np.concatenate([-x[:300], [-0.0, np.inf, -np.inf, np.nan, -2.0 ** 53], x[:59]])
    S, C = dev.math("fresnel", y)
    rs, rc = R.fresnel(y)
    assert np.array_equal(S, rs, equal_nan=True) and np.array_equal(C, rc, equal_nan=True)
    assert S[300:305].tolist()[:3] == [-0.0, 0.5, -0.5] and np.signbit(S[300]) and np.isnan(S[303]) and np.isnan(C[303]) and C[304] == -0.5


# ---- the C interface into guarded buffers ------------------------------------------------------------------------------------------
def _dev(torch, a, dt=np.float64):
    return torch.as_tensor(np.ascontiguousarray(a, dt), device="cuda")


def _buffers(torch, n, max_points, planes):
    rows = max(max_points, 1)
    out = [torch.full((n * rows + GUARD,) + p, SENTINEL, dtype=torch.float64, device="cuda") for p in planes]
    count = torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    return out, count


def _spirals(torch, par, ni, rule, max_points, stream=None):
    from tactics2d_amd import _ffi
    p = _dev(torch, par)
    (xy,), count = _buffers(torch, len(par), max_points, [(2,)])
    rc = _ffi.lib().t2d_spiral_curves(0, len(par), p.data_ptr(), ni, rule, max_points, xy.data_ptr(), count.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, xy.cpu().numpy(), count.cpu().numpy()


def _pp3(torch, par, p_range, max_points):
    from tactics2d_amd import _ffi
    p, r = _dev(torch, par), _dev(torch, p_range, np.int32)
    (xy,), count = _buffers(torch, len(par), max_points, [(2,)])
    rc = _ffi.lib().t2d_param_poly3_curves(0, len(par), p.data_ptr(), r.data_ptr(), max_points, xy.data_ptr(), count.data_ptr(), None)
    torch.cuda.synchronize()
    return rc, xy.cpu().numpy(), count.cpu().numpy()


def _records(roads, max_geom, n_geom=None):
    """specification geometry dicts -> (records f64 [n, max_geom, 14], n_geom i32 [n]); unused slots hold values the kernel must
    not read"""
    rec = np.full((len(roads), max_geom, 14), 7.0e30)
    head = rec.view(np.int32).reshape(len(roads), max_geom, 28)
    head[:, :, :2] = 99
    for e, road in enumerate(roads):
        for i, g in enumerate(road):
            names = R.PAR_NAMES.get(g["kind"], ())
            head[e, i, 0], head[e, i, 1] = g["kind"], g.get("pRange", 0)
            rec[e, i, 1:6] = [g[k] for k in ("s", "x", "y", "hdg", "length")]
            rec[e, i, 6:6 + len(names)] = [g[k] for k in names]
    return rec, np.array([len(r) for r in roads] if n_geom is None else n_geom, np.int32)


def _lines(torch, rec, n_geom, rule, max_points, stream=None, planes=(True, True)):
    from tactics2d_amd import _ffi
    r, g = _dev(torch, rec), _dev(torch, n_geom, np.int32)
    n = len(rec)
    (xy, s, kappa), count = _buffers(torch, n, max_points, [(2,), (), ()])
    rc = _ffi.lib().t2d_planview_lines(0, n, r.data_ptr(), g.data_ptr(), rec.shape[1], rule, max_points, xy.data_ptr(),
                                       s.data_ptr() if planes[0] else None, kappa.data_ptr() if planes[1] else None, count.data_ptr(), stream)
    torch.cuda.synchronize()
    return rc, xy.cpu().numpy(), s.cpu().numpy(), kappa.cpu().numpy(), count.cpu().numpy()


def _check(xy, count, want, max_points, what, extra=()):
    """device rows against the expected curves (None: count 0, nothing written); the guards untouched; -> largest deviation.
    extra: (device plane, [expected row or None]) pairs laid out like xy (s, kappa)"""
    worst = 0.0
    assert (count[len(want):] == -7).all(), what
    for plane, rows in ((xy, want),) + tuple(extra):
        for k, w in enumerate(rows):
            row = plane[k * max_points:(k + 1) * max_points]
            full = 0 if w is None else len(w)
            assert count[k] == full, (what, k, count[k], full)
            c = min(full, max_points)
            if c:
                worst = max(worst, float(np.abs(row[:c] - w[:c]).max()))
            assert (row[c:] == SENTINEL).all(), (what, k)
        assert (plane[len(rows) * max_points:] == SENTINEL).all(), what
    return worst


def _road_rows(roads, rule=R.REFERENCE, max_geom=64):
    got = [R.planview(r, rule, max_geom) for r in roads]
    none = lambda g, k: g[k] if g["count"] else None
    return [none(g, "xy") for g in got], [none(g, "s") for g in got], [none(g, "kappa") for g in got]


# ---- the fixture -------------------------------------------------------------------------------------------------------------------
def test_every_fixture_spiral_and_param_poly3(torch, golden):
    z, spirals, pp3, roads = golden
    worst = 0.0
    for n in sorted(set(z["spiral_n"].tolist())):
        rows = [i for i, s in enumerate(spirals) if s[1] == n]
        rc, xy, count = _spirals(torch, z["spiral_par"][rows], n, R.REFERENCE, n)
        assert rc == 0
        worst = max(worst, _check(xy, count, [spirals[i][2] for i in rows], n, f"spirals of {n} points"))
    print("Spiral against the fixture: largest deviation", worst)
    assert worst <= TOL
    mp = int(z["pp3_count"].max())
    rc, xy, count = _pp3(torch, z["pp3_par"], z["pp3_range"], mp)
    assert rc == 0
    worst = _check(xy, count, [c[2] for c in pp3], mp, "paramPoly3")
    print("ParamPoly3 against the fixture: largest deviation", worst)
    assert worst <= TOL


def test_every_fixture_road(torch, golden):
    from tactics2d_amd import interpolator as I
    z, spirals, pp3, roads = golden
    want = [r["xy"] if r["count"] else None for r in roads], [r["s"] if r["count"] else None for r in roads], \
           [r["kappa"] if r["count"] else None for r in roads]
    rec, n_geom = _records([r["geoms"] for r in roads], 6)
    mp = int(z["road_count"].max()) + 3
    rc, xy, s, kappa, count = _lines(torch, rec, n_geom, R.REFERENCE, mp)
    assert rc == 0 and count[:len(roads)].tolist() == z["road_count"].tolist()
    worst = _check(xy, count, want[0], mp, "fixture roads", ((s, want[1]), (kappa, want[2])))
    print("plan-view lines against the fixture: largest deviation (xy, s, kappa)", worst)
    assert worst <= TOL
    # the same roads through pack_planview and planview_lines, with the bound of max_points computed from the lengths
    names = {v: k for k, v in I.GEOMETRY_KINDS.items()}
    packed = [[dict({k: v for k, v in g.items() if k in ("s", "x", "y", "hdg", "length")},
                    **{names[g["kind"]]: dict({k: g[k] for k in R.PAR_NAMES[g["kind"]]}, pRange="arcLength" if g["pRange"] else "normalized")})
               for g in r["geoms"]] for r in roads]
    records, ng = I.pack_planview(packed)
    assert ng.tolist() == n_geom.tolist() and all(np.array_equal(records.numpy()[e, :g, :6].view(np.int64), rec[e, :g, :6].view(np.int64)) for e, g in enumerate(n_geom))
    out = I.planview_lines(records, ng)
    torch.cuda.synchronize()
    assert out.count.cpu().tolist() == z["road_count"].tolist() and out.xy.shape[1] >= z["road_raw"].max()
    for e, r in enumerate(roads):
        c = r["count"]
        assert c == 0 or np.abs(out.xy[e, :c].cpu().numpy() - r["xy"]).max() <= TOL


# ---- fresh batches at the shapes where the kernels can go wrong ------------------------------------------------------------------
def _fresh_spirals(rng, n):
    par = np.stack([rng.uniform(0.5, 60.0, n), rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(-np.pi, np.pi, n),
                    rng.choice([0.0, 0.03, -0.05], n) * rng.uniform(0.5, 1.5, n), rng.choice([0.0, 0.01, -0.02], n) * rng.uniform(0.5, 1.5, n)], 1)
    return par


@pytest.mark.parametrize("rule", [R.REFERENCE, R.STANDARD], ids=["reference", "standard"])
def test_fresh_spirals_around_the_lanes_of_a_wave_and_the_curves_of_a_workgroup(torch, rule):
    from tactics2d_amd import layout as L
    rng = np.random.default_rng(21 + rule)
    per, worst = L.ROAD_CURVES_PER_BLOCK, 0.0
    for ni in (1, 2, 63, 64, 65, 129):
        for n in (1, per - 1, per, per + 1):
            par = _fresh_spirals(rng, n)
            rc, xy, count = _spirals(torch, par, ni, rule, ni)
            assert rc == 0
            worst = max(worst, _check(xy, count, [R.spiral(*p, ni, rule) for p in par], ni, (ni, n)))
    par = _fresh_spirals(rng, 37)                                   # truncation: count holds the full count
    rc, xy, count = _spirals(torch, par, 100, rule, 70)
    worst = max(worst, _check(xy, count, [R.spiral(*p, 100, rule) for p in par], 70, "truncated"))
    print("fresh spirals: largest deviation", worst)
    assert worst <= TOL


def test_fresh_param_poly3_ragged_and_truncated(torch):
    rng = np.random.default_rng(23)
    n = 9
    lengths = np.array([0.0, 0.15, 0.25, 6.29, 6.31, 6.41, 12.85, 12.95, 3.33])     # counts 2, 2, 2, 62, 63, 64, 128, 129, 33
    k = np.where(np.arange(n) % 2 == 1, 1.0, np.maximum(lengths, 1.0))
    par = np.concatenate([np.stack([lengths, rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(-np.pi, np.pi, n)], 1),
                          np.stack([rng.uniform(-1, 1, n), k, rng.uniform(-0.03, 0.03, n) * k ** 2, rng.uniform(-0.003, 0.003, n) * k ** 3,
                                    rng.uniform(-1, 1, n), rng.uniform(-0.2, 0.2, n) * k, rng.uniform(-0.03, 0.03, n) * k ** 2,
                                    rng.uniform(-0.003, 0.003, n) * k ** 3], 1)], 1)
    p_range = (np.arange(n) % 2).astype(np.int32)
    want = [R.param_poly3(p[0], p[1], p[2], p[3], p[4:], r) for p, r in zip(par, p_range)]
    assert [len(w) for w in want] == [2, 2, 2, 62, 63, 64, 128, 129, 33]
    worst = 0.0
    for mp in (129, 64, 1):
        rc, xy, count = _pp3(torch, par, p_range, mp)
        assert rc == 0
        worst = max(worst, _check(xy, count, want, mp, mp))
    print("fresh paramPoly3: largest deviation", worst)
    assert worst <= TOL


def _draw(rng, kind, s, x, y, hdg, length):
    g = dict(kind=kind, s=s, x=x, y=y, hdg=hdg, length=length, pRange=0)
    if kind == R.SPIRAL:
        g.update(curvStart=float(rng.choice([0.0, 0.04, -0.03])), curvEnd=float(rng.uniform(-0.1, 0.1)))
    elif kind == R.ARC:
        g.update(curvature=float(rng.choice([-1, 1]) * rng.uniform(0.01, 0.2)))
    elif kind == R.POLY3:
        g.update(a=0.0, b=float(rng.uniform(-0.1, 0.1)), c=float(rng.uniform(-0.02, 0.02)), d=float(rng.uniform(-0.002, 0.002)))
    elif kind == R.PARAM_POLY3:
        arc = int(rng.integers(0, 2))
        k = 1.0 if arc else length
        g.update(aU=0.0, bU=k, cU=float(rng.uniform(-0.02, 0.02)) * k * k, dU=float(rng.uniform(-0.002, 0.002)) * k ** 3, aV=0.0,
                 bV=float(rng.uniform(-0.05, 0.05)) * k, cV=float(rng.uniform(-0.02, 0.02)) * k * k,
                 dV=float(rng.uniform(-0.002, 0.002)) * k ** 3, pRange=arc)
    return g


def _chain(rng, kinds, lengths=None, rule=R.REFERENCE):
    """a road whose geometries each start on the last sampled point of the one before (so every seam repeats a point exactly)"""
    road, s, x, y, hdg = [], 0.0, float(rng.uniform(-50, 50)), float(rng.uniform(-50, 50)), float(rng.uniform(-np.pi, np.pi))
    for i, kind in enumerate(kinds):
        length = float(rng.uniform(1.03, 7.97)) if lengths is None else lengths[i]
        g = _draw(rng, kind, s, x, y, hdg, length)
        road.append(g)
        xy = R.sample_geometry(g, rule)[0]
        if len(xy):
            x, y = float(xy[-1, 0]), float(xy[-1, 1])
        s, hdg = s + length, hdg + float(rng.uniform(-0.2, 0.2))
    return road


def _stable(roads, rule):
    """no keep decision of these roads within 1e-6 of the filter's threshold"""
    for r in roads:
        raw = R.planview(r, rule)["raw"]
        d = np.diff(raw, axis=0)
        if np.any(np.abs(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) - 0.02) < 1e-6):
            return False
    return True


@pytest.mark.parametrize("rule", [R.REFERENCE, R.STANDARD], ids=["reference", "standard"])
def test_fresh_roads_of_one_two_and_max_geom_geometries(torch, rule):
    from tactics2d_amd import layout as L
    per, G = L.ROAD_CURVES_PER_BLOCK, L.PLANVIEW_MAX_GEOM
    worst = 0.0
    for seed, (n, n_g) in enumerate([(1, [1]), (per - 1, [2, 1, G]), (per, [G, 2, 1, 5]), (per + 1, [3, G, 1, 2, 4])]):
        rng = np.random.default_rng(300 + 10 * seed + rule)
        for _ in range(50):
            roads = [_chain(rng, rng.integers(0, 5, g).tolist(), rule=rule) for g in n_g]
            if _stable(roads, rule):
                break
        rec, n_geom = _records(roads, G)
        want = _road_rows(roads, rule)
        mp = max(len(w) for w in want[0])
        rc, xy, s, kappa, count = _lines(torch, rec, n_geom, rule, mp)
        assert rc == 0
        worst = max(worst, _check(xy, count, want[0], mp, n_g, ((s, want[1]), (kappa, want[2]))))
    print("fresh roads: largest deviation", worst)
    assert worst <= TOL


def test_a_seam_duplicate_on_lane_0_and_on_lane_63_of_a_pass(torch):
    rng = np.random.default_rng(31)
    # a first line of 64 raw points puts the next geometry's first point -- a duplicate -- on lane 0 of the second pass; one of 63
    # puts it on lane 63 of the first; 127 / 128: the same one pass later.  Behind each seam, every kind.
    roads, seams = [], []
    for first, points in ((6.35, 64), (6.25, 63), (12.75, 128), (12.65, 127)):
        for kind in range(5):
            road = _chain(rng, [R.LINE, kind, R.ARC], [first, 3.37, 2.21])
            assert len(R.sample_geometry(road[0])[0]) == points
            roads.append(road)
            seams.append(points)
    assert _stable(roads, R.REFERENCE)
    for road, k in zip(roads, seams):
        got = R.planview(road)
        assert not got["keep"][k] and np.abs(got["raw"][k] - got["raw"][k - 1]).max() < 1e-12 and got["keep"][k - 1] and got["keep"][k + 1]   # (an arc's first point is its start only to an ulp)
    rec, n_geom = _records(roads, 3)
    want = _road_rows(roads)
    mp = max(len(w) for w in want[0])
    rc, xy, s, kappa, count = _lines(torch, rec, n_geom, R.REFERENCE, mp)
    worst = _check(xy, count, want[0], mp, "seams", ((s, want[1]), (kappa, want[2])))
    print("seam duplicates on lane 0 / lane 63: largest deviation", worst)
    assert rc == 0 and worst <= TOL


def test_a_line_that_crosses_max_points_and_the_optional_planes(torch):
    rng = np.random.default_rng(33)
    roads = [_chain(rng, [R.LINE, R.ARC, R.POLY3], [7.77, 5.55, 6.66]) for _ in range(5)]
    assert _stable(roads, R.REFERENCE)
    rec, n_geom = _records(roads, 3)
    want = _road_rows(roads)
    full = [len(w) for w in want[0]]
    for mp in (max(full), min(full) - 1, 65, 64, 1):
        rc, xy, s, kappa, count = _lines(torch, rec, n_geom, R.REFERENCE, mp)
        assert rc == 0 and count[:5].tolist() == full
        assert _check(xy, count, want[0], mp, mp, ((s, want[1]), (kappa, want[2]))) <= TOL
    for planes in ((False, True), (True, False), (False, False)):
        rc, xy, s, kappa, count = _lines(torch, rec, n_geom, R.REFERENCE, 100, planes=planes)
        assert rc == 0 and _check(xy, count, want[0], 100, planes) <= TOL
        assert planes[0] or (s == SENTINEL).all()
        assert planes[1] or (kappa == SENTINEL).all()


# ---- bad rows ------------------------------------------------------------------------------------------------------------------------
def test_bad_rows_touch_only_their_own_outputs(torch):
    rng = np.random.default_rng(35)
    par = _fresh_spirals(rng, 7)
    par[1, 0], par[3, 2], par[5, 5] = -1.0, np.nan, np.inf
    rc, xy, count = _spirals(torch, par, 65, R.REFERENCE, 65)
    assert rc == 0 and _check(xy, count, [R.spiral(*p, 65) for p in par], 65, "spirals") <= TOL and count[:7].tolist() == [65, 0, 65, 0, 65, 0, 65]
    k = np.stack([rng.uniform(0.5, 9.0, 7)] + [rng.uniform(-1, 1, 7) for _ in range(11)], 1)
    k[1, 0], k[3, 11], k[5, 4] = -0.5, np.nan, -np.inf
    p_range = np.array([0, 1, 1, 0, 5, 0, 1], np.int32)
    want = [R.param_poly3(p[0], p[1], p[2], p[3], p[4:], r) for p, r in zip(k, p_range)]
    assert [w is None for w in want] == [False, True, False, True, True, True, False]
    rc, xy, count = _pp3(torch, k, p_range, 90)
    assert rc == 0 and _check(xy, count, want, 90, "paramPoly3") <= TOL

    good = lambda: _chain(rng, [R.LINE, R.SPIRAL, R.ARC], [4.44, 5.55, 3.33])
    bad = []
    r = good(); r[1]["length"] = -1.0; bad.append(r)                        # a negative length
    r = good(); r[2]["curvature"] = np.nan; bad.append(r)                   # a value its kind reads is not finite
    r = good(); r[0]["x"] = np.inf; bad.append(r)
    r = good(); r[1]["kind"] = 5; bad.append(r)                             # an unknown kind
    r = good(); r[1]["kind"] = -1; bad.append(r)
    r = good(); r[0] = _draw(rng, R.PARAM_POLY3, 0.0, 1.0, 2.0, 0.3, 4.0); r[0]["pRange"] = 2; bad.append(r)
    r = good(); r[0]["length"] = 0.1 * (R.MAX_RAW + 10); bad.append(r)      # more raw points than T2D_PLANVIEW_MAX_RAW
    roads = []
    for b in bad:
        roads += [good(), b]
    roads += [good(), good(), good(), good()]
    n_geom = [len(r) for r in roads]
    n_geom[-3], n_geom[-2] = 0, 4                                           # n_geom outside [1, max_geom]
    assert _stable([r for r in roads if R.planview(r)["count"]], R.REFERENCE)
    rec, ng = _records(roads, 3, n_geom)
    want = [list(w) for w in _road_rows(roads)]
    for w in want:
        w[-3] = w[-2] = None
    assert [w is None for w in want[0]] == [False, True] * len(bad) + [False, True, True, False]
    # a value the row's kinds do NOT read may be anything: the unused par entries hold 7e30, and here one holds a NaN
    rec[0, 0, 13] = np.nan
    mp = max(len(w) for w in want[0] if w is not None)
    rc, xy, s, kappa, count = _lines(torch, rec, ng, R.REFERENCE, mp)
    worst = _check(xy, count, want[0], mp, "roads", ((s, want[1]), (kappa, want[2])))
    print("good rows between bad rows: largest deviation", worst)
    assert rc == 0 and worst <= TOL


# ---- error paths, a side stream ----------------------------------------------------------------------------------------------------
def test_every_invalid_call_launches_nothing(torch):
    from tactics2d_amd import _ffi, layout as L
    lib = _ffi.lib()
    buf = torch.zeros(4096, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    I = _ffi.ERR_INVALID
    sp = lambda n=1, par=p, ni=10, rule=0, mp=16, xy=p, cnt=p: lib.t2d_spiral_curves(0, n, par, ni, rule, mp, xy, cnt, None)
    for kw in (dict(n=-1), dict(mp=0), dict(mp=-3), dict(ni=0), dict(ni=-1), dict(rule=2), dict(rule=-1), dict(par=None), dict(xy=None),
               dict(cnt=None), dict(par=p + 4), dict(xy=p + 8), dict(cnt=p + 2)):
        assert sp(**kw) == I, kw
    pp = lambda n=1, par=p, rng=p, mp=16, xy=p, cnt=p: lib.t2d_param_poly3_curves(0, n, par, rng, mp, xy, cnt, None)
    for kw in (dict(n=-1), dict(mp=0), dict(par=None), dict(rng=None), dict(xy=None), dict(cnt=None), dict(par=p + 4), dict(rng=p + 2),
               dict(xy=p + 8), dict(cnt=p + 2)):
        assert pp(**kw) == I, kw
    pv = lambda n=1, rec=p, ng=p, mg=4, rule=0, mp=16, xy=p, s=p, k=p, cnt=p: lib.t2d_planview_lines(0, n, rec, ng, mg, rule, mp, xy, s, k, cnt, None)
    for kw in (dict(n=-1), dict(mp=0), dict(mg=0), dict(mg=L.PLANVIEW_MAX_GEOM + 1), dict(rule=2), dict(rec=None), dict(ng=None), dict(xy=None),
               dict(cnt=None), dict(rec=p + 4), dict(ng=p + 2), dict(xy=p + 8), dict(s=p + 4), dict(k=p + 4), dict(cnt=p + 2)):
        assert pv(**kw) == I, kw
    assert sp(n=0) == _ffi.OK and pp(n=0) == _ffi.OK and pv(n=0) == _ffi.OK
    torch.cuda.synchronize()
    assert (buf == 0).all()


def test_the_classes_on_a_side_stream_and_with_their_defaults(torch):
    from tactics2d_amd.interpolator import ParamPoly3, Spiral, pack_planview, planview_lines
    rng = np.random.default_rng(37)
    par = _fresh_spirals(rng, 5)
    side = torch.cuda.Stream()
    dev = torch.as_tensor(par, device="cuda")
    torch.cuda.synchronize()
    a = Spiral.get_curve(dev[:, 0], dev[:, 1:3], dev[:, 3], dev[:, 4], dev[:, 5], stream=side)                   # CUDA tensors, 100 points
    b = Spiral.get_curve(par[:, 0], par[:, 1:3], par[:, 3], par[:, 4], par[:, 5], 33, rule="standard", stream=side)
    c = ParamPoly3.get_curve(par[:, 0], par[:, 1:3], par[:, 3], 0.0, 1.0, 0.01, 0.001, 0.0, 0.1, -0.02, 0.002, "arcLength", stream=side)
    road = _chain(rng, [R.LINE, R.SPIRAL, R.ARC, R.SPIRAL, R.LINE], rule=R.STANDARD)
    names = ("line", "spiral", "arc")
    packed = [dict(type=names[g["kind"]], **{k: v for k, v in g.items() if k not in ("kind", "pRange")}) for g in road]
    rec, ng = pack_planview([packed, packed[:2]])
    d = planview_lines(rec, ng, rule="standard", stream=side, want_kappa=False)
    side.synchronize()
    torch.cuda.synchronize()
    assert tuple(a.xy.shape) == (5, 100, 2) and a.count.tolist() == [100] * 5 and tuple(b.xy.shape) == (5, 33, 2) and d.kappa is None
    worst = 0.0
    for e in range(5):
        want = R.param_poly3(par[e, 0], par[e, 1], par[e, 2], par[e, 3], (0.0, 1.0, 0.01, 0.001, 0.0, 0.1, -0.02, 0.002), R.ARC_LENGTH)
        assert int(c.count[e]) == len(want)
        worst = max(worst, np.abs(a.xy[e].cpu().numpy() - R.spiral(*par[e], 100)).max(), np.abs(b.xy[e].cpu().numpy() - R.spiral(*par[e], 33, R.STANDARD)).max(),
                    np.abs(c.xy[e, :len(want)].cpu().numpy() - want).max())
    for e, r in enumerate((road, road[:2])):
        want = R.planview(r, R.STANDARD)
        assert int(d.count[e]) == want["count"]
        worst = max(worst, np.abs(d.xy[e, :want["count"]].cpu().numpy() - want["xy"]).max(), np.abs(d.s[e, :want["count"]].cpu().numpy() - want["s"]).max())
    assert worst <= TOL
    one = Spiral.get_curve(20.0, [0.0, 0.0], 0.3, 0.05, 0.01)                                                   # scalars: one curve as numpy
    assert isinstance(one, np.ndarray) and one.shape == (100, 2) and np.abs(one - R.spiral(20.0, 0.0, 0.0, 0.3, 0.05, 0.01)).max() <= TOL
    one = ParamPoly3.get_curve(5.05, (1.0, 2.0), 0.3, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.1, 0.0)
    assert one.shape == (50, 2) and np.abs(one - R.param_poly3(5.05, 1.0, 2.0, 0.3, (0, 1, 0, 0, 0, 0, 0.1, 0))).max() <= TOL
    bad = dev.clone()
    bad[2, 0] = -1.0                                               # a device tensor is not looked at: the row comes back with count 0
    assert Spiral.get_curve(bad[:, 0], bad[:, 1:3], bad[:, 3], bad[:, 4], bad[:, 5], 7).count.tolist() == [7, 7, 0, 7, 7]


# ---- roads as routes ----------------------------------------------------------------------------------------------------------------
def _routes_against_the_specification_and_a_twin_pool(torch, stride, n_env, no_line, make_caps):
    """one road per env of a pool of n_env envs; env `no_line` (None: no env) has a road without a line; make_caps(counts) gives
    the route capacities from the vertex counts of the lines"""
    from tactics2d_amd import layout as L
    rng = np.random.default_rng(41)
    roads = [_chain(rng, [R.LINE, R.SPIRAL, R.ARC, R.POLY3][:1 + e % 4] + [R.LINE], rng.uniform(5.03, 7.97, 5).tolist(), R.STANDARD) for e in range(n_env)]
    for r in roads:                                          # near the origin, where the cars are
        dx, dy = r[0]["x"], r[0]["y"]
        for g in r:
            g["x"], g["y"] = g["x"] - dx, g["y"] - dy
    if no_line is not None:
        roads[no_line] = [dict(kind=R.SPIRAL, s=0.0, x=0.0, y=0.0, hdg=0.0, length=1.5, curvStart=0.0, curvEnd=0.01, pRange=0)]   # one kept point: no line
    assert _stable(roads, R.STANDARD)
    lines = [R.planview(r, R.STANDARD) for r in roads]
    counts = [R.route_vertices(l["xy"], stride, 1 << 20)[1] for l in lines]
    assert (no_line is None or counts[no_line] == 0) and min(c for e, c in enumerate(counts) if e != no_line) > 12
    caps = make_caps(counts)
    rec, n_geom = _records(roads, 5)
    x = np.repeat(np.linspace(0.0, 9.0, A)[None], n_env, 0).astype(np.float32).ravel()
    y = rng.uniform(-5.0, 5.0, n_env * A).astype(np.float32)
    z = np.zeros(n_env * A, np.float32)
    pool = _route_pool(x, y, z, z, n_env)
    pool.set_routes([[_placeholder(caps[e], e)] for e in range(n_env)], np.arange(n_env), 0, 1.5)
    before = pool.route_vertices().cpu().numpy().copy()
    pool.profile_enable(True)
    count = pool.planview_routes(torch.as_tensor(rec), torch.as_tensor(n_geom), stride=stride, route=0, rule="standard")
    pool.sync()
    assert pool.profile_read(L.PROFILE_PLANVIEW_ROUTES)[1] == 1 and pool.profile_read(L.PROFILE_SPLINE_ROUTES)[1] == 0
    pool.profile_enable(False)
    assert count.cpu().tolist() == counts
    verts = pool.route_vertices().cpu().numpy()
    off = np.concatenate([[0], np.cumsum(caps)])
    equal = total = 0
    for e in range(n_env):
        got = verts[off[e]:off[e + 1]]
        want, c = R.route_vertices(lines[e]["xy"], stride, caps[e])
        if e == no_line:
            assert want is None and np.array_equal(got, before[off[e]:off[e + 1]])                  # untouched, bit for bit
            continue
        equal, total = equal + int((got == want).sum()), total + got.size
        if caps[e] > c:                                                                             # padding: the last kept point
            assert (got[c:] == lines[e]["xy"][-1].astype(np.float32)).all(), e
        elif caps[e] < c:                                                                           # overflow: the first `capacity`
            assert np.array_equal(got, lines[e]["xy"][::stride][:caps[e]].astype(np.float32)), e
    on_stride = sum(1 for l in lines if l["count"] and (l["count"] - 1) % stride == 0)
    print(f"stride {stride}: plan-view route vertices bit-equal to the fp32 rounding of the specification: {equal} of {total}; "
          f"{on_stride} of {sum(1 for c in counts if c)} lines end on the stride")
    assert equal == total
    got = _off_route(pool)
    twin = _route_pool(x, y, z, z, n_env)
    twin.set_routes([[verts[off[e]:off[e + 1]]] for e in range(n_env)], np.arange(n_env), 0, 1.5)
    ref = _off_route(twin)
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.isfinite(got[0]).all()
    pool.close()
    twin.close()


@pytest.mark.parametrize("stride", [7, 1])
def test_planview_routes_against_the_specification_and_a_twin_pool(torch, stride):
    _routes_against_the_specification_and_a_twin_pool(torch, stride, N_ENV, 5, lambda c: [c[0] - 5, c[1], c[2] + 9, c[3] + 70, 2, 33, c[6] - 1, c[7] + 1])     # below, equal, above


@pytest.mark.parametrize("no_line", [None, 4], ids=["env4_alone", "no_writer"])
def test_planview_routes_of_a_pool_that_ends_inside_a_workgroup(torch, no_line):
    """5 envs, four roads to a workgroup: env 4 is the only live wave of the last workgroup (a route longer than its line: the head,
    the last kept point and the padding are all its own stores); without a line in env 4 that workgroup has no writer at all.
    The capacities are those of the 8-env test's envs 0 .. 3, and its env 7's or (no line) env 5's for env 4."""
    _routes_against_the_specification_and_a_twin_pool(torch, 7, 5, no_line,
                                                      lambda c: [c[0] - 5, c[1], c[2] + 9, c[3] + 70, 33 if no_line == 4 else c[4] + 1])


def test_planview_routes_error_paths(torch):
    from tactics2d_amd import _ffi, layout as L
    z = np.zeros(N_ENV * A, np.float32)
    pool = _route_pool(z, z, z, z)
    rng = np.random.default_rng(43)
    rec, n_geom = _records([_chain(rng, [R.LINE, R.ARC]) for _ in range(N_ENV)], 2)
    r, g = _dev(torch, rec), _dev(torch, n_geom, np.int32)
    lib = _ffi.lib()

    def code(rec=r.data_ptr(), ng=g.data_ptr(), mg=2, rule=0, stride=1, route=0, cnt=None, h=pool._h):
        return lib.t2d_planview_routes(h, rec, ng, mg, rule, stride, route, cnt, None)

    assert code() == _ffi.ERR_STATE                                                   # no routes installed
    pool.set_routes([[_placeholder(40, 0)]], None, 0, 1.0)                            # one set shared by every env
    assert code() == _ffi.ERR_STATE
    sets = [[_placeholder(40, e)] + ([_placeholder(4, e)] if e != 3 else []) for e in range(N_ENV)]
    pool.set_routes(sets, np.arange(N_ENV), 0, 1.0)
    before = pool.route_vertices().cpu().numpy().copy()
    assert code(route=1) == _ffi.ERR_STATE and code(route=2) == _ffi.ERR_STATE        # env 3's set has no route 1
    for kw in (dict(stride=0), dict(stride=-2), dict(rule=2), dict(route=-1), dict(mg=0), dict(mg=L.PLANVIEW_MAX_GEOM + 1), dict(rec=None),
               dict(ng=None), dict(rec=r.data_ptr() + 4), dict(ng=g.data_ptr() + 2), dict(cnt=g.data_ptr() + 2), dict(h=None)):
        assert code(**kw) == _ffi.ERR_INVALID, kw
    with pytest.raises(_ffi.T2DError) as ei:
        pool.planview_routes(r, g, route=1)
    assert ei.value.code == _ffi.ERR_STATE
    with pytest.raises(ValueError):
        pool.planview_routes(r[:4], g[:4])
    with pytest.raises(ValueError):
        pool.planview_routes(r, g, count=torch.zeros(3, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError):
        pool.planview_routes(r, g, rule="euler")
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before)                # nothing was launched
    assert code() == _ffi.OK                                                          # a NULL count pointer is allowed
    pool.sync()
    assert not np.array_equal(pool.route_vertices().cpu().numpy(), before)
    pool.clear_routes()
    assert code() == _ffi.ERR_STATE
    pool.close()


def _clothoid_road(rng):
    """straight -> clothoid -> arc -> clothoid -> straight, each geometry starting at the true end of the one before"""
    k = float(rng.choice([-1, 1]) * rng.uniform(0.03, 0.05))
    x, y, h, s, road = 0.0, float(rng.uniform(-3, 3)), float(rng.uniform(-0.3, 0.3)), 0.0, []
    for kind, length, k0, k1 in ((R.LINE, 30.3, 0, 0), (R.SPIRAL, 20.2, 0.0, k), (R.ARC, 25.5, k, k), (R.SPIRAL, 20.2, k, 0.0), (R.LINE, 30.3, 0, 0)):
        g = dict(kind=kind, s=s, x=x, y=y, hdg=h, length=length, pRange=0)
        if kind == R.SPIRAL:
            g.update(curvStart=k0, curvEnd=k1)
        if kind == R.ARC:
            g.update(curvature=k)
            x, y = x + (np.sin(h + k * length) - np.sin(h)) / k, y + (np.cos(h) - np.cos(h + k * length)) / k
        else:
            x, y = (float(v) for v in R.sample_geometry(g, R.STANDARD)[0][-1])
        road.append(g)
        s, h = s + length, h + (k0 + k1) / 2 * length
    return road


def test_pure_pursuit_cars_follow_a_clothoid_road_written_on_the_device(torch):
    """8 envs x 4 cars under pure pursuit for 100 steps on a straight-clothoid-arc-clothoid-straight road per env, written by
    planview_routes (rule "standard", stride 10).  The yardstick is the same run on the same polyline installed from the host:
    its largest off-route distance is the threshold, and the two runs agree bit for bit."""
    import pursuit_scenes as US
    from tactics2d_amd import layout as L
    from tactics2d_amd.controller import PathFollower, install_pursuit
    rng = np.random.default_rng(47)
    roads = [_clothoid_road(rng) for _ in range(N_ENV)]
    rec, n_geom = _records(roads, 5)
    cap, stride = 160, 10
    s0 = np.array([2.0, 9.0, 16.0, 23.0])
    x = np.concatenate([r[0]["x"] + s0 * np.cos(r[0]["hdg"]) for r in roads]).astype(np.float32)
    y = np.concatenate([r[0]["y"] + s0 * np.sin(r[0]["hdg"]) for r in roads]).astype(np.float32)
    h = np.repeat([r[0]["hdg"] for r in roads], A).astype(np.float32)
    v = np.full(N_ENV * A, 8.0, np.float32)

    def run(vertices, threshold, steps=100):
        pool = _route_pool(x, y, h, v)
        pool.set_routes([[_placeholder(cap, e)] for e in range(N_ENV)] if vertices is None else vertices, np.arange(N_ENV), 0, threshold)
        if vertices is None:
            count = pool.planview_routes(torch.as_tensor(rec), torch.as_tensor(n_geom), stride=stride, rule="standard")
        install_pursuit(pool, [US.ring_controller()], np.zeros(N_ENV * A, np.uint8), v)
        follower = PathFollower(pool)
        rows = torch.zeros((steps, N_ENV * A, 2), dtype=torch.float32, device="cuda")
        dist, off = [], []
        for k in range(steps):
            follower.follow(None, rows[k])
            p = rows[k].data_ptr()
            pool.bind_actions(p + 4, p, stride=2)
            pool.step(100)
            d, o = _off_route(pool)
            dist.append(d)
            off.append(o)
        pool.sync()
        verts = pool.route_vertices().cpu().numpy().copy()
        state = [pool.download(f).copy() for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED)]
        counts = count.cpu().numpy() if vertices is None else None
        pool.bind_actions(None, None)
        pool.close()
        return verts, np.array(dist), np.array(off), rows.cpu().numpy(), state, counts

    verts, _, _, _, _, counts = run(None, 1.0e6, steps=0)
    want = [R.route_vertices(R.planview(r, R.STANDARD)["xy"], stride, cap) for r in roads]
    assert counts.tolist() == [c for _, c in want] and max(counts) < cap and min(counts) > 60
    assert np.array_equal(verts.reshape(N_ENV, cap, 2), np.stack([w for w, _ in want]))
    host = run([[verts[e * cap:(e + 1) * cap]] for e in range(N_ENV)], 1.0e6)               # the same polyline from the host
    # (the verdict compares the fp64 distance, the report is its fp32 rounding: the next fp32 value bounds both)
    threshold = float(np.nextafter(host[1].max(), np.float32(np.inf)))
    print("pure pursuit on the clothoid roads: largest off-route distance of the host-installed run", threshold, "m; travelled",
          float(np.hypot(host[4][0] - x, host[4][1] - y).min()), "m at least")
    assert np.isfinite(host[1]).all() and np.hypot(host[4][0] - x, host[4][1] - y).min() > 40.0
    device = run(None, threshold)
    assert not device[2].any()                                                               # within the threshold for 100 steps
    assert np.array_equal(device[1], host[1]) and np.array_equal(device[3].view(np.uint32), host[3].view(np.uint32))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(device[4], host[4]))
