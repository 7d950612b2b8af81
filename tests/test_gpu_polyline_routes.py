"""t2d_polyline_routes / ParticipantPool.polyline_routes on the device: a planner's path that is already on the device becomes the
route traffic follows.  Routes written from an RRT path and from a hybrid A* path (with its heading column) equal the fp32 rounding
of the points, padded with the last point; rows with count 0, a NaN point, a count above max_pts or above the route's capacity
behave as specified and leave the placeholder routes of the other envs untouched; off_route reads distance ~ 0 for vehicles placed
on the written path; pure-pursuit cars follow a route written on the device bit for bit as they follow the same polyline installed
from the host; and the shared gate's refusals hold for the fourth writer."""
import numpy as np
import pytest

from route_writers import A, N_ENV, off_route, placeholder, route_pool

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _want(points, count, cap):
    """the vertices of a route of `cap` vertices written from points [max_pts, C] with `count`"""
    used = min(int(count), len(points))
    with np.errstate(over="ignore"):   # (a coordinate beyond fp32 rounds to inf, as on the device)
        xy = points[:used, :2].astype(np.float32)
    return np.concatenate([xy, np.repeat(xy[-1:], cap - used, 0)])[:cap] if used < cap else xy[:cap]


def _planned(torch, hybrid):
    """N_ENV planned paths on the device: (path [N_ENV, max_path, C], path_len [N_ENV])"""
    from tactics2d_amd import search
    rng = np.random.RandomState(3 + hybrid)
    grids = np.ones((N_ENV, 16, 16))
    for e in range(N_ENV):
        grids[e][rng.rand(16, 16) < (0.03 if hybrid else 0.08)] = np.inf
        grids[e][:3, :3] = grids[e][12:, 12:] = 1.0
    boundary = [0.0, 16.0, 0.0, 16.0]
    if hybrid:
        starts = np.float64([[1.0, 1.0, 0.7]] * N_ENV)
        targets = np.float64([[13.0 + 0.1 * e, 14.0, 0.7] for e in range(N_ENV)])
        out = search.HybridAStar.plan_batch(starts, targets, boundary, grids, max_path=128)
        assert (out.status.cpu().numpy() == search.HYBRID_FOUND).all() and out.path.shape == (N_ENV, 128, 3)
    else:
        starts = np.float64([[1.0, 1.0]] * N_ENV)
        targets = np.float64([[13.0 + 0.1 * e, 14.0] for e in range(N_ENV)])
        out = search.RRT.plan_batch(starts, targets, boundary, grids, 11, max_iter=3000, max_path=128)
        assert (out.status.cpu().numpy() == search.SAMPLE_FOUND).all() and out.path.shape == (N_ENV, 128, 2)
    return out.path, out.path_len


@pytest.mark.parametrize("hybrid", [0, 1], ids=["rrt", "hybrid_astar"])
def test_a_planned_path_becomes_the_route(torch, hybrid):
    from tactics2d_amd import layout as L
    path, path_len = _planned(torch, hybrid)
    pts, counts = path.cpu().numpy(), path_len.cpu().numpy()
    assert counts.min() >= 8 and counts.max() <= 128
    caps = [int(counts[0]) - 3, int(counts[1]), int(counts[2]) + 9, int(counts[3]) + 70, 2, 33, int(counts[6]) - 1, int(counts[7]) + 1]
    z = np.zeros(N_ENV * A, np.float32)
    pool = route_pool(z, z, z, z)
    pool.set_routes([[placeholder(caps[e], e)] for e in range(N_ENV)], np.arange(N_ENV), 0, 1.5)
    pool.profile_enable(True)
    count = pool.polyline_routes(path, path_len)
    pool.sync()
    assert pool.profile_read(L.PROFILE_POLYLINE_ROUTES)[1] == 1 and pool.profile_read(L.PROFILE_PLANVIEW_ROUTES)[1] == 0
    pool.profile_enable(False)
    assert count.dtype == torch.int32 and count.cpu().tolist() == counts.tolist()
    verts = pool.route_vertices().cpu().numpy()
    off = np.concatenate([[0], np.cumsum(caps)])
    for e in range(N_ENV):
        assert np.array_equal(verts[off[e]:off[e + 1]], _want(pts[e], counts[e], caps[e])), e
    # vehicles placed on the written path are on the route
    x = np.concatenate([verts[off[e]:off[e + 1]][np.arange(A) % caps[e], 0] for e in range(N_ENV)])
    y = np.concatenate([verts[off[e]:off[e + 1]][np.arange(A) % caps[e], 1] for e in range(N_ENV)])
    on = route_pool(x, y, z, z)
    on.set_routes([[placeholder(caps[e], e)] for e in range(N_ENV)], np.arange(N_ENV), 0, 1.5)
    far = off_route(on)
    assert far[0].min() > 100.0 and far[1].all()
    given = torch.full((N_ENV,), -5, dtype=torch.int32, device="cuda")
    assert on.polyline_routes(path, path_len, count=given) is given
    dist, verdict = off_route(on)
    assert given.cpu().tolist() == counts.tolist() and dist.max() <= 1e-4 and not verdict.any()
    pool.close()
    on.close()


def test_rows_without_points_with_a_nan_and_with_too_many_points(torch):
    cap, max_pts = 12, 10
    rng = np.random.RandomState(8)
    pts = rng.uniform(-50.0, 50.0, (N_ENV, max_pts, 3))
    counts = np.int32([0, 5, 10, 25, -3, 7, 10, 6])        # none, fewer than the route, all, more than max_pts, negative, ...
    pts[5, 6, 1] = np.nan                                  # among the points env 5 would write
    pts[6, 3, 0] = np.inf
    pts[7, 6:, :] = np.nan                                 # past env 7's count: never read as a vertex
    pts[1, 2, 2] = np.nan                                  # a third column is not a coordinate
    pts[2, 7, 0] = 1e39                                    # finite, but not as fp32
    caps = [cap, cap, cap, 4, cap, cap, cap, cap]          # env 3: more points than its route has vertices
    z = np.zeros(N_ENV * A, np.float32)
    pool = route_pool(z, z, z, z)
    pool.set_routes([[placeholder(caps[e], e), placeholder(5, e, 900.0)] for e in range(N_ENV)], np.arange(N_ENV), 0, 1.0)
    before = pool.route_vertices().cpu().numpy().copy()
    d_pts, d_counts = torch.as_tensor(pts, device="cuda"), torch.as_tensor(counts, device="cuda")
    count = pool.polyline_routes(d_pts, d_counts)
    pool.sync()
    assert count.cpu().tolist() == [0, 5, 0, 10, 0, 0, 0, 6]
    verts = pool.route_vertices().cpu().numpy()
    off = np.concatenate([[0], np.cumsum([c + 5 for c in caps])])
    for e in range(N_ENV):
        got, was = verts[off[e]:off[e] + caps[e]], before[off[e]:off[e] + caps[e]]
        assert np.array_equal(verts[off[e] + caps[e]:off[e + 1]], before[off[e] + caps[e]:off[e + 1]]), e        # route 1 of every env
        if e in (0, 2, 4, 5, 6):
            assert np.array_equal(got, was), e                                                               # left as it is
        else:
            assert np.array_equal(got, _want(pts[e], counts[e], caps[e])) and np.isfinite(got).all(), e
    # route 1, five vertices: the NaN of env 5 lies past them now, so its route is written
    count = pool.polyline_routes(d_pts, d_counts, route=1)
    pool.sync()
    assert count.cpu().tolist() == [0, 5, 10, 10, 0, 7, 0, 6]
    after = pool.route_vertices().cpu().numpy()
    for e in range(N_ENV):
        assert np.array_equal(after[off[e]:off[e] + caps[e]], verts[off[e]:off[e] + caps[e]]), e                 # route 0 as it was
        got = after[off[e] + caps[e]:off[e + 1]]
        if e in (0, 4, 6):
            assert np.array_equal(got, before[off[e] + caps[e]:off[e + 1]]), e
        else:
            assert np.array_equal(got, _want(pts[e], counts[e], 5)), e
    pool.close()


def test_pure_pursuit_cars_follow_a_polyline_written_on_the_device(torch):
    """8 envs x 4 cars under pure pursuit for 60 steps along a gentle S-curve per env, written by polyline_routes.  The yardstick
    is the same run on the same polyline installed from the host: the two runs agree bit for bit."""
    import pursuit_scenes as US
    from tactics2d_amd import layout as L
    from tactics2d_amd.controller import PathFollower, install_pursuit
    cap, n_pts = 160, 140
    s = np.linspace(0.0, 139.0, n_pts)
    pts = np.stack([np.stack([s, (3.0 + 0.5 * e) * np.sin(s / (18.0 + e)), 0.0 * s], 1) for e in range(N_ENV)])   # [N_ENV, n_pts, 3]
    counts = np.int32([n_pts - 3 * e for e in range(N_ENV)])
    s0 = np.array([2.0, 9.0, 16.0, 23.0])
    x = np.tile(s0, N_ENV).astype(np.float32)
    y = np.concatenate([(3.0 + 0.5 * e) * np.sin(s0 / (18.0 + e)) for e in range(N_ENV)]).astype(np.float32)
    h = np.concatenate([np.arctan((3.0 + 0.5 * e) / (18.0 + e) * np.cos(s0 / (18.0 + e))) for e in range(N_ENV)]).astype(np.float32)
    v = np.full(N_ENV * A, 8.0, np.float32)

    def run(vertices, steps=60):
        pool = route_pool(x, y, h, v)
        pool.set_routes([[placeholder(cap, e)] for e in range(N_ENV)] if vertices is None else vertices, np.arange(N_ENV), 0, 1.0e6)
        if vertices is None:
            pool.polyline_routes(torch.as_tensor(pts, device="cuda"), torch.as_tensor(counts, device="cuda"))
        install_pursuit(pool, [US.ring_controller()], np.zeros(N_ENV * A, np.uint8), v)
        follower = PathFollower(pool)
        rows = torch.zeros((steps, N_ENV * A, 2), dtype=torch.float32, device="cuda")
        dist = []
        for k in range(steps):
            follower.follow(None, rows[k])
            p = rows[k].data_ptr()
            pool.bind_actions(p + 4, p, stride=2)
            pool.step(100)
            dist.append(off_route(pool)[0])
        pool.sync()
        verts = pool.route_vertices().cpu().numpy().copy()
        state = [pool.download(f).copy() for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED)]
        pool.bind_actions(None, None)
        pool.close()
        return verts, np.array(dist), rows.cpu().numpy(), state

    device = run(None)
    assert np.array_equal(device[0].reshape(N_ENV, cap, 2), np.stack([_want(pts[e], counts[e], cap) for e in range(N_ENV)]))
    host = run([[device[0][e * cap:(e + 1) * cap]] for e in range(N_ENV)])
    assert np.isfinite(host[1]).all() and host[1].max() < 2.0 and np.hypot(host[3][0] - x, host[3][1] - y).min() > 30.0
    assert np.array_equal(device[1], host[1]) and np.array_equal(device[2].view(np.uint32), host[2].view(np.uint32))
    assert all(np.array_equal(a.view(np.uint32), b.view(np.uint32)) for a, b in zip(device[3], host[3]))


def _refused(pool, rc, code, text):
    from tactics2d_amd import _ffi
    assert rc == code, (rc, code, text)
    with pytest.raises(_ffi.T2DError) as ei:
        _ffi.check(rc, pool._h)
    assert str(ei.value) == f"libt2d_hip error {code}: {text}"


def test_the_shared_gate_and_the_argument_checks_hold_for_the_fourth_writer(torch):
    from tactics2d_amd import _ffi
    who = "t2d_polyline_routes"
    z = np.zeros(N_ENV * A, np.float32)
    pool = route_pool(z, z, z, z)
    lib, h = _ffi.lib(), pool._h
    pts = torch.as_tensor(np.cumsum(np.ones((N_ENV, 6, 2)), 1), device="cuda")
    counts = torch.full((N_ENV,), 6, dtype=torch.int32, device="cuda")
    count = torch.zeros(N_ENV + 1, dtype=torch.int32, device="cuda")

    def call(route=0, cnt=None, p=pts.data_ptr(), c=counts.data_ptr(), max_pts=6, cols=2):
        return lib.t2d_polyline_routes(h, p, c, max_pts, cols, route, cnt, None)

    no_sets = f"{who} writes into route sets: t2d_set_routes must precede it"
    for bad in (dict(p=None), dict(c=None), dict(p=pts.data_ptr() + 4), dict(c=counts.data_ptr() + 2), dict(max_pts=0), dict(cols=1)):
        assert call(**bad) == _ffi.ERR_INVALID, bad                                     # the family's own check wins over the state
    _refused(pool, call(route=-1), _ffi.ERR_INVALID, f"{who}: route must be >= 0")
    _refused(pool, call(cnt=count.data_ptr() + 2), _ffi.ERR_INVALID, f"{who}: misaligned count_dev")
    _refused(pool, call(), _ffi.ERR_STATE, no_sets)
    pool.set_routes([[placeholder(40, 0)]], None, 0, 1.0)                               # one set shared by every env
    _refused(pool, call(), _ffi.ERR_STATE, f"{who}: two envs share a route set; install one set per env (set_of_env)")
    sets = [[placeholder(40, e)] + ([placeholder(4, e), placeholder(4, e)] if e != 3 else []) for e in range(N_ENV)]
    pool.set_routes(sets, np.arange(N_ENV), 0, 1.0)                                     # env 3's set has one route, the others three
    before = pool.route_vertices().cpu().numpy().copy()
    for route in (1, 2, 1000):
        _refused(pool, call(route=route), _ffi.ERR_STATE,
                 f"{who}: route {route} does not exist in every env's set (the smallest set has 1 routes)")
    with pytest.raises(_ffi.T2DError) as ei:
        pool.polyline_routes(pts, counts, route=1)
    assert ei.value.code == _ffi.ERR_STATE
    for bad_pts, bad_counts in ((pts[:4], counts[:4]), (pts.float(), counts), (pts, counts.long()), (pts.cpu().numpy(), counts)):
        with pytest.raises(ValueError):
            pool.polyline_routes(bad_pts, bad_counts)
    with pytest.raises(ValueError):
        pool.polyline_routes(pts, counts, count=torch.zeros(3, dtype=torch.int32, device="cuda"))
    pool.sync()
    assert np.array_equal(pool.route_vertices().cpu().numpy(), before) and not count.cpu().numpy().any()   # nothing was launched
    assert call(cnt=count.data_ptr() + 4) == _ffi.OK                                    # (and a NULL count pointer is allowed:)
    assert call() == _ffi.OK
    pool.sync()
    assert not np.array_equal(pool.route_vertices().cpu().numpy(), before)
    assert count.cpu().tolist() == [0] + [6] * N_ENV
    pool.clear_routes()
    _refused(pool, call(), _ffi.ERR_STATE, no_sets)
    pool.close()
