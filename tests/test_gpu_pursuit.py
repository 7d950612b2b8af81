"""The pure-pursuit and cruise / ACC controllers on the device (t2d_pursuit_actions): the fixture recorded from the reference's own
classes, teacher-forced; the build-defined walk against tests/pursuit_ref.py; the projection against t2d_pid_actions' record;
ACC's leader against t2d_idm_actions; the bookkeeping of the call; and the closed loop on the device's own physics.

Pools: 3 envs x 3 participants (a partial wave), 2 x 64 (whole waves), 1 x 130 (three waves with invalid tail lanes: the leader
search crosses wave boundaries); the closed loop runs 8 x 16.

Teacher-forced: cruise is held bit for bit; ACC (sqrt(dx * dx + dy * dy) against np.hypot) and the steering (the library's own
atan2 / sin / atan against numpy's) to TOL = 1e-9 absolute, the project's figure for results through its own transcendental
functions (tests/test_gpu_pid.py).  Every test prints the largest difference it saw before it asserts.
Measured on an MI355X: ACC within 8.9e-16 of the reference (bit-equal in 1197 of the 1200 calls of the 3 x 3 pool, in all 120
of the other two -- not bit-equal, so the bound stays at TOL); steering within 1.2e-15; the walk's point and the action within
1.4e-15 of pursuit_ref; ACC against pursuit_ref on the platoon bit-equal.

Closed loop (pid_scenes.ring_scene: 128 kinematic cars on the 24-gon rings at r = 14 and 18 m, 4 - 8 m/s, up to 0.5 m off the
circle; pursuit_scenes.ring_controller: 5 m minimum look-ahead, cruise on the car's own start speed; 150 steps of
pursuit_actions -> bound rows -> t2d_step).  The bands come from pursuit_ref driven by the C oracle's kinematics on the CPU
(tests/test_pursuit.py recomputes them):

    figure                                                          CPU run      held to
    largest excess of a vehicle's |error| over its own start        0.7385 m     <= 0.74 m (pursuit_scenes.RING_MARGIN)
    largest |mean signed offset| over the second half               0.6555 m     <= 0.9833 m (the CPU figure + 50 %)
    largest mean |offset| over the second half                      0.6555 m     <= 0.9833 m (the CPU figure + 50 %)
    mean signed offsets of the cars                                 -0.66 .. -0.33 m: every car settles INSIDE its ring
    PID on the same scene (tests/pid_scenes.py)                     0.0870 m

and, measured, every step's action rows and cross-track errors equal the CPU run's bit for bit (not asserted: the steering goes
through the library's own atan2 / sin / atan on the device and numpy's on the CPU).
"""
import numpy as np
import pytest

import pid_scenes as PS
import pursuit_ref as UR
import pursuit_scenes as US
import route_scenes as RS

pytestmark = pytest.mark.gpu
SHAPES = [(3, 3), (2, 64), (1, 130)]
TOL = 1e-9
STRAIGHT = np.float32([[-1024, 0], [1024, 0]])


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _types():
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, full_type_table
    rows, names = full_type_table()
    ty = names.index(list(VEHICLE_TEMPLATE)[0] + ":kin")
    return rows, ty, rows[ty, L.P_LF] + rows[ty, L.P_LR]


def _pool(n_env, A, x=None, y=None, heading=None, speed=None, active=None):
    from tactics2d_amd.pool import ParticipantPool
    rows, ty, _ = _types()
    pool = ParticipantPool(n_env, A)
    pool.set_param_table(rows)
    pool.set_status_config(max_step=100000)
    z = np.zeros(n_env * A, np.float32)
    pool.reset(z if x is None else x, z if y is None else y, z if heading is None else heading, z if speed is None else speed,
               np.full(n_env * A, ty, np.uint8), active)
    return pool


def _set_pose(pool, x, y, heading, speed, accel=None):
    from tactics2d_amd import layout as L
    for f, v in ((L.F_X, x), (L.F_Y, y), (L.F_HEADING, heading), (L.F_SPEED, speed), (L.F_APPLIED0, accel)):
        if v is not None:
            pool.upload(f, np.ascontiguousarray(v, np.float32))


def _record(rec, n):
    r = rec.cpu().numpy()
    i32 = r.view(np.int32).reshape(n, -1)
    return dict(point=r[:, 0:2], pre_aiming_distance=r[:, 2], distance=r[:, 3], cross_track=r[:, 4], segment=i32[:, 10],
                target_segment=i32[:, 11], leader=i32[:, 12], events=i32[:, 13].view(np.uint32), action=r[:, 7:9])


def _run(torch, pool, act_in=None):
    """one t2d_pursuit_actions into fresh tensors -> (rows float32 [n, 2], record dict of numpy arrays)"""
    from tactics2d_amd import layout as L
    n = pool.n
    out = torch.full((n, 2), 7.0, dtype=torch.float32, device="cuda")
    rec = torch.zeros((n, L.PURSUIT_RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
    a = None if act_in is None else torch.as_tensor(np.ascontiguousarray(act_in, np.float32), device="cuda")
    pool.pursuit_actions(None if a is None else a.data_ptr(), out.data_ptr(), rec.data_ptr())
    pool.sync()
    if a is not None:
        assert (a.cpu().numpy().view(np.uint32) == np.ascontiguousarray(act_in, np.float32).view(np.uint32)).all(), "act_in was written"
    return out.cpu().numpy(), _record(rec, n)


def _same(a, b):
    """bit-equal float arrays, NaN = NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and bool(((a == b) | (np.isnan(a) & np.isnan(b))).all())


def _close(a, b, tol=TOL):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return bool((np.isnan(a) == np.isnan(b)).all()) and np.nanmax(np.abs(a - b), initial=0.0) <= tol


def _check(got_rows, rec, want, what=""):
    """a launch against pursuit_ref.evaluate: integers, events, the projection and pre_aiming_distance bit for bit; the point, the
    distance and the action within TOL; the row = the fp32 rounding of the record's action, or the caller's row"""
    assert (rec["events"] == want["events"]).all(), (what, np.flatnonzero(rec["events"] != want["events"])[:8])
    for key in ("segment", "target_segment", "leader"):
        assert (rec[key] == want[key]).all(), (what, key, np.flatnonzero(rec[key] != want[key])[:8])
    assert _same(rec["cross_track"], want["cross_track"]) and _same(rec["pre_aiming_distance"], want["pre_aiming_distance"]), what
    for key in ("point", "distance", "action"):
        assert _close(rec[key], want[key]), (what, key)
    acted = ~np.isnan(rec["action"][:, 0])
    assert (got_rows[acted].view(np.uint32) == rec["action"][acted].astype(np.float32).view(np.uint32)).all(), what
    assert (got_rows[~acted].view(np.uint32) == want["rows"][~acted].view(np.uint32)).all(), what
    with np.errstate(invalid="ignore"):
        assert np.nanmax(np.abs(got_rows[acted] - want["rows"][acted]), initial=0.0) <= 1e-6, what


def _per_env(routes, n_env, A):
    return [routes[e * A:(e + 1) * A] for e in range(n_env)]


# ---------------------------------------------------------------------------------------------------- 1. the fixture
@pytest.mark.parametrize("shape", SHAPES)
def test_fixture_cruise_and_pre_aiming_teacher_forced(torch, shape):
    """the cruise calls and the step calls without a front_state: acceleration and pre_aiming_distance bit for bit"""
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    f = US.fixture()
    free = np.isnan(f["s_front"][:, 0])
    par = np.concatenate([f["c_par"], f["s_par"][free, 2:]])
    speed = np.concatenate([f["c_in"][:, 0], f["s_in"][free, 3]])
    ts = np.concatenate([f["c_in"][:, 1], f["s_in"][free, 6]])
    last = np.concatenate([f["c_in"][:, 2], f["s_in"][free, 4]])
    want = np.concatenate([f["c_out"], f["s_out"][free, 1]])
    lat = np.concatenate([np.zeros(900), np.ones(free.sum())])
    min_pre = np.concatenate([np.full(900, 10.0), f["s_par"][free, 0]])
    ilat = np.concatenate([np.ones(900), f["s_par"][free, 1]])
    d_want = np.concatenate([np.full(900, np.nan), f["s_d"][free]])
    total = len(want)
    order = np.arange(total) if shape == (2, 64) else np.concatenate([np.arange(0, 4 * n), np.arange(total - 4 * n, total)])
    pool = _pool(n_env, A)
    pool.set_routes([[STRAIGHT]], None, 0, 0.0)
    z = np.zeros(n, np.float32)
    pad = lambda v: np.concatenate([v, np.zeros(n - len(v))])
    for lo in range(0, len(order), n):
        idx = order[lo:lo + n]
        k = len(idx)
        R = US.accel_rows(par[idx], 0, min_pre[idx], ilat[idx], lat[idx])
        _set_pose(pool, z, z, z, pad(speed[idx]), pad(last[idx]))
        pool.set_pursuit(R, np.where(np.arange(n) < k, np.arange(n), L.PURSUIT_NONE).astype(np.uint8), pad(ts[idx]))
        got, rec = _run(torch, pool)
        assert (rec["action"][:k, 1] == want[idx]).all(), f"calls {idx[0]}.."
        assert _same(rec["pre_aiming_distance"][:k], d_want[idx])
        assert (got[:k, 1].view(np.uint32) == want[idx].astype(np.float32).view(np.uint32)).all() and not rec["events"][:k].any()
        assert (rec["events"][k:] == 0).all() and np.isnan(rec["action"][k:]).all() and (got[k:] == 0).all()
    pool.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_fixture_acc_teacher_forced(torch, shape):
    """the ACC calls and the step calls with a front_state: the ego in slot 0 of each env, its front vehicle in the LAST slot
    (another wave at A = 130), everybody between inactive; the ego heads for the front vehicle, so the leader rule finds it"""
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    f = US.fixture()
    has = ~np.isnan(f["s_front"][:, 0])
    s_in, s_fr = f["s_in"][has], f["s_front"][has]
    par = np.concatenate([f["a_par"], f["s_par"][has, 2:]])
    ego = np.concatenate([f["a_in"][:, :4], s_in[:, [0, 1, 3, 4]]])          # x, y, speed, accel_last
    front = np.concatenate([f["a_in"][:, 4:8], s_fr])                        # x, y, speed, accel
    want = np.concatenate([f["a_out"], f["s_out"][has, 1]])
    total = len(want)
    order = np.arange(total) if shape == (3, 3) else np.concatenate([np.arange(0, 20 * n_env), np.arange(total - 20 * n_env, total)])
    active = np.zeros(n, np.uint8)
    active[0::A] = active[A - 1::A] = 1
    pool = _pool(n_env, A, active=active)
    worst, exact = 0.0, 0
    for lo in range(0, len(order), n_env):
        idx = order[lo:lo + n_env]
        k = len(idx)
        x, y, v, a = (np.zeros(n, np.float32) for _ in range(4))
        h = np.zeros(n, np.float32)
        e0, e1 = np.arange(k) * A, np.arange(k) * A + A - 1
        x[e0], y[e0], v[e0], a[e0] = ego[idx].T
        x[e1], y[e1], v[e1], a[e1] = front[idx].T
        h[e0] = np.arctan2(front[idx, 1] - ego[idx, 1], front[idx, 0] - ego[idx, 0])
        _set_pose(pool, x, y, h, v, a)
        R = US.accel_rows(par[idx], 1)
        R[:, UR.LANE_HALF_WIDTH] = 1.0
        cid = np.full(n, L.PURSUIT_NONE, np.uint8)
        cid[e0] = np.arange(k)
        pool.set_pursuit(R, cid, 3.0)
        got, rec = _run(torch, pool)
        assert (rec["leader"][e0] == A - 1).all() and not rec["events"][e0].any(), f"calls {idx[0]}.."
        diff = np.abs(rec["action"][e0, 1] - want[idx])
        worst, exact = max(worst, diff.max()), exact + int((diff == 0).sum())
        assert (rec["action"][e0, 0] == 0.0).all() and (got[e0, 1].view(np.uint32) == rec["action"][e0, 1].astype(np.float32).view(np.uint32)).all()
    print("ACC: largest deviation from the reference", worst, "; bit-equal in", exact, "of", len(order), "calls")
    assert worst <= TOL
    pool.close()


@pytest.mark.parametrize("shape", SHAPES)
def test_fixture_lateral_teacher_forced(torch, shape):
    """the _lateral_control calls: each participant's route ends in the fixture's pre-aiming point and the look-ahead is longer
    than the route, so the walk hands the law exactly that point (an open route that ends first gives its last vertex)"""
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    f = US.fixture()
    l_in, want = f["l_in"], f["l_out"]
    total = len(want)
    order = np.arange(total) if shape == (2, 64) else np.concatenate([np.arange(0, 3 * n), np.arange(total - 3 * n, total)])
    pool = _pool(n_env, A)
    worst = 0.0
    n_nan = n_half_pi = 0
    for lo in range(0, len(order), n):
        idx = order[lo:lo + n]
        k = len(idx)
        fill = lambda v, c=0.0: np.concatenate([v, np.full(n - k, c)]).astype(np.float32)
        x, y, h, px, py = (fill(l_in[idx, c]) for c in range(5))
        px[k:], py[k:] = 5.0, 0.0
        routes = [np.float32([[px[j] - 3.0, py[j] + 1.0], [px[j], py[j]]]) for j in range(n)]
        _set_pose(pool, x, y, h, np.ones(n, np.float32), np.zeros(n, np.float32))
        pool.set_routes(_per_env(routes, n_env, A), np.arange(n_env), np.tile(np.arange(A), n_env), 0.0)
        R = np.repeat(US.ring_controller().row("caller")[None], n, 0)
        R[:, UR.MIN_PRE_AIMING] = 1.0e4
        R[:k, UR.WHEEL_BASE] = l_in[idx, 5]
        pool.set_pursuit(R, np.arange(n).astype(np.uint8), None)
        act_in = np.full((n, 2), 0.25, np.float32)
        got, rec = _run(torch, pool, act_in)
        assert (rec["point"][:k, 0] == l_in[idx, 3]).all() and (rec["point"][:k, 1] == l_in[idx, 4]).all()
        assert ((rec["events"][:k] & L.PURSUIT_ROUTE_END) != 0).all()
        nan = np.isnan(want[idx])
        assert (((rec["events"][:k] & L.PURSUIT_NONFINITE) != 0) == nan).all() and (np.isnan(rec["action"][:k, 0]) == nan).all()
        assert (got[:k][nan].view(np.uint32) == act_in[:k][nan].view(np.uint32)).all()      # 0 / 0: the caller's row
        diff = np.abs(rec["action"][:k, 0][~nan] - want[idx][~nan])
        worst = max(worst, diff.max(initial=0.0))
        n_nan += int(nan.sum())
        n_half_pi += int((np.abs(rec["action"][:k, 0]) == np.pi / 2).sum())
        assert (rec["action"][:k, 1][~nan] == 0.25).all()
    print("steering: largest deviation from the reference", worst, "; NaN outcomes", n_nan, ", +-pi/2 outcomes", n_half_pi)
    few = 1 if shape != (2, 64) else 30   # (the slices of the small pools hold a handful of coincident calls, the full set ~150)
    assert worst <= TOL and n_nan >= few and n_half_pi >= few
    pool.close()


# ---------------------------------------------------------------------------------------------------- 2. the walk
def _walk_cases():
    """(route, pose, look-ahead): the known answers of tests/test_pursuit.py"""
    L = np.float32([(0, 0), (8, 0), (8, 4), (20, 4), (20, -30)])
    Z = np.float32([(0, 0), (4, 0), (4, 0), (4, 0), (4, 8), (4, 8), (9, 8)])
    ring = RS.roundabout_routes(40.0)[0]
    side = 2 * 14.0 * np.sin(np.pi / 24)
    mid = np.float32(0.5 * (ring[22].astype(np.float64) + ring[23]))
    return [(np.float32([(0, 0), (16, 0)]), (4, 1), 8.0), (L, (4, -1), 4.0), (L, (4, 2), 8.0), (L, (2, 0), 27.0), (Z, (1, 0), 13.0),
            (Z, (1, 0), 3.0), (Z, (1, 0), 3.5), (np.float32([(0, 0), (4, 0), (4, 3)]), (1, 0), 10.0),
            (np.float32([(0, 0), (4, 0), (4, 3), (4, 3)]), (1, 0), 10.0), (L, (-5, 3), 2.0), (L, (25, -40), 2.0),
            (np.float32([(2, 2), (2, 2), (2, 2)]), (0, 0), 1.0), (ring, mid, 3.0 * side), (ring, mid, 0.25 * side), (ring, mid, 30 * side),
            (ring, (14.0, 0.2), 30 * side), (ring, (14.0, 0.2), 5.0), (ring, (13.0, -0.5), 5.0)]


def _walk_batch(torch, pool, n_env, A, routes, x, y, h, v, R, ts=5.0):
    n = n_env * A
    _set_pose(pool, x, y, h, v, np.zeros(n, np.float32))
    pool.set_routes(_per_env(routes, n_env, A), np.arange(n_env), np.tile(np.arange(A), n_env), 0.0)
    pool.set_pursuit(R, np.arange(n).astype(np.uint8) if len(R) == n else np.zeros(n, np.uint8), ts)
    got, rec = _run(torch, pool)
    rows = R if len(R) == n else np.repeat(R, n, 0)
    want = UR.evaluate(rows, np.ones(n, bool), x, y, h, v, np.zeros(n), np.ones(n), np.full(n, ts), routes, np.arange(n), np.full(n, _types()[2]))
    return got, rec, want


@pytest.mark.parametrize("shape", SHAPES)
def test_walk_known_answers_and_random_poses(torch, shape):
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    pool = _pool(n_env, A)
    base = US.ring_controller().row()
    # the known answers: one row per participant, its look-ahead in MIN_PRE_AIMING, speed 0
    cases = _walk_cases()
    seen = 0
    for lo in range(0, len(cases), n):
        batch = [cases[(lo + j) % len(cases)] for j in range(n)]
        R = np.repeat(base[None], n, 0)
        R[:, UR.MIN_PRE_AIMING] = [b[2] for b in batch]
        x, y = np.float32([b[1][0] for b in batch]), np.float32([b[1][1] for b in batch])
        got, rec, want = _walk_batch(torch, pool, n_env, A, [b[0] for b in batch], x, y, np.linspace(-3, 3, n).astype(np.float32),
                                     np.zeros(n, np.float32), R)
        _check(got, rec, want, f"known answers {lo}..")
        seen |= int(np.bitwise_or.reduce(rec["events"]))
    assert seen & L.PURSUIT_ROUTE_END and seen & L.PURSUIT_WRAPPED and seen & L.PURSUIT_NO_ROUTE
    # random poses around the benchmark's routes; the look-ahead comes from the speed (2 m at rest, up to 60 m)
    pool_routes = RS.roundabout_routes(40.0) + RS.intersection_routes(60.0) + RS.highway_routes()
    rng = np.random.default_rng(100 + A)
    R = base[None].copy()
    R[:, UR.MIN_PRE_AIMING] = 2.0
    worst = 0.0
    events = 0
    for rep in range(3):
        which = rng.integers(0, len(pool_routes), n)
        routes = [pool_routes[k] for k in which]
        at = np.float32([r[rng.integers(0, len(r))] for r in routes])
        x, y = np.float32(at[:, 0] + rng.normal(0, 1.5, n)), np.float32(at[:, 1] + rng.normal(0, 1.5, n))
        h, v = np.float32(rng.uniform(-4, 4, n)), np.float32(rng.choice([0.0, 3.0, 9.0, 25.0, 60.0], n) * rng.uniform(0.5, 1, n))
        got, rec, want = _walk_batch(torch, pool, n_env, A, routes, x, y, h, v, R)
        _check(got, rec, want, f"random poses {rep}")
        worst = max(worst, np.nanmax(np.abs(rec["point"] - want["point"]), initial=0.0), np.nanmax(np.abs(rec["action"] - want["action"]), initial=0.0))
        events |= int(np.bitwise_or.reduce(rec["events"]))
    print("random poses: largest deviation of point / action from pursuit_ref", worst, "events seen", events)
    pool.close()


def test_walk_at_the_vertex_cap(torch):
    from tactics2d_amd import layout as L
    k = np.arange(L.MAX_ROUTE_SET_VERTS)
    long_route = np.float32(np.stack([0.5 * k - 1000.0, 3.0 * np.sin(0.05 * k)], 1))   # 4096 vertices: the whole set
    n_env, A = 3, 3
    n = n_env * A
    pool = _pool(n_env, A)
    rng = np.random.default_rng(3)
    at = rng.integers(0, len(k), n)
    at[0], at[1], at[2] = 0, len(k) - 1, len(k) - 30
    x = (long_route[at, 0] + rng.normal(0, 0.3, n)).astype(np.float32)
    y = (long_route[at, 1] + rng.normal(0, 0.8, n)).astype(np.float32)
    h = np.zeros(n, np.float32)
    v = np.float32(rng.uniform(0, 40, n))
    v[0] = 3000.0                                                                        # past the whole route: 4095 segments walked
    _set_pose(pool, x, y, h, v, np.zeros(n, np.float32))
    pool.set_routes([[long_route]], None, 0, 0.0)
    R = US.ring_controller().row()[None]
    pool.set_pursuit(R, np.zeros(n, np.uint8), 5.0)
    got, rec = _run(torch, pool)
    want = UR.evaluate(np.repeat(R, n, 0), np.ones(n, bool), x, y, h, v, np.zeros(n), np.ones(n), np.full(n, 5.0), [long_route], np.zeros(n, int),
                       np.full(n, _types()[2]))
    _check(got, rec, want, "cap")
    assert rec["segment"].max() > 2000 and rec["target_segment"][0] == len(k) - 2 and (rec["events"][:2] & L.PURSUIT_ROUTE_END).all()
    assert (rec["point"][0] == long_route[-1]).all()
    pool.close()


# ---------------------------------------------------------------------------------------------------- 3. the shared measurement
@pytest.mark.parametrize("shape", SHAPES)
def test_projection_equals_the_pid_record(torch, shape):
    """the same poses through t2d_pid_actions and t2d_pursuit_actions: segment and cross-track error bit for bit"""
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    pool_routes = RS.roundabout_routes(40.0) + RS.intersection_routes(60.0) + [np.float32([[0, 0], [4, 0], [4, 0], [4, 4], [4, 4]])]
    rng = np.random.default_rng(7 + A)
    which = rng.integers(0, len(pool_routes), n)
    routes = [pool_routes[k] for k in which]
    at = np.float32([r[rng.integers(0, len(r))] for r in routes])
    x, y = np.float32(at[:, 0] + rng.normal(0, 2.0, n)), np.float32(at[:, 1] + rng.normal(0, 2.0, n))
    h, v = np.float32(rng.uniform(-3, 3, n)), np.float32(rng.uniform(0, 10, n))
    pool = _pool(n_env, A, x, y, h, v)
    pool.set_routes(_per_env(routes, n_env, A), np.arange(n_env), np.tile(np.arange(A), n_env), 0.0)
    c = PS.ring_controller()
    c.configure(control_mode="lateral")
    pool.set_pid(c.row()[None], np.zeros(n, np.uint8))
    out = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    prec = torch.zeros((n, L.PID_RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
    pool.pid_actions(None, out.data_ptr(), prec.data_ptr())
    pool.sync()
    p = prec.cpu().numpy()
    pid_cte, pid_seg = p[:, 0], p.view(np.int32).reshape(n, -1)[:, 4]
    pool.set_pid(None)
    pool.set_pursuit(US.ring_controller().row()[None], np.zeros(n, np.uint8), 5.0)
    got, rec = _run(torch, pool)
    assert np.isfinite(pid_cte).all() and (pid_cte != 0).sum() > n // 2
    assert (rec["segment"] == pid_seg).all() and (rec["cross_track"].view(np.uint64) == pid_cte.view(np.uint64)).all()
    pool.close()


# ---------------------------------------------------------------------------------------------------- 4. ACC's leader
@pytest.mark.parametrize("shape", SHAPES)
def test_acc_leader_equals_idm_actions(torch, shape):
    from tactics2d_amd import layout as L
    from tactics2d_amd.controller import IDMController
    n_env, A = shape
    n = n_env * A
    rng = np.random.default_rng(A)
    # test_gpu_pid's platoon: a gentle line, two lanes, some inactive: leaders far down the list and across wave boundaries
    s = rng.permutation(n).astype(np.float64) * 6.0 + rng.uniform(-1, 1, n)
    lane = rng.integers(0, 2, n) * 3.75
    x, y = np.float32(s * np.cos(0.1) - lane * np.sin(0.1)), np.float32(s * np.sin(0.1) + lane * np.cos(0.1))
    h = np.float32(0.1 + rng.normal(0, 0.02, n))
    v = np.float32(rng.uniform(0, 15, n))
    a = np.float32(rng.uniform(-4, 1.5, n))
    active = (rng.random(n) > 0.1).astype(np.uint8)
    rule = [(1.875, np.inf), (1.875, 40.0), (6.0, np.inf)]
    idm_rows = np.stack([IDMController(lane_half_width=hw, horizon=hz).row() for hw, hz in rule])
    which = rng.integers(0, 3, n).astype(np.uint8)
    twin = _pool(n_env, A, x, y, h, v, active)
    twin.set_idm(idm_rows, which)
    twin.idm_actions()
    twin.sync()
    lead = twin.download(L.F_LEADER)
    twin.close()
    pool = _pool(n_env, A, x, y, h, v, active)
    _set_pose(pool, None, None, None, None, a)
    R = np.repeat(US.ring_controller().row("acc")[None], 3, 0)
    R[:, UR.LAT_MODE] = 0
    R[:, UR.LANE_HALF_WIDTH], R[:, UR.HORIZON] = np.float64(rule).T
    ts = np.float32(rng.uniform(0, 15, n))
    pool.set_pursuit(R, which, ts)
    act_in = rng.uniform(-1, 1, (n, 2)).astype(np.float32)
    got, rec = _run(torch, pool, act_in)
    on = active != 0
    assert (rec["leader"][on] == lead[on]).all() and (rec["leader"][~on] == -1).all() and (lead[on] >= 0).sum() > n // 4
    assert (((rec["events"] & L.PURSUIT_NO_LEADER) != 0) == (on & (lead < 0))).all() and (on & (lead < 0)).any()
    if A > 64:
        follower = np.flatnonzero(on & (lead >= 0))
        assert ((lead[follower] // 64) != ((follower % A) // 64)).sum() > 10          # the leader sits in another wave
    want = UR.evaluate(R[which], np.ones(n, bool), x, y, h, v, a, active, ts, [], np.full(n, -1), np.full(n, _types()[2]), act_in, lead, A)
    _check(got, rec, want, "acc")
    diff = np.abs(rec["action"][on, 1] - want["action"][on, 1])
    print("ACC against pursuit_ref: largest deviation", diff.max(), "; bit-equal in", int((diff == 0).sum()), "of", int(on.sum()))
    assert (got[~on].view(np.uint32) == act_in[~on].view(np.uint32)).all() and (got[on, 0] == 0.0).all()
    pool.close()


# ---------------------------------------------------------------------------------------------------- 5. bookkeeping
def _small(torch, longitudinal="cruise", active=None, **kw):
    """3 x 3 on a straight route east through y = 0; participants 0, 3, 6 uncontrolled -> (pool, ctrl, ref, pose, target_speed)"""
    from tactics2d_amd import layout as L
    n = 9
    rng = np.random.default_rng(17)
    x, y = np.float32(rng.uniform(-50, 50, n)), np.float32(rng.normal(0, 0.6, n))
    h, v = np.float32(rng.normal(0, 0.1, n)), np.float32(rng.uniform(3, 9, n))
    a = np.float32(rng.uniform(-1, 1, n))
    pool = _pool(3, 3, x, y, h, v, active)
    _set_pose(pool, None, None, None, None, a)
    pool.set_routes([[STRAIGHT]], None, 0, 0.0)
    ctrl = np.where(np.arange(n) % 3 == 0, L.PURSUIT_NONE, 0).astype(np.uint8)
    c = US.ring_controller()
    c.configure(**kw)
    ts = np.float32(rng.uniform(3, 9, n))
    pool.set_pursuit(c.row(longitudinal)[None], ctrl, ts)

    def ref(act_in=None, active=None, pose=None, route_index=None):
        px, py, ph, pv, pa = pose if pose is not None else (x, y, h, v, a)
        return UR.evaluate(np.repeat(c.row(longitudinal)[None], n, 0), ctrl != L.PURSUIT_NONE, px, py, ph, pv, pa,
                           np.ones(n) if active is None else active, ts, [STRAIGHT], np.zeros(n, int) if route_index is None else route_index,
                           np.full(n, _types()[2]), act_in)
    return pool, ctrl, ref, (x, y, h, v, a), ts


def test_rows_copied_aliased_and_null_input(torch):
    from tactics2d_amd import layout as L
    pool, ctrl, ref, _, ts0 = _small(torch)
    act_in = np.random.default_rng(2).uniform(-1, 1, (9, 2)).astype(np.float32)
    act_in[0] = [np.nan, -0.0]                         # an uncontrolled row goes through bit for bit, whatever it holds
    act_in.view(np.uint32)[3] = [0x7fc12345, 0xff800000]
    got, rec = _run(torch, pool, act_in)               # (asserts that act_in is unchanged)
    _check(got, rec, ref(act_in))
    free = ctrl == L.PURSUIT_NONE
    assert (got[free].view(np.uint32) == act_in[free].view(np.uint32)).all()
    assert np.isnan(rec["action"][free]).all() and (rec["events"][free] == 0).all() and (rec["segment"][free] == -1).all()
    assert np.isfinite(rec["action"][~free]).all() and (got[~free] != act_in[~free]).all()
    # NULL act_in = zeros
    got0, rec0 = _run(torch, pool, None)
    _check(got0, rec0, ref(None))
    assert (got0[free].view(np.uint32) == 0).all() and (got0[~free].view(np.uint32) == got[~free].view(np.uint32)).all()
    # in and out the same memory; the pool's own records
    t = torch.as_tensor(act_in.copy(), device="cuda")
    pool.pursuit_actions(t.data_ptr(), t.data_ptr(), None)
    pool.sync()
    assert (t.cpu().numpy().view(np.uint32) == got.view(np.uint32)).all()
    own = pool.pursuit_records()
    for key in ("action", "point", "cross_track", "distance", "pre_aiming_distance"):
        assert _same(own[key].cpu().numpy(), rec[key]), key
    for key in ("segment", "target_segment", "leader"):
        assert (own[key].cpu().numpy() == rec[key]).all(), key
    assert (own["events"].cpu().numpy().view(np.uint32) == rec["events"]).all()
    # the caller's acceleration (lon_mode 2): the steering is the law's, the acceleration the caller's fp32
    pool.close()
    pool, ctrl, ref, _, ts0 = _small(torch, "caller")
    got, rec = _run(torch, pool, act_in)
    _check(got, rec, ref(act_in))
    on = ctrl != L.PURSUIT_NONE
    assert (got[on, 1].view(np.uint32) == act_in[on, 1].view(np.uint32)).all() and (got[on, 0] != act_in[on, 0]).all()
    pool.close()


def test_inactive_nonfinite_and_no_route_rows(torch):
    from tactics2d_amd import layout as L
    active = np.ones(9, np.uint8); active[4] = 0
    pool, ctrl, ref, (x, y, h, v, a), ts0 = _small(torch, active=active)
    x, y, h, v, a = x.copy(), y.copy(), h.copy(), v.copy(), a.copy()
    x[1], h[5], v[7], a[8] = np.nan, np.inf, np.nan, -np.inf
    _set_pose(pool, x, y, h, v, a)
    route_of = np.zeros(9, np.int32); route_of[2] = -1
    pool.set_route_assignment(route_of, None)
    act_in = np.random.default_rng(5).uniform(-1, 1, (9, 2)).astype(np.float32)
    got, rec = _run(torch, pool, act_in)
    for i in (1, 5, 7, 8):   # non-finite pose, speed or stored acceleration: the caller's row goes through
        assert rec["events"][i] == L.PURSUIT_NONFINITE and (got[i].view(np.uint32) == act_in[i].view(np.uint32)).all()
        assert np.isnan(rec["action"][i]).all() and rec["segment"][i] == -1
    assert rec["events"][4] == 0 and (got[4].view(np.uint32) == act_in[4].view(np.uint32)).all()            # inactive
    # no route: steering 0.0, the longitudinal side acts
    assert rec["events"][2] == L.PURSUIT_NO_ROUTE and got[2, 0] == 0.0 and got[2, 1] != act_in[2, 1] and np.isfinite(rec["action"][2]).all()
    assert np.isnan(rec["cross_track"][2]) and rec["segment"][2] == -1 and np.isnan(rec["point"][2]).all()
    assert np.isfinite(rec["pre_aiming_distance"][2])
    _check(got, rec, ref(act_in, active, (x, y, h, v, a), route_of))
    # a non-finite target speed is a non-finite input under cruise -- and none when the caller's acceleration is used
    pool.close()
    for lon, hit in (("cruise", True), ("caller", False)):
        pool, ctrl, ref, _, ts0 = _small(torch, lon)
        ts = np.full(9, 5.0, np.float32); ts[1] = np.inf
        pool.set_pursuit(US.ring_controller().row(lon)[None], ctrl, ts)
        got, rec = _run(torch, pool, act_in)
        assert bool(rec["events"][1] & L.PURSUIT_NONFINITE) == hit and np.isnan(rec["action"][1, 0]) == hit and rec["events"][2] == 0
        pool.close()


def test_a_nonfinite_result_passes_the_row_through_and_inf_that_a_clip_tames_is_kept(torch):
    from tactics2d_amd import layout as L
    act_in = np.random.default_rng(9).uniform(-1, 1, (9, 2)).astype(np.float32)
    # kp = 0 is not refused: (target - speed) / 0 = +-inf, which the clips make finite -- kept
    pool, ctrl, ref, (x, y, h, v, a), ts0 = _small(torch)
    c = US.ring_controller()
    c._longitudinal_control.configure(kp=0.0)
    ts = np.float32(v + np.where(np.arange(9) % 2, 1.0, -1.0))
    pool.set_pursuit(c.row()[None], ctrl, ts)
    got, rec = _run(torch, pool, act_in)
    on = ctrl != L.PURSUIT_NONE
    step = 3.0 * 0.1
    want = np.clip(np.clip(np.where(np.arange(9) % 2, np.inf, -np.inf), a.astype(np.float64) - step, a.astype(np.float64) + step), -4.0, 1.5)
    assert (rec["events"][on] == 0).all() and (rec["action"][on, 1] == want[on]).all()
    # ... and 0 / 0 where target_speed equals the speed: NaN, the caller's row
    pool.set_pursuit(c.row()[None], ctrl, v)
    got, rec = _run(torch, pool, act_in)
    assert (rec["events"][on] == L.PURSUIT_NONFINITE).all() and (got.view(np.uint32) == act_in.view(np.uint32)).all()
    assert np.isnan(rec["action"]).all() and np.isfinite(rec["point"][on]).all() and (rec["segment"][on] == 0).all()   # the walk was made
    pool.close()
    # the look-ahead point coincides with the position and the heading equals the bearing: 0 / 0 in the steering
    pool = _pool(3, 3, np.full(9, 4.0, np.float32), np.zeros(9, np.float32), np.zeros(9, np.float32), np.ones(9, np.float32))
    pool.set_routes([[np.float32([[0, 0], [4, 0]])]], None, 0, 0.0)
    c = US.ring_controller()
    pool.set_pursuit(c.row()[None], np.zeros(9, np.uint8), 5.0)
    got, rec = _run(torch, pool, act_in)
    assert (rec["events"] == (L.PURSUIT_NONFINITE | L.PURSUIT_ROUTE_END)).all() and (got.view(np.uint32) == act_in.view(np.uint32)).all()
    assert (rec["point"] == [4.0, 0.0]).all() and (rec["distance"] == 0.0).all() and np.isnan(rec["action"]).all()
    # with another heading: +-inf, which atan makes +-pi/2 -- kept
    _set_pose(pool, None, None, np.full(9, 0.5, np.float32), None)
    got, rec = _run(torch, pool, act_in)
    assert (rec["events"] == L.PURSUIT_ROUTE_END).all() and (rec["action"][:, 0] == -np.pi / 2).all()
    pool.close()


def _refusal_kit(torch):
    """_small's pool with what the refusal tests share: `works()` -- a launch still gives the rows of the first one -- and
    `refused(code, rows, cid, ts)` -- set_pursuit raises `code` and the installation works as before"""
    from tactics2d_amd import _ffi
    pool, ctrl, ref, _, ts0 = _small(torch)
    before, _ = _run(torch, pool)
    good = US.ring_controller().row()
    ts_good = np.full(9, 5.0, np.float32)

    def works():
        again, _ = _run(torch, pool)
        assert (again.view(np.uint32) == before.view(np.uint32)).all()

    def refused(code, rows, cid=ctrl, ts=ts_good):
        with pytest.raises(_ffi.T2DError) as ei:
            pool.set_pursuit(rows, cid, ts)
        assert ei.value.code == code
        works()
    return pool, ctrl, ts0, before, good, ts_good, works, refused


def test_set_pursuit_refusals_leave_the_installation_working(torch):
    from tactics2d_amd import _ffi, layout as L
    pool, ctrl, ts0, before, good, ts_good, works, refused = _refusal_kit(torch)
    for col, bad in ((L.PURSUIT_MIN_PRE_AIMING, 0.0), (L.PURSUIT_MIN_PRE_AIMING, -1.0), (L.PURSUIT_LAT_MODE, 2.0), (L.PURSUIT_LAT_MODE, 0.5),
                     (L.PURSUIT_LON_MODE, 3.0), (L.PURSUIT_LON_MODE, -1.0), (L.PURSUIT_KP, np.nan), (L.PURSUIT_DELTA_T, np.inf),
                     (L.PURSUIT_HORIZON, np.nan), (L.PURSUIT_HORIZON, -np.inf), (L.PURSUIT_WHEEL_BASE, np.inf),
                     (L.PURSUIT_LANE_HALF_WIDTH, np.inf), (L.PURSUIT_MIN_PRE_AIMING, np.nan)):
        r = good.copy(); r[col] = bad
        refused(_ffi.ERR_INVALID, r[None])
    refused(_ffi.ERR_INVALID, good[None], np.full(9, 1, np.uint8))                      # a controller id without a row
    refused(_ffi.ERR_INVALID, good[None, :12])                                          # too few columns
    bad_ts = ts_good.copy(); bad_ts[1] = -0.5
    refused(_ffi.ERR_INVALID, good[None], ctrl, bad_ts)                                 # the constructors' target_speed < 0
    bad_ts[1] = np.nan
    refused(_ffi.ERR_INVALID, good[None], ctrl, bad_ts)
    bad_ts[1], bad_ts[0] = 5.0, -3.0                                                    # (participant 0 is uncontrolled: not looked at)
    pool.set_pursuit(good[None], ctrl, bad_ts)
    kp0 = good.copy(); kp0[L.PURSUIT_KP] = 0.0                                          # kp = 0 is accepted, as in the reference
    pool.set_pursuit(kp0[None], ctrl, ts_good)
    pool.close()


def test_one_controller_per_participant_in_all_three_directions(torch):
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.controller import IDMController, PIDController
    pool, ctrl, ts0, before, good, ts_good, works, refused = _refusal_kit(torch)
    idm_row, pid_row = IDMController().row()[None], PIDController(dt=0.1).row()[None]
    only0 = lambda none: np.where(np.arange(9) == 0, 0, none).astype(np.uint8)
    for call in (lambda: pool.set_idm(idm_row, np.zeros(9, np.uint8)), lambda: pool.set_pid(pid_row, np.zeros(9, np.uint8), 5.0)):
        with pytest.raises(_ffi.T2DError) as ei:                                        # participants 1, 2, ... are pursuit-controlled
            call()
        assert ei.value.code == _ffi.ERR_INVALID
        works()
    pool.set_idm(idm_row, only0(L.IDM_NONE))                                            # participant 0 is not: accepted, as before
    works()
    refused(_ffi.ERR_INVALID, good[None], np.zeros(9, np.uint8))                        # ... and now IDM-controlled
    pool.set_idm(None, None)
    pool.set_pid(pid_row, only0(L.PID_NONE), 5.0)
    works()
    refused(_ffi.ERR_INVALID, good[None], np.zeros(9, np.uint8))                        # ... and now PID-controlled
    pool.set_pid(None)
    pool.set_pursuit(good[None], np.zeros(9, np.uint8), ts_good)                        # free again
    pool.set_pursuit(good[None], ctrl, ts0)
    works()
    pool.close()


def test_pursuit_actions_refusals_leave_the_installation_working(torch):
    from tactics2d_amd import _ffi, layout as L
    pool, ctrl, ts0, before, good, ts_good, works, refused = _refusal_kit(torch)

    def raises(code, call):
        with pytest.raises(_ffi.T2DError) as ei:
            call()
        assert ei.value.code == code

    # no output, a misaligned record
    raises(_ffi.ERR_INVALID, lambda: pool.pursuit_actions(None, None))
    t = torch.zeros((9, 2), dtype=torch.float32, device="cuda")
    r = torch.zeros((9 * L.PURSUIT_RECORD_BYTES // 8 + 1,), dtype=torch.float64, device="cuda")
    raises(_ffi.ERR_INVALID, lambda: pool.pursuit_actions(None, t.data_ptr(), r.data_ptr() + 4))
    works()
    # no routes: refused with a lateral side, not needed without one
    pool.clear_routes()
    raises(_ffi.ERR_STATE, lambda: _run(torch, pool))
    no_lat = good.copy(); no_lat[L.PURSUIT_LAT_MODE] = 0
    pool.set_pursuit(no_lat[None], ctrl, ts0)
    got, rec = _run(torch, pool)
    on = ctrl != L.PURSUIT_NONE
    assert (got[on, 1].view(np.uint32) == before[on, 1].view(np.uint32)).all() and (got[:, 0] == 0).all()
    pool.set_pursuit(good[None], ctrl, ts0)
    pool.set_routes([[STRAIGHT]], None, 0, 0.0)
    works()
    # the applied acceleration is no longer stored: cruise has no accel_last -- refused; the caller's acceleration needs none
    pool.set_outputs(applied=False)
    raises(_ffi.ERR_STATE, lambda: _run(torch, pool))
    pool.set_pursuit(US.ring_controller().row("caller")[None], ctrl, ts0)
    _run(torch, pool)
    pool.set_outputs()
    pool.set_pursuit(good[None], ctrl, ts0)
    works()
    # uninstalled: every pursuit call is refused
    pool.set_pursuit(None)
    raises(_ffi.ERR_STATE, lambda: _run(torch, pool))
    raises(_ffi.ERR_STATE, pool.pursuit_records)
    pool.close()
    # before t2d_reset
    from tactics2d_amd.pool import ParticipantPool
    fresh = ParticipantPool(1, 2)
    fresh.set_param_table(_types()[0])
    fresh.set_pursuit(no_lat[None], np.zeros(2, np.uint8), 5.0)
    t2 = torch.zeros((2, 2), dtype=torch.float32, device="cuda")
    raises(_ffi.ERR_STATE, lambda: fresh.pursuit_actions(None, t2.data_ptr()))
    fresh.close()


def test_trace_routes_are_refused(torch):
    from tactics2d_amd import _ffi
    from tactics2d_amd.history import DeviceTrajectory
    pool, ctrl, ref, _, ts0 = _small(torch)
    traj = DeviceTrajectory(pool, 0, capacity=4)
    for k in range(3):
        traj.record(pool, 100 * k)
    pool.set_routes_from(traj)
    with pytest.raises(_ffi.T2DError) as ei:
        _run(torch, pool)
    assert ei.value.code == _ffi.ERR_STATE
    pool.clear_routes()
    traj.close()
    pool.close()


def test_profile_counts_one_launch_per_call_and_none_from_stepping(torch):
    from tactics2d_amd import layout as L
    pool, ctrl, ref, _, ts0 = _small(torch)
    pool.profile_enable(True)
    for _ in range(3):
        _run(torch, pool)
    assert pool.profile_read(L.PROFILE_PURSUIT)[1] == 3 and pool.profile_read(L.PROFILE_PID)[1] == 0
    pool.profile_enable(True)   # (clears the counts)
    pool.step(100)
    pool.step_n(3, 100)
    pool.integrate(100)
    pool.collide()
    pool.sync()
    assert pool.profile_read(L.PROFILE_PURSUIT)[1] == 0
    pool.close()
    # a pool with pursuit rows enqueues exactly what it did without them: the same kernels, the same counts, the same state
    counts = []
    for install in (False, True):
        sc, route_of, ts = PS.ring_scene(2, 16)
        from tactics2d_amd.pool import ParticipantPool
        p = ParticipantPool(sc.n_env, sc.A)
        sc.load(p)
        if install:
            p.set_routes([PS.ring_routes()], None, route_of, 0.0)
            p.set_pursuit(US.ring_controller().row()[None], np.zeros(sc.n, np.uint8), ts)
        p.profile_enable(True)
        p.step(100)
        p.step_n(4, 100)
        p.sync()
        counts.append(([p.profile_read(k)[1] for k in range(17)], p.download(L.F_X), p.download(L.F_HEADING)))
        p.close()
    assert counts[0][0] == counts[1][0] and counts[0][0][L.PROFILE_PURSUIT] == 0
    assert (counts[0][1] == counts[1][1]).all() and (counts[0][2] == counts[1][2]).all()


# ---------------------------------------------------------------------------------------------------- 6. the closed loop
def test_closed_loop_on_the_rings(torch, oracle):
    from tactics2d_amd import layout as L
    from tactics2d_amd.controller import PathFollower, install_pursuit
    from tactics2d_amd.pool import ParticipantPool
    want_rows, want_cte, want_events, want_states = US.ring_rollout(oracle)
    sc, route_of, ts = PS.ring_scene()
    n, steps = sc.n, US.RING_STEPS
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    pool.set_integrator_variant("exact")
    pool.set_routes([PS.ring_routes()], None, route_of, PS.OFF_ROUTE_THRESHOLD)
    install_pursuit(pool, [US.ring_controller()], np.zeros(n, np.uint8), ts)
    follower = PathFollower(pool)
    rows = torch.zeros((steps, n, 2), dtype=torch.float32, device="cuda")
    cte = torch.zeros((steps, n), dtype=torch.float64, device="cuda")
    events = torch.zeros((steps, n), dtype=torch.int32, device="cuda")
    for k in range(steps):
        r = follower.follow(None, rows[k])
        cte[k], events[k] = r["cross_track"], r["events"]
        p = rows[k].data_ptr()
        pool.bind_actions(p + 4, p, stride=2)
        pool.step(sc.interval_ms)
    pool.sync()
    got_rows, got_cte, got_events = rows.cpu().numpy(), cte.cpu().numpy(), events.cpu().numpy()
    assert np.isfinite(got_cte).all() and np.isfinite(got_rows).all()
    assert not (got_events & (L.PURSUIT_NO_ROUTE | L.PURSUIT_NONFINITE | L.PURSUIT_ROUTE_END)).any() and (got_events & L.PURSUIT_WRAPPED).any()
    excess, signed, settled = US.ring_figures(got_cte)
    half = got_cte[steps // 2:].mean(0)
    print("largest excess", excess, "largest |mean signed|", signed, "settled", settled, "signed means", half.min(), half.max(),
          "; against the CPU run: largest |d row|", np.abs(got_rows - want_rows).max(), "largest |d cross-track|", np.abs(got_cte - want_cte).max(),
          "steps with every row bit-equal", int((got_rows.view(np.uint32) == want_rows.view(np.uint32)).all((1, 2)).sum()), "of", steps)
    assert excess <= US.RING_MARGIN and signed <= US.RING_SIGNED and settled <= US.RING_SETTLED and half.max() < 0
    assert np.abs(got_cte).max() < PS.OFF_ROUTE_THRESHOLD
    dist, off = pool.off_route_host()
    assert not off.any()
    pool.bind_actions(None, None)
    pool.close()
