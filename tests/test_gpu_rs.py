"""The Reeds-Shepp kernels on the device: t2d_rs_paths against the fixture made by running the reference
(tests/golden/reeds_shepp.npz) and against the reference-free word-integration property on fresh inputs; t2d_rs_plan against
the specification (tests/rs_ref.py) on synthetic scans, inside VecParkingEnv, and at its edges."""
import numpy as np
import pytest

import rs_ref as R
import rs_scenes as S

pytestmark = pytest.mark.gpu
TOL = 1e-9   # see tests/test_rs.py


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _run(torch, radius, start, goal):
    from tactics2d_amd.interpolator import ReedsShepp
    r = ReedsShepp(radius).get_all_path(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2])
    torch.cuda.synchronize()
    return dict(valid=r.valid.cpu().numpy(), seg=r.segments.cpu().numpy(), length=r.length.cpu().numpy(),
                shortest=r.shortest.cpu().numpy(), first=r.shortest_first.cpu().numpy(), mask=r.mask.cpu().numpy())


@pytest.fixture(scope="module")
def device_paths(torch):
    """all 4000 queries of the fixture in one launch per radius"""
    g = S.fixture()
    return [_run(torch, float(r), g["start"], g["goal"]) for r in g["radius"]]


@pytest.mark.parametrize("which", [0, 1])
def test_paths_agree_with_the_reference(device_paths, which):
    g = S.fixture()
    d = device_paths[which]
    rows = g["query_radius"] == which
    st = rows & g["stable"].astype(bool)
    assert np.array_equal(d["valid"][st], g["valid"][st])
    assert np.array_equal(d["mask"].view(np.uint64)[st], g["valid_mask"][st])
    both = d["valid"] & g["valid"] & rows[:, None]
    err_s = np.abs(d["seg"] - g["seg"])[both].max()
    err_l = (np.abs(d["length"][both] - g["length"][both]) / np.maximum(1.0, g["length"][both])).max()
    print("segments", err_s, "length", err_l, "rows", int(rows.sum()))
    assert err_s <= TOL and err_l <= TOL
    # None: zero segments, +inf length
    assert (d["seg"][~d["valid"]] == 0).all() and np.isinf(d["length"][~d["valid"]]).all() and np.isfinite(d["length"][d["valid"]]).all()
    two = np.sort(g["length"], 1)[:, :2]
    clear = st & ~(two[:, 1] - two[:, 0] <= TOL)
    assert np.array_equal(d["shortest"][clear], g["get_path"][clear])
    # the two tie rules, from the device's own lengths
    last, first = R.shortest_slots(d["length"])
    assert np.array_equal(d["shortest"], last) and np.array_equal(d["first"], first)


def test_shortest_length_at_the_degenerate_goals(torch):
    g = S.fixture()
    for r in g["radius"]:
        k = g["deg_radius"] == r
        d = _run(torch, float(r), g["deg_start"][k], g["deg_goal"][k])
        err = np.abs(d["length"].min(1) - g["deg_shortest"][k]).max()
        print("radius", r, "shortest length error", err)
        assert err <= TOL


@pytest.mark.parametrize("n", [1, 63, 65])
def test_block_edges(torch, device_paths, n):
    g = S.fixture()
    d = _run(torch, float(g["radius"][0]), g["start"][:n], g["goal"][:n])
    for k in ("mask", "seg", "length", "shortest", "first"):
        assert d[k].shape[0] == n and np.array_equal(d[k], device_paths[0][k][:n], equal_nan=True), k


def test_words_integrate_to_the_goal_on_fresh_inputs(torch):
    rng = np.random.default_rng(991)
    n, radius = 2000, 3.3
    start = np.concatenate([rng.uniform(-25, 25, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(-14, 14, (n, 2)), rng.uniform(-7, 7, (n, 1))], 1)
    d = _run(torch, radius, start, goal)
    assert d["valid"].any(1).all()
    x, y, phi = R.normalise(start, goal, radius)
    worst = 0.0
    for s in range(48):
        k = d["valid"][:, s]
        if not k.any():
            continue
        ex, ey, eyaw = R.integrate(s, d["seg"][k, s])
        dyaw = np.abs((eyaw - phi[k] + np.pi) % (2 * np.pi) - np.pi)
        worst = max(worst, np.abs(ex - x[k]).max(), np.abs(ey - y[k]).max(), dyaw.max())
        assert np.abs(np.abs(d["seg"][k, s]).sum(1) * radius - d["length"][k, s]).max() <= TOL * 100
    print("worst end-pose error", worst)
    assert worst <= TOL


def test_get_path_and_numpy_or_tensor_inputs(torch):
    from tactics2d_amd.interpolator import ReedsShepp
    g = S.fixture()
    rs = ReedsShepp(float(g["radius"][0]))
    s, e = g["start"][:100], g["goal"][:100]
    a = rs.get_path(s[:, :2], s[:, 2], e[:, :2], e[:, 2])
    t = lambda v: torch.as_tensor(v, device="cuda")
    b = rs.get_path(t(s[:, :2].copy()), t(s[:, 2].copy()), t(e[:, :2].copy()), t(e[:, 2].copy()))
    for k in ("slot", "segments", "steer", "n_seg", "length"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    # packed float64 [n, 3] poses are read in place
    ps, pe = t(s.copy()), t(e.copy())
    c = rs.get_all_path(ps, None, pe, None)
    assert c._inputs[0].data_ptr() == ps.data_ptr() and c._inputs[1].data_ptr() == pe.data_ptr()
    assert torch.equal(c.shortest, a.slot) and torch.equal(c.length[torch.arange(100), a.slot.long()], a.length)
    slot = a.slot.cpu().numpy()
    two = np.sort(g["length"][:100], 1)[:, :2]
    clear = ~(two[:, 1] - two[:, 0] <= TOL)   # (equal shortest lengths: the choice hangs on the last bit)
    assert np.array_equal(slot[clear], g["get_path"][:100][clear]) and clear.sum() > 50
    assert np.array_equal(a.steer.cpu().numpy(), g["letters"][slot]) and np.array_equal(a.n_seg.cpu().numpy(), g["n_seg"][slot])
    assert np.abs(a.length.cpu().numpy() - g["length"][np.arange(100), slot]).max() <= TOL * 100


# ---- the planner ---------------------------------------------------------------------------------------------------------------
def _pool(case, n_beams, active=None):
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    from tactics2d_amd.pool import ParticipantPool
    n = len(case["ego"])
    pool = ParticipantPool(n, 1)
    ego = vehicle_model("medium_car", "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0), steer_range=(-0.524, 0.524))
    pool.set_param_table(ego.param_row(L.SHAPE_OBB, *VEHICLE_TEMPLATE["medium_car"][:2])[None])
    pool.set_status_config()
    pool.set_target_areas(case["target"])
    pool.set_target_headings(case["target_heading"])
    z = np.zeros(n, np.float32)
    pool.reset(case["ego"][:, 0], case["ego"][:, 1], case["ego"][:, 2], z, np.zeros(n, np.int32), active)
    pool.lidar_config(n_beams, S.LIDAR_RANGE)
    return pool


def _plan(torch, pool, scan, **overrides):
    from tactics2d_amd.planner import RSPlanner
    planner = RSPlanner(pool, "medium_car", steer_hi=0.524, **overrides)
    out = planner.plan(torch.as_tensor(np.ascontiguousarray(scan, np.float32), device="cuda"))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _compare(got, plans, radius):
    """device records against the specification's plans, envs whose decision is a knife edge left out; returns how many"""
    left_out = 0
    for e, (p, robust) in enumerate(plans):
        if not robust:
            left_out += 1
            continue
        assert got["status"][e] == p.status, (e, got["status"][e], p.status)
        if p.status in (R.FOUND, R.NONE_FREE, R.UNCHECKED):
            assert abs(got["shortest"][e] - p.shortest) <= TOL, e
        else:
            assert np.isnan(got["shortest"][e]), e
        if p.slot < 0:   # no path in the record
            assert got["slot"][e] == -1 and got["n_seg"][e] == 0 and np.isnan(got["length"][e]), e
            assert not got["steer"][e].any() and not got["distance"][e].any(), e
            if p.status != R.NO_TARGET:
                assert got["n_visited"][e] == p.n_visited, e
            continue
        # FOUND, or UNCHECKED at the pose cap: the record carries the slot's path
        assert abs(got["length"][e] - p.length) <= TOL, (e, got["length"][e], p.length)
        seg, length = p.candidates
        r, ranked, slot = p.n_visited - 1, p.sorted_lengths, int(got["slot"][e])
        tie = (r > 0 and ranked[r] - ranked[r - 1] <= TOL) or (r + 1 < len(ranked) and ranked[r + 1] - ranked[r] <= TOL)
        if not tie:   # the chosen candidate's rank is unambiguous: same slot, same number of candidates visited
            assert slot == p.slot and got["n_visited"][e] == p.n_visited, (e, slot, p.slot)
        else:         # a neighbour in rank has the same length to 1e-9: the device may hold that one
            assert 0 <= slot < 48 and abs(length[slot] - p.length) <= TOL, (e, slot, p.slot)
        n = int(R.N_SEG[slot])   # ... and whichever slot it holds, the record is the specification's path of that slot
        assert got["n_seg"][e] == n and np.array_equal(got["steer"][e], R.LETTERS[slot].astype(np.int32)), e
        assert np.abs(got["distance"][e] - seg[slot] * radius).max() <= TOL * radius, e
    return left_out


@pytest.mark.parametrize("n_env,n_beams", [(65, 120), (65, 24), (65, 360), (1, 120)])
def test_plan_agrees_with_the_specification(torch, n_env, n_beams):
    case, plans = S.planner_case(n_env, n_beams), S.spec_plans(n_env, n_beams)
    if n_env == 65:   # from the specification alone: the comparison below cannot go vacuous
        assert min(S.categories(plans).values()) >= 3, S.categories(plans)
    pool = _pool(case, n_beams)
    got = _plan(torch, pool, case["scan"])
    left_out = _compare(got, plans, case["params"].radius)
    print(n_env, n_beams, S.categories(plans), "left out", left_out)
    assert left_out <= 0.02 * n_env
    pool.close()


def test_pose_cap_gives_unchecked_never_free(torch):
    """sample_step = 15 mm: a path longer than some 15.3 m has more than T2D_RS_MAX_POSES poses and stops the plan as UNCHECKED
    with its slot -- as the first candidate or behind swept ones --; shorter ones are still swept"""
    step = 0.015
    case, plans = S.planner_case(65, 120), S.spec_plans(65, 120, sample_step=step)
    capped = [p for p, _ in plans if p.status == R.UNCHECKED]
    swept = [p for p, _ in plans if p.status in (R.FOUND, R.NONE_FREE)]
    print("capped", len(capped), "swept", len(swept), "longest checked", max([p.length for p in swept if p.status == R.FOUND] + [0]))
    assert len(capped) >= 3 and all(p.slot >= 0 and p.n_seg > 0 for p in capped) and len(swept) >= 3
    assert sum(p.n_visited > 1 for p in capped) >= 3 and sum(p.n_visited == 1 for p in capped) >= 3
    pool = _pool(case, 120)
    got = _plan(torch, pool, case["scan"], sample_step=step)
    assert _compare(got, plans, case["params"].radius) <= 0.02 * 65
    pool.close()


def test_plan_in_the_env(torch):
    from tactics2d_amd.envs import VecParkingEnv
    from tactics2d_amd.planner import RSPlanner
    envs = {k: VecParkingEnv(8, lidar_beams=360, seed=3, **kw) for k, kw in
            (("plan", dict(rs_planner=True)), ("off", dict(rs_planner=False)), ("default", {}))}
    for env in envs.values():
        env.reset()
    rng = np.random.default_rng(5)
    env = envs["plan"]
    pool = env.scenario_manager.pool
    alone = RSPlanner(pool, "medium_car", steer_hi=0.524)
    for step in range(3):
        act = torch.as_tensor(rng.uniform([-0.5, -1.0], [0.5, 1.0], (8, 2)).astype(np.float32), device="cuda")
        outs = {k: e.step_torch(act) for k, e in envs.items()}
        torch.cuda.synchronize()
        assert "rs_plan" in outs["plan"] and "rs_plan" not in outs["off"] and "rs_plan" not in outs["default"]
        for k in outs["default"]:
            a, b, c = (outs[n][k].cpu().numpy() for n in ("default", "off", "plan"))
            assert a.tobytes() == b.tobytes() == c.tobytes(), (step, k)
        got = {k: v.cpu().numpy().copy() for k, v in outs["plan"]["rs_plan"].items()}
        again = alone.plan(outs["plan"]["lidar"])
        torch.cuda.synchronize()
        for k, v in again.items():
            assert v.cpu().numpy().tobytes() == got[k].tobytes(), (step, k)
        o = outs["plan"]
        ego = np.stack([o[k].cpu().numpy() for k in ("x", "y", "heading")], 1)
        target, heading = env._targets()
        scan = o["lidar"].cpu().numpy()
        plans = [R.plan_with_margin(S.PARAMS, S.LIDAR_RANGE, ego[e], target[e], heading[e], scan[e]) for e in range(8)]
        left_out = _compare(got, plans, S.PARAMS.radius)
        print(step, [p.status for p, _ in plans], "left out", left_out)
        assert left_out <= 0.02 * 8
        assert sum(p.status in (R.FOUND, R.NONE_FREE) for p, _ in plans) >= 2   # (the sweep runs: not all FAR)
    for e in envs.values():
        e.close()


def test_rows_that_cannot_plan_and_call_order(torch):
    from tactics2d_amd import _ffi, layout as L
    n, n_beams = 5, 120
    case = {k: (v[:n] if isinstance(v, np.ndarray) else v) for k, v in S.planner_case(65, n_beams).items()}
    active = np.ones(n, np.uint8)
    active[1] = 0
    pool = _pool(case, n_beams, active)
    with pytest.raises(_ffi.T2DError) as ei:   # before t2d_rs_config
        pool.rs_plan()
    assert ei.value.code == _ffi.ERR_STATE
    clean = [R.plan(case["params"], S.LIDAR_RANGE, case["ego"][e], case["target"][e], case["target_heading"][e],
                    np.full(n_beams, np.inf, np.float32)) for e in range(n)]
    assert [p.status for p in clean] == [R.FOUND, R.FOUND, R.FOUND, R.FAR, R.FOUND]   # (what the seeded scenes give in the open)
    scan = np.full((n, n_beams), np.inf, np.float32)
    scan[2, 7] = np.nan   # a NaN in the scan of an env that would plan
    got = _plan(torch, pool, scan)
    assert got["status"].tolist() == [R.FOUND, R.NO_TARGET, R.UNCHECKED, R.FAR, R.FOUND]
    assert got["slot"][2] == -1 and got["n_seg"][2] == 0 and got["n_visited"][2] == 0 and np.isnan(got["length"][2])
    assert abs(got["shortest"][2] - clean[2].shortest) <= TOL
    for e in (0, 4):   # the neighbours plan as without it
        assert got["slot"][e] == clean[e].slot and abs(got["length"][e] - clean[e].length) <= TOL
    assert L.RS_NO_TARGET == R.NO_TARGET and L.RS_UNCHECKED == R.UNCHECKED and L.RS_FOUND == R.FOUND
    scan[2, 7] = np.inf
    scan[2, 9] = -np.inf   # not finite, not a NaN: clipped like any value (np.clip), the env plans
    assert _plan(torch, pool, scan)["status"][2] in (R.FOUND, R.NONE_FREE)
    # the pool's own records and its own scan buffer (all zero after lidar_config: every beam at the vehicle base)
    pool.profile_enable(True)
    pool.rs_plan()
    pool.sync()
    own = pool.rs_plan_views()["status"].cpu().numpy()
    assert own[1] == R.NO_TARGET and own.shape == (n,)
    ms, launches = pool.profile_read(L.PROFILE_RS_PLAN)
    assert launches == 1 and ms > 0
    pool.profile_enable(False)
    pool.lidar_config(60, S.LIDAR_RANGE)   # the beam count changed behind the planner's back
    with pytest.raises(_ffi.T2DError) as ei:
        pool.rs_plan()
    assert ei.value.code == _ffi.ERR_STATE
    # beams that are not at k * 2 pi / n: the planner's chain would stand at the wrong angles
    th = np.linspace(0, 2 * np.pi, 60, endpoint=False) + 0.01
    bs, bc = np.ascontiguousarray(np.sin(th)), np.ascontiguousarray(np.cos(th))
    _ffi.check(pool._lib.t2d_lidar_config(pool._h, 60, S.LIDAR_RANGE, 0, bs.ctypes.data, bc.ctypes.data), pool._h, pool._lib)
    with pytest.raises(_ffi.T2DError) as ei:
        pool.rs_config(**{k: getattr(pool.rs_params, k) for k, _ in _ffi.RSParams._fields_})
    assert ei.value.code == _ffi.ERR_STATE
    pool.lidar_config(60, S.LIDAR_RANGE)
    pool.rs_config(**{k: getattr(pool.rs_params, k) for k, _ in _ffi.RSParams._fields_})
    pool.rs_plan()
    pool.sync()
    pool.close()
    # radius <= 0: refused without a launch
    lib = _ffi.lib()
    buf = torch.zeros(64, dtype=torch.float64, device="cuda")
    p = buf.data_ptr()
    assert lib.t2d_rs_paths(0, 1, 0.0, p, p, p, p, p, p, None) == _ffi.ERR_INVALID
    assert lib.t2d_rs_paths(0, 1, -2.0, p, p, p, p, p, p, None) == _ffi.ERR_INVALID
    torch.cuda.synchronize()
    assert (buf == 0).all()
