"""The Reeds-Shepp path follower on the device: t2d_rs_follow teacher-forced through the fixture made by executing the tutorial's
cells (tests/golden/rs_follow.npz), in closed loop on the device's own physics against the specification
(tests/rs_follow_ref.py), inside VecParkingEnv, and at its edges."""
import numpy as np
import pytest

import rs_follow_cases as S
import rs_follow_ref as F

pytestmark = pytest.mark.gpu
TOL = 1e-9   # the project's Reeds-Shepp tolerance (tests/test_rs.py); the follower adds O(1) gains on fp64 metres


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _pool(n, state=None, active=None):
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(n, 1)
    ego = vehicle_model("medium_car", "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0), steer_range=(-0.524, 0.524))
    pool.set_param_table(ego.param_row(L.SHAPE_OBB, *VEHICLE_TEMPLATE["medium_car"][:2])[None])
    pool.set_status_config()
    pool.set_target_areas(np.tile(np.float64([30, 30, 32, 30, 32, 35, 30, 35]), (n, 1)))
    pool.set_target_headings(np.zeros(n))
    st = np.zeros((n, 4), np.float32) if state is None else state
    pool.reset(st[:, 0], st[:, 1], st[:, 2], st[:, 3], np.zeros(n, np.int32), active)
    pool.lidar_config(24, 20.0)
    return pool


def _follower(pool, **overrides):
    from tactics2d_amd.planner import RSFollower, RSPlanner
    return RSFollower(pool, RSPlanner(pool, "medium_car", steer_hi=0.524), **overrides)


def _gain_overrides(g, gains):
    t = g["gain_table"][gains]
    return dict(zip(("kp_v", "ki_v", "kd_v", "kp_a", "ki_a", "kd_a", "kp_s", "ki_s", "kd_s"), (float(v) for v in t)))


def _plan_records(torch, g, rows):
    """t2d_rs_plan_record [n] as a float64 tensor: status FOUND with the plan table's row for rows >= 0, NO_TARGET otherwise"""
    from tactics2d_amd import layout as L
    rec = np.zeros((len(rows), L.RS_RECORD_BYTES // 8))
    i32 = rec.view(np.int32).reshape(len(rows), -1)
    for e, k in enumerate(rows):
        if k >= 0:
            i32[e, 0], i32[e, 2] = L.RS_FOUND, g["plan_n"][k]
            i32[e, 4:9] = g["plan_steer"][k]
            rec[e, 5:10] = g["plan_distance"][k]
    t = torch.as_tensor(rec, device="cuda")
    return dict(status=t)   # (RSFollower.follow reads the records at the first field's address)


def _set_state(torch, pool, state, status=None):
    from tactics2d_amd import layout as L
    for col, f in enumerate((L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED)):
        pool.upload(f, np.ascontiguousarray(state[:, col]))
    if status is not None:
        pool.upload(L.F_STATUS, status)


def _teacher_forced(torch, g, seqs, n_env, n_steps=None):
    """env e replays sequence seqs[e % len(seqs)]; returns the largest action deviation"""
    which = [seqs[e % len(seqs)] for e in range(n_env)]
    length = np.array([g["off"][q + 1] - g["off"][q] for q in which])
    steps = int(length.max()) if n_steps is None else n_steps
    pool = _pool(n_env)
    fol = _follower(pool, **_gain_overrides(g, int(g["gains"][which[0]])))
    policy = torch.as_tensor(np.random.default_rng(1).uniform(-1, 1, (n_env, 2)).astype(np.float32), device="cuda")
    worst, ulps = 0.0, 0
    for t in range(steps):
        k = np.array([g["off"][q] + min(t, n - 1) for q, n in zip(which, length)])
        over = t >= length                      # the sequence is over: the last state again, the episode ended, no plan
        status = np.zeros((n_env, 4), np.uint8)
        status[:, 2] = np.where(over, 1, g["ended"][k])
        _set_state(torch, pool, g["state"][k], status)
        out = fol.follow(policy, plan=_plan_records(torch, g, np.where(over, -1, g["plan"][k])))
        torch.cuda.synchronize()
        rows = out["action_rows"].cpu().numpy()
        ex, seg, ev, act = (out[n].cpu().numpy() for n in ("executing", "segment", "events", "action"))
        live = ~over
        assert np.array_equal(ex[live], g["left"][k][live]) and np.array_equal(seg[live], g["head"][k][live]), t
        assert np.array_equal(ev[live], g["events"][k][live].astype(np.int32)), (t, ev[live], g["events"][k][live])
        acted = live & ~np.isnan(g["action"][k, 0])
        assert not np.isnan(act[acted]).any() and np.isnan(act[~acted]).all(), t
        if acted.any():
            worst = max(worst, np.abs(act[acted] - g["action"][k][acted]).max())
            want = g["row"][k][acted]
            d = np.abs(rows[acted].view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
            same_sign = np.signbit(rows[acted]) == np.signbit(want)
            ulps = max(ulps, int(d[same_sign].max(initial=0)))
            assert ((rows[acted] == want) | same_sign).all(), t
        assert rows[~acted].tobytes() == policy.cpu().numpy()[~acted].tobytes(), t   # the policy's row, bit for bit
        assert (ex[over] == 0).all() and (ev[over] == F.EV_RESET).all()
    pool.close()
    print("n_env", n_env, "steps", steps, "largest action deviation", worst, "largest row deviation in fp32 ulps", ulps)
    assert worst <= TOL and ulps <= 1
    return worst


@pytest.mark.parametrize("n_env,n_steps", [(24, None), (1, 40), (63, 40), (65, 40)])
def test_teacher_forced_closed_loops(torch, n_env, n_steps):
    _teacher_forced(torch, S.fixture(), list(range(S.N_LOOPS)), n_env, n_steps)


@pytest.mark.parametrize("gains", [0, 1])
def test_teacher_forced_synthetic_sequences(torch, gains):
    g = S.fixture()
    seqs = [q for q in range(S.N_LOOPS, len(g["off"]) - 1) if g["gains"][q] == gains]
    _teacher_forced(torch, g, seqs, len(seqs))


def test_closed_loop_on_the_device_physics(torch):
    from tactics2d_amd import layout as L
    g = S.fixture()
    n = S.N_LOOPS
    first = g["off"][:n]
    pool = _pool(n, g["state"][first])
    fol = _follower(pool)
    refs = [F.Follower(S.params(g)) for _ in range(n)]
    cap = 2 * (g["off"][1:n + 1] - first)
    rows = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    pool.bind_actions(rows.data_ptr() + 4, rows.data_ptr(), stride=2)
    done_at, final, worst = np.full(n, -1), np.zeros((n, 3)), 0.0
    for t in range(int(cap.max())):
        state = np.stack([pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED)], 1)
        out = fol.follow(None, plan=_plan_records(torch, g, g["plan"][first] if t == 0 else np.full(n, -1)), out=rows)
        torch.cuda.synchronize()
        ex, seg, ev, act = (out[k].cpu().numpy() for k in ("executing", "segment", "events", "action"))
        stepped = rows.cpu().numpy()
        for e in range(n):
            if done_at[e] >= 0:
                assert ex[e] == 0 and ev[e] == 0 and (stepped[e] == 0).all()
                continue
            r = refs[e].call(state[e], False, True, S.plan_of(g, int(g["plan"][first[e]])) if t == 0 else None)
            assert F.margin(r) >= 1e-9, (t, e, "a knife edge of the device's own trajectory")
            assert (ex[e], seg[e], ev[e]) == (r.executing, r.segment, r.events), (t, e, r)
            worst = max(worst, np.abs(act[e] - np.array(r.action)).max())
            if r.events & F.EV_FINISHED:
                done_at[e] = t
        pool.step(100)
        pool.sync()
        for e in np.nonzero(done_at == t)[0]:
            final[e] = [pool.download(f)[e] for f in (L.F_X, L.F_Y, L.F_HEADING)]
        if (done_at >= 0).all():
            break
        assert (t < cap)[done_at < 0].all(), ("not finished within twice the fixture's steps", np.nonzero(done_at < 0)[0])
    assert (done_at >= 0).all() and worst <= TOL
    dr = float(g["dr"].reshape(-1)[0])
    err = np.hypot(final[:, 0] - dr * np.cos(final[:, 2]) - g["end_pose"][:, 0], final[:, 1] - dr * np.sin(final[:, 2]) - g["end_pose"][:, 1])
    fx = g["state"][g["off"][1:n + 1] - 1]
    print("largest action deviation", worst, "rear axle to the path's end", err.max(), "finishing step - fixture's",
          np.abs(done_at + 1 - (g["off"][1:n + 1] - first)).max(), "final pose - fixture's", np.abs(final[:, :2] - fx[:, :2]).max())
    assert err.max() <= 0.15   # popped within 0.1 m of the target, one further step at <= 0.5 m/s moves <= 0.05 m
    pool.close()


def test_in_the_env(torch):
    from tactics2d_amd.envs import VecParkingEnv
    from tactics2d_amd.planner import rs_params
    with pytest.raises(ValueError):
        VecParkingEnv(8, rs_follow=True)
    kw = dict(seed=3, lidar_beams=360, rs_planner=True, auto_reset=True, max_step=25)
    env, twin = VecParkingEnv(8, rs_follow=True, **kw), VecParkingEnv(8, rs_follow=False, **kw)
    env.reset()
    twin.reset()
    p = rs_params("medium_car", steer_hi=0.524)
    refs = [F.Follower(F.Params(p["radius"], p["center_shift"])) for _ in range(8)]
    rng = np.random.default_rng(5)
    o0 = env.planner._views
    torch.cuda.synchronize()
    plan = {k: v.cpu().numpy().copy() for k, v in o0.items()}
    state = np.stack([env.scenario_manager.pool.download(f) for f in range(4)], 1)   # F_X, F_Y, F_HEADING, F_SPEED
    status = np.zeros((8, 4), np.uint8)
    executing, reset_then_adopted, worst = set(), 0, 0.0
    for step in range(60):
        act = torch.as_tensor(rng.uniform([-0.5, -1.0], [0.5, 1.0], (8, 2)).astype(np.float32), device="cuda")
        keep = act.clone()
        a = env.step_torch(act)
        b = twin.step_torch(a["action"].clone())
        torch.cuda.synchronize()
        assert torch.equal(act, keep)
        for k in ("x", "y", "heading", "speed", "vx", "vy", "reward", "status", "iou", "lidar"):
            assert a[k].cpu().numpy().tobytes() == b[k].cpu().numpy().tobytes(), (step, k)
        for k in a["rs_plan"]:
            assert a["rs_plan"][k].cpu().numpy().tobytes() == b["rs_plan"][k].cpu().numpy().tobytes(), (step, k)
        rec = {k: v.cpu().numpy() for k, v in a["rs_follow"].items()}
        rows = a["action"].cpu().numpy()
        for e in range(8):
            found = plan["status"][e] == 2
            pl = (plan["steer"][e, :plan["n_seg"][e]], plan["distance"][e, :plan["n_seg"][e]]) if found else None
            r = refs[e].call(state[e], bool(status[e, 2] | status[e, 3]), True, pl, keep[e].cpu().numpy())
            if F.margin(r) < 1e-9:
                pytest.fail("a knife edge in the env's own trajectory: change the seed")
            assert (rec["executing"][e], rec["segment"][e], rec["events"][e]) == (r.executing, r.segment, r.events), (step, e, r)
            if np.isnan(r.action[0]):
                assert rows[e].tobytes() == r.row.tobytes()
            else:
                worst = max(worst, np.abs(rec["action"][e] - np.array(r.action)).max())
                assert np.abs(rows[e] - r.row).max() <= np.spacing(np.abs(r.row).max())
                executing.add(e)
            reset_then_adopted += (r.events & (F.EV_RESET | F.EV_ADOPTED)) == (F.EV_RESET | F.EV_ADOPTED)
        plan = {k: v.cpu().numpy().copy() for k, v in a["rs_plan"].items()}
        state = np.stack([a[k].cpu().numpy() for k in ("x", "y", "heading", "speed")], 1)
        status = a["status"].cpu().numpy().copy()
    print("executing envs", sorted(executing), "reset then adopted", reset_then_adopted, "largest action deviation", worst)
    assert len(executing) >= 2 and reset_then_adopted >= 1 and worst <= TOL
    env.close()
    twin.close()


def test_rows_and_call_order(torch):
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.planner import RSPlanner, rs_follow_params
    g = S.fixture()
    n = 6
    first = g["off"][:n]
    active = np.ones(n, np.uint8)
    active[1] = 0
    pool = _pool(n, g["state"][first].copy(), active)
    rows = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    with pytest.raises(_ffi.T2DError) as ei:   # before t2d_rs_config
        pool.rs_follow_config(**F.Params()._asdict())
    assert ei.value.code == _ffi.ERR_STATE
    planner = RSPlanner(pool, "medium_car", steer_hi=0.524)
    with pytest.raises(_ffi.T2DError) as ei:   # before t2d_rs_follow_config
        pool.rs_follow(None, rows.data_ptr())
    assert ei.value.code == _ffi.ERR_STATE
    good = rs_follow_params(planner.params)
    for k, v in (("radius", 0.0), ("max_speed", -1.0), ("reach_radius", 0.0), ("kp_v", float("nan")), ("dr", float("inf")),
                 ("accel_bound", 0.0)):
        with pytest.raises(_ffi.T2DError) as ei:
            pool.rs_follow_config(**dict(good, **{k: v}))
        assert ei.value.code == _ffi.ERR_INVALID, k
    from tactics2d_amd.planner import RSFollower
    fol = RSFollower(pool, planner)
    st = g["state"][first].copy()
    st[2, 0] = np.nan
    _set_state(torch, pool, st)
    policy = torch.as_tensor(np.random.default_rng(2).uniform(-1, 1, (n, 2)).astype(np.float32), device="cuda")
    plan = _plan_records(torch, g, g["plan"][first])
    pool.profile_enable(True)
    out = fol.follow(policy, plan=plan)
    pool.sync()
    ms, launches = pool.profile_read(L.PROFILE_RS_FOLLOW)
    assert launches == 1 and ms > 0
    pool.profile_enable(False)
    ev, ex = out["events"].cpu().numpy(), out["executing"].cpu().numpy()
    got = out["action_rows"].cpu().numpy()
    assert ev.tolist() == [1, 0, 32, 1, 1, 1] and ex[1] == 0 and ex[2] == 0 and (ex[[0, 3, 4, 5]] > 0).all()
    assert got[[1, 2]].tobytes() == policy.cpu().numpy()[[1, 2]].tobytes() and np.isnan(out["action"].cpu().numpy()[[1, 2]]).all()
    k = first[[0, 3, 4, 5]]
    assert np.abs(out["action"].cpu().numpy()[[0, 3, 4, 5]] - g["action"][k]).max() <= TOL   # the neighbours are unaffected
    assert np.abs(got[[0, 3, 4, 5]] - g["row"][k]).max() <= np.spacing(np.float32(2.0))
    # in place: the same rows
    _set_state(torch, pool, g["state"][first])
    fol.reset()
    a = fol.follow(policy, plan=plan)["action_rows"].cpu().numpy().copy()
    fol.reset()
    inplace = policy.clone()
    b = fol.follow(inplace, plan=plan, out=inplace)["action_rows"].cpu().numpy()
    assert a.tobytes() == b.tobytes()
    # a masked reset clears exactly those envs
    mask = torch.as_tensor(np.uint8([1, 0, 0, 1, 0, 0]), device="cuda")
    fol.reset(mask)
    out = fol.follow(policy, plan=_plan_records(torch, g, np.full(n, -1)))
    torch.cuda.synchronize()
    assert (out["executing"].cpu().numpy() > 0).tolist() == [False, False, True, False, True, True]
    pool.close()
    fresh = __import__("tactics2d_amd.pool", fromlist=["ParticipantPool"]).ParticipantPool(2, 1)   # before t2d_reset
    with pytest.raises(_ffi.T2DError) as ei:
        fresh.rs_follow(None, rows.data_ptr())
    assert ei.value.code == _ffi.ERR_STATE
    fresh.close()
