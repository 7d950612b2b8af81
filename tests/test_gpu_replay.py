"""Replayed participants on the device (model layout.MODEL_REPLAY, t2d_replay_bind / t2d_replay_apply, replay_kernel in
tactics2d_amd/csrc/t2d_history.hip): the reference's `p.is_active(frame)` / `p.get_state(frame)` loop
(participant/element/participant_base.py:166-203, traffic/scenario_manager.py:83-94) inside the device step.

The feature copies fp32 words: every state comparison here is bit equality."""
import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

STATE_FIELDS = ("F_X", "F_Y", "F_HEADING", "F_SPEED", "F_VX", "F_VY")
STEP_FIELDS = STATE_FIELDS + ("F_FLAGS", "F_ENV_FLAGS", "F_STATUS", "F_REWARD", "F_CNT_STEP", "F_FRAME_MS")


def _fields(pool, names=STEP_FIELDS):
    from tactics2d_amd import layout as L
    return {n: pool.download(getattr(L, n)) for n in names}


def _same(a, b, what):
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), (what, k, int((a[k].view(np.uint8) != b[k].view(np.uint8)).sum()))


def _states(pool):
    """float32 [N, 6] of the pool's six state columns"""
    from tactics2d_amd import layout as L
    return np.stack([pool.download(getattr(L, n)) for n in STATE_FIELDS], 1)


def _active(pool):
    from tactics2d_amd import layout as L
    return ((pool.download(L.F_IDS) >> 16) & 0xff).astype(np.uint8)


def _compact_scene(n_env, A, seed):
    """scenarios.mixed with its 25 participant types folded onto eight (two kinematic and two dynamic cars, a cyclist, a
    moped, two pedestrians): the three integrated model kinds, boxes and circles, in a table that leaves room for as many
    replayed rows.  Returns (scene, rows, type_id)."""
    from tactics2d_amd import scenarios as S
    sc = S.mixed(n_env, A, seed=seed)
    names = sc.type_names
    keep = ["small_car:kin", "large_car:kin", "medium_car:dyn", "luxury_car:dyn", "cyclist", "moped", "adult_male",
            "children_ten_year_old"]
    fold = {}
    for i, n in enumerate(names):
        if n.endswith(":kin"):
            fold[i] = keep.index(keep[i % 2])
        elif n.endswith(":dyn"):
            fold[i] = keep.index(keep[2 + i % 2])
        elif n in ("cyclist", "moped", "motorcycle"):
            fold[i] = keep.index(keep[4 + i % 2])
        else:
            fold[i] = keep.index(keep[6 + i % 2])
    rows = np.stack([sc.rows[names.index(n)] for n in keep])
    tid = np.array([fold[int(t)] for t in sc.type_id], np.uint8)
    return sc, rows, tid


def _replayed_copy(rows):
    """one replayed row per row: its shape, length and width, model 5"""
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import replayed_shape_row
    return np.stack([replayed_shape_row(r[L.P_SHAPE], r[L.P_LENGTH], r[L.P_WIDTH]) for r in rows])


def _load(pool, sc, rows, tid, active=None, status=None):
    pool.set_param_table(rows)
    pool.set_static_geometry(sc.static, sc.boundary, sc.boundary_valid)
    pool.set_lane_geometry(sc.lanes)
    pool.set_status_config(**(sc.status if status is None else status))
    pool.reset(sc.x, sc.y, sc.heading, sc.speed, tid, sc.active if active is None else active)


def _record_run(sc, rows, tid, n_steps, interval, seed, status=None):
    """pool A: every participant integrated; returns (pool, its DeviceTrajectory with slot k = the state at k * interval,
    the action sets, the fields after every step)"""
    from tactics2d_amd.history import DeviceTrajectory
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc.n_env, sc.A)
    _load(pool, sc, rows, tid, status=status)
    traj = DeviceTrajectory(pool, 0, capacity=n_steps + 1)
    traj.record(pool, 0)
    rng = np.random.default_rng(seed)
    acts, after = [], []
    for k in range(n_steps):
        acts.append(sc.sample_actions(rng))
        pool.set_actions(*acts[-1])
        pool.step(interval)
        traj.record(pool, (k + 1) * interval)
        after.append(_fields(pool))
    return pool, traj, acts, after


# ------------------------------------------------------------------------------------------------------------------ 4
def test_a_replay_of_a_recording_reproduces_the_recording():
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    n_env, A, n_steps, interval = 64, 8, 40, 100
    sc, rows, tid = _compact_scene(n_env, A, seed=11)
    assert sc.static[0][-1] > 0 and sc.lanes[0][-1] > 0 and sc.status["check_dynamic"] == 1
    models = set(rows[tid, 0].astype(int))
    assert models == {0, 1, 2}, models
    a, traj, acts, after = _record_run(sc, rows, tid, n_steps, interval, seed=5)
    b = ParticipantPool(n_env, A)
    try:
        assert a.step_form(1) != "unfused"
        ego = (np.arange(n_env * A) % A) == 0
        tid_b = np.where(ego, tid, tid + len(rows)).astype(np.uint8)
        _load(b, sc, np.concatenate([rows, _replayed_copy(rows)]), tid_b)
        b.replay_bind(ReplaySource.from_device(traj, 0, interval))
        assert b.step_form(1) == "unfused" and b.step_form(8) == "unfused"
        b.replay_apply()
        assert _states(b).tobytes() == np.ascontiguousarray(traj._buf.read(0).T).tobytes()   # (stamp 0: where the recording starts)
        for k in range(n_steps):
            b.set_actions(*acts[k])
            b.step(interval)
            _same(_fields(b), after[k], f"step {k}")
        flagged = int((after[-1]["F_FLAGS"] != 0).sum())
        assert flagged > 0, "the scene raises no event at all: the comparison of the flags would be empty"
        # the replayed participants are still replayed ones: model byte 5, active
        from tactics2d_amd import layout as L
        ids = b.download(L.F_IDS)
        assert ((ids[~ego] & 0xff) == L.MODEL_REPLAY).all() and (((ids >> 16) & 0xff) == 1).all()
        b.replay_unbind()
    finally:
        b.close()
        a.close()


# ------------------------------------------------------------------------------------------------------------------ 5
W_FULL, W_LATE, W_EARLY, W_ONE, W_NEVER = range(5)


def _window_source(rng, n_src_env, A, n_slots, extent=(40.0, 24.0)):
    """random walks on the grid + staggered windows of every kind; returns (states [n_slots, n_src_env, A, 6], first, last, kind)"""
    n = n_src_env * A
    st = np.zeros((n_slots, n, 6), np.float32)
    pos = np.stack([rng.uniform(-extent[0] / 2, extent[0] / 2, n), rng.uniform(-extent[1] / 2, extent[1] / 2, n)], 1)
    head = rng.uniform(0, 2 * np.pi, n)
    speed = rng.uniform(0, 12, n)
    for k in range(n_slots):
        st[k, :, 0], st[k, :, 1], st[k, :, 2], st[k, :, 3] = pos[:, 0], pos[:, 1], head, speed
        st[k, :, 4], st[k, :, 5] = speed * np.cos(head), speed * np.sin(head)
        pos = pos + 0.04 * speed[:, None] * np.stack([np.cos(head), np.sin(head)], 1)
        head = np.mod(head + rng.normal(0, 0.03, n), 2 * np.pi)
    kind = rng.integers(0, 5, n)
    kind[:5] = np.arange(5)
    first, last = np.zeros(n, np.int32), np.full(n, n_slots - 1, np.int32)
    late, early, one, never = kind == W_LATE, kind == W_EARLY, kind == W_ONE, kind == W_NEVER
    first[late] = rng.integers(2, 25, late.sum())
    last[early] = rng.integers(2, 25, early.sum())
    first[one] = last[one] = rng.integers(1, 30, one.sum())
    first[never], last[never] = 1, 0
    return st.reshape(n_slots, n_src_env, A, 6), first, last, kind


@pytest.mark.parametrize("mult", [1, 2])
def test_windows_decide_who_is_there_and_the_events_see_it(oracle, mult):
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    rng = np.random.default_rng(77 + mult)
    n_env, A, period, n_slots, n_steps = 32, 8, 40, 64, 30
    interval = mult * period
    sc = H.polygon_scene(rng, n_env, A)
    rows = sc["rows"].copy()
    rows[:, L.P_MODEL] = L.MODEL_REPLAY
    st, first, last, kind = _window_source(rng, n_env, A, n_slots)
    counts = np.bincount(kind, minlength=5)
    assert (counts >= 5).all(), counts
    pool = ParticipantPool(n_env, A)
    try:
        src = ReplaySource.from_arrays(pool, st, first, last, 0, period)
        pool.set_param_table(rows)
        pool.set_static_geometry(sc["static"], sc["boundary"], sc["boundary_valid"])
        pool.set_lane_geometry(sc["lanes"])
        pool.set_status_config(max_step=100000, check_dynamic=1, check_off_lane=1)
        # everybody starts inactive at a place of its own: what a participant holds before its window opens
        park = np.stack([sc["x"], sc["y"], sc["heading"], np.zeros(n_env * A, np.float32)], 1).astype(np.float32)
        pool.reset(park[:, 0], park[:, 1], park[:, 2], park[:, 3], sc["type_id"], np.zeros(n_env * A, np.uint8))
        pool.replay_bind(src)
        mirror = _states(pool)
        seen = dict(appear=0, leave=0, absent_all=0, one=0, collisions=0, absent_near=0)
        was = np.zeros(n_env * A, bool)
        flat = st.reshape(n_slots, -1, 6)
        for k in range(n_steps + 1):
            if k == 0:
                pool.replay_apply()
                pool.collide()
            else:
                pool.step(interval)
            slot = k * interval // period
            want_act = (slot >= first) & (slot <= last) & (slot < n_slots)
            got_act = _active(pool).astype(bool)
            assert (got_act == want_act).all(), (k, np.nonzero(got_act != want_act)[0][:8])
            mirror[want_act] = flat[min(slot, n_slots - 1)][want_act]
            got = _states(pool)
            assert got.tobytes() == mirror.tobytes(), (k, np.nonzero((got != mirror).any(1))[0][:8])
            flags, env_flags = pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS)
            wf, we = oracle.collide(rows, n_env, A, got[:, 0], got[:, 1], got[:, 2], sc["type_id"], want_act.astype(np.uint8),
                                    sc["static"], sc["boundary"], sc["boundary_valid"], sc["lanes"])
            assert (flags == wf).all() and (env_flags == we).all(), k
            # ... and nobody collides with an absent participant: the oracle with everybody present finds more
            wf_all, _ = oracle.collide(rows, n_env, A, got[:, 0], got[:, 1], got[:, 2], sc["type_id"], np.ones(n_env * A, np.uint8),
                                       sc["static"], sc["boundary"], sc["boundary_valid"], sc["lanes"])
            seen["absent_near"] += int(((wf_all & L.FLAG_COLLISION_DYNAMIC) != 0).sum() - ((wf & L.FLAG_COLLISION_DYNAMIC) != 0).sum())
            seen["collisions"] += int(((flags & L.FLAG_COLLISION_DYNAMIC) != 0).sum())
            seen["appear"] += int((want_act & ~was).sum())
            seen["leave"] += int((~want_act & was).sum())
            seen["one"] += int((want_act & (kind == W_ONE)).sum())
            was = want_act
        assert not _active(pool)[kind == W_NEVER].any()
        # (with interval = 2 x period a one-slot window on an odd slot is stepped over: it must never show)
        one_hit = ((first % mult == 0) & (first // mult <= n_steps) & (kind == W_ONE)).sum()
        assert seen["one"] == one_hit and (mult == 2 or one_hit == counts[W_ONE])
        assert seen["appear"] >= 20 and seen["leave"] >= 20 and seen["collisions"] > 0 and seen["absent_near"] > 0, seen
        frame = pool.download(L.F_FRAME_MS)
        assert (frame == n_steps * interval).all()
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------------------------ 6
def test_many_envs_share_four_logs_at_their_own_offsets():
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    rng = np.random.default_rng(9)
    n_env, n_src, A, period, n_slots = 256, 4, 8, 40, 48
    st, first, last, _ = _window_source(rng, n_src, A, n_slots)
    rows = _replayed_copy(H.shape_rows(True))
    tid = rng.integers(0, len(rows), n_env * A).astype(np.uint8)
    src_env = rng.integers(0, n_src, n_env).astype(np.int32)
    src_env[:4] = np.arange(4)
    offset = (rng.integers(0, 12, n_env) * period).astype(np.int32)
    pool = ParticipantPool(n_env, A)
    try:
        src = ReplaySource.from_arrays(pool, st, first, last, 0, period)
        assert src.device_buffer().pool is not pool and src.device_buffer().pool.n_env == n_src   # a library pool of its own
        pool.set_param_table(rows)
        pool.set_status_config(max_step=100000, check_dynamic=1)
        z = np.zeros(n_env * A, np.float32)
        pool.reset(z, z, z, z, tid, np.zeros(n_env * A, np.uint8))
        pool.replay_bind(src, src_env, offset)
        flat = st.reshape(n_slots, n_src, A, 6)
        mirror = _states(pool).reshape(n_env, A, 6)
        fw, lw = first.reshape(n_src, A)[src_env], last.reshape(n_src, A)[src_env]
        for k in range(1, 31):
            pool.step(period)
            slot = (k * period + offset) // period
            want = (slot[:, None] >= fw) & (slot[:, None] <= lw) & (slot[:, None] < n_slots)
            rows_now = flat[np.minimum(slot, n_slots - 1), src_env]
            mirror[want] = rows_now[want]
            assert (_active(pool).reshape(n_env, A).astype(bool) == want).all(), k
            assert _states(pool).tobytes() == mirror.tobytes(), k
        assert len(set(zip(src_env.tolist(), offset.tolist()))) > 30
        # the manager's frame query answers by the same windows, per env, without a device call
        from tactics2d_amd.traffic import BatchedScenarioManager
        m = BatchedScenarioManager.__new__(BatchedScenarioManager)
        m.pool, m.n_env, m.max_agents = pool, n_env, A
        got = m.get_active_participants(frame=30 * period)
        assert got == [np.nonzero(w)[0].tolist() for w in want]
        assert m.get_active_participants() == got   # (frame None: the ids on the device, which the last step wrote)
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------------------------ 7
def test_auto_reset_puts_the_replayed_participants_back_at_the_snapshot():
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    n_env, A, interval, max_step, n_steps = 64, 8, 100, 20, 50
    sc, rows, tid = _compact_scene(n_env, A, seed=21)
    status = dict(sc.status, max_step=max_step)
    a, traj, _, _ = _record_run(sc, rows, tid, max_step + 2, interval, seed=6, status=status)
    b = ParticipantPool(n_env, A)
    try:
        ego = (np.arange(n_env * A) % A) == 0
        tid_b = np.where(ego, tid, tid + len(rows)).astype(np.uint8)
        _load(b, sc, np.concatenate([rows, _replayed_copy(rows)]), tid_b, status=status)
        b.replay_bind(ReplaySource.from_device(traj, 0, interval))
        b.replay_apply()
        b.snapshot()
        b.set_auto_reset(True)
        snap_state, snap_ids = _states(b), b.download(L.F_IDS)
        a0 = np.where(ego, 0.5, 0.0).astype(np.float32)
        b.set_actions(a0, np.zeros_like(a0))
        first_ep = [dict() for _ in range(n_env)]   # per env: steps into the episode -> the env's state block, first episode
        pos, resets, compared = np.zeros(n_env, int), np.zeros(n_env, int), 0
        snap = snap_state.reshape(n_env, A, 6)
        for k in range(n_steps):
            b.step(interval)
            st, cnt, status_now = _states(b).reshape(n_env, A, 6), b.download(L.F_CNT_STEP), b.download(L.F_STATUS)
            ids, frame = b.download(L.F_IDS).reshape(n_env, A), b.download(L.F_FRAME_MS)
            done = (status_now[:, 2:] != 0).any(1)
            for e in range(n_env):
                if done[e]:      # the step's epilogue has put the env back at the snapshot
                    resets[e] += 1
                    pos[e] = 0
                    assert frame[e] == 0 and cnt[e] == 0, (k, e)
                    assert st[e].tobytes() == snap[e].tobytes(), (k, e)
                    assert (ids[e] == snap_ids.reshape(n_env, A)[e]).all(), (k, e)
                    continue
                pos[e] += 1
                assert frame[e] == pos[e] * interval
                if resets[e] == 0:
                    first_ep[e][pos[e]] = st[e].copy()
                elif pos[e] in first_ep[e]:
                    assert st[e].tobytes() == first_ep[e][pos[e]].tobytes(), (k, e, pos[e])
                    compared += 1
        assert (resets >= 2).all(), resets.min()
        long_first = sum(len(d) >= 5 for d in first_ep)
        assert long_first >= n_env // 2 and compared >= 10 * long_first, (long_first, compared)
        # the replayed participants really moved inside an episode (the comparison is not of a still picture)
        e = int(np.argmax([len(d) for d in first_ep]))
        assert first_ep[e][1][1:].tobytes() != first_ep[e][2][1:].tobytes()
        b.replay_unbind()
    finally:
        b.close()
        a.close()


# ------------------------------------------------------------------------------------------------------------------ 8
def test_step_step_n_and_the_two_call_form_agree_on_a_replay_pool():
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    n_env, A, interval, n = 48, 8, 100, 12
    sc, rows, tid = _compact_scene(n_env, A, seed=31)
    a, traj, acts, _ = _record_run(sc, rows, tid, n, interval, seed=8)
    src = ReplaySource.from_device(traj, 0, interval)
    ego = (np.arange(n_env * A) % A) == 0
    tid_b = np.where(ego, tid, tid + len(rows)).astype(np.uint8)
    names = STEP_FIELDS + ("F_IDS", "F_RECORD", "F_APPLIED0", "F_APPLIED1")
    out = {}
    pools = []
    try:
        for how in ("step", "step_n", "two_calls"):
            p = ParticipantPool(n_env, A)
            pools.append(p)
            _load(p, sc, np.concatenate([rows, _replayed_copy(rows)]), tid_b)
            p.replay_bind(src)
            p.set_actions(*acts[0])
            if how == "step":
                for _ in range(n):
                    p.step(interval)
            elif how == "step_n":
                p.step_n(n, interval)
            else:
                for _ in range(n):
                    p.integrate(interval)
                    p.check_status(interval)
            assert p.step_count() == n
            out[how] = _fields(p, names)
        _same(out["step"], out["step_n"], "step_n")
        _same(out["step"], out["two_calls"], "integrate + check_status")
        # and what they agree on is the recording
        for i, f in enumerate(STATE_FIELDS):
            assert out["step"][f][~ego].tobytes() == traj._buf.read(n)[i][~ego].tobytes(), f
    finally:
        for p in pools:
            p.close()
        a.close()


# ------------------------------------------------------------------------------------------------------------------ 9
def test_the_lidar_and_idm_followers_see_replayed_participants():
    from tactics2d_amd import layout as L
    from tactics2d_amd.controller import IDMController, install
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.participant import replayed_row, vehicle_row
    from tactics2d_amd.pool import ParticipantPool
    n_env, A, period = 16, 4, 40
    rng = np.random.default_rng(3)
    # agent 0: an IDM-driven car on y = 0 heading +x; agent 1: a replayed leader ahead of it; 2: a replayed car in the next lane;
    # 3: a replayed pedestrian that shows up late
    n_slots = 12
    st = np.zeros((n_slots, n_env, A, 6), np.float32)
    gap = rng.uniform(0, 10, n_env)
    for k in range(n_slots):
        st[k, :, 1, 0] = 25.0 + gap + 0.2 * k
        st[k, :, 1, 3] = st[k, :, 1, 4] = 5.0
        st[k, :, 2, 0], st[k, :, 2, 1] = 12.0, 3.75
        st[k, :, 3, 0], st[k, :, 3, 1] = 8.0, -4.0 - 0.1 * k
    first = np.zeros((n_env, A), np.int32)
    first[:, 3] = 2
    last = np.full((n_env, A), n_slots - 1, np.int32)
    rows = np.stack([vehicle_row("medium_car"), replayed_row("medium_car"), replayed_row("adult_male")])
    plain = np.stack([vehicle_row("medium_car"), vehicle_row("medium_car"), rows[2].copy()])
    plain[2, L.P_MODEL] = L.MODEL_POINTMASS
    tid = np.tile(np.array([0, 1, 1, 2], np.uint8), n_env)
    x0 = np.tile(np.float32([0, 30, 12, 8]), n_env)
    y0 = np.tile(np.float32([0, 0, 3.75, -4]), n_env)
    z = np.zeros(n_env * A, np.float32)
    v0 = np.tile(np.float32([8, 5, 0, 0]), n_env)
    active0 = np.tile(np.array([1, 1, 1, 0], np.uint8), n_env)
    cid = np.tile(np.array([0, L.IDM_NONE, L.IDM_NONE, L.IDM_NONE], np.uint8), n_env)
    a, b = ParticipantPool(n_env, A), ParticipantPool(n_env, A)
    try:
        for p, table in ((a, rows), (b, plain)):
            p.set_param_table(table)
            p.set_status_config(max_step=100000, check_dynamic=1)
            p.reset(x0, y0, z, v0, tid, active0)
            p.lidar_config(120, 40.0, True)
            install(p, [IDMController(desired_speed=15.0, horizon=100.0)], cid)
        a.replay_bind(ReplaySource.from_arrays(a, st, first, last, 0, period))
        for k in range(4):
            a.step(period)
        assert _active(a).reshape(n_env, A)[:, 3].all()       # the pedestrian has appeared (slot 4 >= 2)
        # an ordinary pool in the same state: columns and ids uploaded
        for f in STATE_FIELDS:
            b.upload(getattr(L, f), a.download(getattr(L, f)))
        ids = a.download(L.F_IDS)
        b.upload(L.F_IDS, ((ids & ~np.uint32(0xff)) | plain[(ids >> 8) & 0xff, L.P_MODEL].astype(np.uint32)).astype(np.uint32))
        a.lidar_scan_all()
        b.lidar_scan_all()
        la, lb = a.lidar_all(), b.lidar_all()
        assert la.tobytes() == lb.tobytes() and np.isfinite(la[:, 0]).any() and np.isfinite(la[:, 1]).any()
        a.idm_actions()
        b.idm_actions()
        lead_a, lead_b = a.download(L.F_LEADER).reshape(n_env, A), b.download(L.F_LEADER).reshape(n_env, A)
        assert (lead_a[:, 0] == 1).all() and (lead_a == lead_b).all()
        acc_a, acc_b = a.download(L.F_ACT0).reshape(n_env, A)[:, 0], b.download(L.F_ACT0).reshape(n_env, A)[:, 0]
        assert acc_a.tobytes() == acc_b.tobytes() and len(set(acc_a.tolist())) > 1
        # and inside the step: the follower's next state is what the ordinary pool computes when its other participants are held
        # where the recording puts them
        a.step(period)
        nxt = _states(a).reshape(n_env, A, 6)
        assert (nxt[:, 1, 0] == st[5, :, 1, 0]).all()
        b.step(period)
        assert _states(b).reshape(n_env, A, 6)[:, 0].tobytes() == nxt[:, 0].tobytes()
    finally:
        a.close()
        b.close()


# ----------------------------------------------------------------------------------------------------------------- 10
@pytest.mark.parametrize("n_env,A,n_src", [(4096, 64, 4096), (50, 3, 7)])
def test_both_kernel_paths_at_both_extremes(n_env, A, n_src):
    """4096 x 64: four participants per lane, 16-byte loads and stores; max_agents = 3 over 7 source envs (N_src = 21): the
    one-participant-per-lane path on rows that start anywhere"""
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    rng = np.random.default_rng(n_env)
    period, n_slots = 40, 6
    n, ns = n_env * A, n_src * A
    st = rng.standard_normal((n_slots, n_src, A, 6)).astype(np.float32)
    first = rng.integers(0, 3, ns).astype(np.int32)
    last = rng.integers(2, n_slots, ns).astype(np.int32)
    never = rng.uniform(size=ns) < 0.1
    first[never], last[never] = 1, 0
    rows = np.concatenate([H.shape_rows(True)[:4], _replayed_copy(H.shape_rows(True)[:4])])
    tid = rng.integers(0, 8, n).astype(np.uint8)       # half the participants are not replayed ones: untouched
    replayed = tid >= 4
    src_env = (np.arange(n_env) % n_src).astype(np.int32) if n_src != n_env else None
    offset = (rng.integers(0, 3, n_env) * period).astype(np.int32)
    pool = ParticipantPool(n_env, A)
    try:
        src = ReplaySource.from_arrays(pool, st, first, last, 0, period)
        pool.set_param_table(rows)
        x0 = rng.uniform(-100, 100, (4, n)).astype(np.float32)
        act0 = (rng.uniform(size=n) < 0.7).astype(np.uint8)
        pool.reset(x0[0], x0[1], x0[2], x0[3], tid, act0)
        pool.replay_bind(src, src_env, offset)
        mirror, ids0 = _states(pool), pool.download(L.F_IDS)
        se = np.arange(n_env) if src_env is None else src_env
        fw, lw = first.reshape(n_src, A)[se].reshape(-1), last.reshape(n_src, A)[se].reshape(-1)
        flat = st.reshape(n_slots, n_src, A, 6)
        for k in range(3):     # apply at the current stamp, three times over a moving frame
            pool.upload(L.F_FRAME_MS, np.full(n_env, k * period, np.int32))
            pool.replay_apply()
            slot = np.repeat((k * period + offset) // period, A)
            want = replayed & (slot >= fw) & (slot <= lw) & (slot < n_slots)
            now = flat[np.minimum((k * period + offset) // period, n_slots - 1), se].reshape(n, 6)
            mirror[want] = now[want]
            assert _states(pool).tobytes() == mirror.tobytes(), k
            ids = pool.download(L.F_IDS)
            assert (ids[~replayed] == ids0[~replayed]).all()
            assert ((((ids >> 16) & 0xff) == 1) == want)[replayed].all()
            assert ((ids[want] & 0xff) == L.MODEL_REPLAY).all() and (((ids >> 8) & 0xff) == tid).all()
        assert want.sum() > n // 8 and (replayed & ~want).sum() > n // 64
    finally:
        pool.close()


def test_late_replayed_participants_do_not_narrow_the_integrator_of_a_large_pool():
    """2 M participants, every second one a point mass, the others replayed ones that are inactive at t2d_reset: the types
    in use at reset are all point masses, which is the evidence the wide integrator's one-model instantiation is picked on.
    t2d_integrate must integrate the point masses exactly as a pool without the replayed rows does, and nobody else."""
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.participant import pedestrian_row, replayed_row
    from tactics2d_amd.pool import ParticipantPool
    n_env, A, period = 32768, 64, 100
    n = n_env * A
    rng = np.random.default_rng(1)
    rows = np.stack([pedestrian_row("adult_male"), replayed_row("medium_car")])
    tid = (np.arange(n) % 2).astype(np.uint8)
    pm = tid == 0
    x, y = rng.uniform(-200, 200, (2, n)).astype(np.float32)
    vx, vy = rng.uniform(-2, 2, (2, n)).astype(np.float32)
    z = np.zeros(n, np.float32)
    a0, a1 = rng.uniform(-1, 1, (2, n)).astype(np.float32)
    st = rng.standard_normal((2, 1, A, 6)).astype(np.float32)     # one source env shared by every env
    ref = ParticipantPool(n_env, A)
    try:
        ref.set_param_table(rows[:1])
        ref.reset(x, y, z, z, np.zeros(n, np.uint8), pm.astype(np.uint8), vx=vx, vy=vy)
        ref.set_actions(a0, a1)
        ref.integrate(period)
        want = _states(ref)
    finally:
        ref.close()
    pool = ParticipantPool(n_env, A)
    try:
        pool.set_param_table(rows)
        pool.set_status_config(max_step=100000)
        pool.reset(x, y, z, z, tid, pm.astype(np.uint8), vx=vx, vy=vy)
        src = ReplaySource.from_arrays(pool, st, None, None, 0, period)
        pool.replay_bind(src, np.zeros(n_env, np.int32))
        pool.set_actions(a0, a1)
        pool.integrate(period)
        got = _states(pool)
        assert got[pm].tobytes() == want[pm].tobytes()
        assert got[~pm].tobytes() == np.tile(st[1, 0], (n_env, 1, 1)).reshape(n, 6)[~pm].tobytes()
        assert _active(pool).all()
        pool.check_status(period)  # (env time moves on with the status check, not with t2d_integrate)
        pool.integrate(period)     # the replayed ones are now active and past their recording: they leave, untouched
        again = _states(pool)
        assert again[~pm].tobytes() == got[~pm].tobytes() and not _active(pool)[~pm].any() and _active(pool)[pm].all()
        assert (again[pm] != got[pm]).any()
    finally:
        pool.close()


# ----------------------------------------------------------------------------------------------------------------- 11
def test_every_refusal_leaves_the_pool_usable():
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.history import ReplaySource, _TrajBuffer
    from tactics2d_amd.participant import replayed_row, vehicle_row
    from tactics2d_amd.pool import ParticipantPool
    import ctypes as C
    n_env, A, period, n_slots = 8, 4, 40, 24
    rng = np.random.default_rng(0)
    st = rng.uniform(-50, 50, (n_slots, n_env, A, 6)).astype(np.float32)
    rows = np.stack([vehicle_row("medium_car"), replayed_row("small_car")])
    tid = np.tile(np.array([0, 1, 1, 1], np.uint8), n_env)
    z = np.zeros(n_env * A, np.float32)
    pool, other, wide = ParticipantPool(n_env, A), ParticipantPool(n_env, A + 1), ParticipantPool(3, A)
    try:
        pool.set_param_table(rows)
        pool.set_status_config(max_step=100000)
        pool.reset(z, z, z, z, tid)
        src = ReplaySource.from_arrays(pool, st, None, None, 0, period)
        flat = st.reshape(n_slots, -1, 6)
        replayed = tid == 1
        steps = [0]

        def good_step():
            """a successful step on the good binding: the replayed participants move on by one slot"""
            pool.step(period)
            steps[0] += 1
            assert _states(pool)[replayed].tobytes() == flat[steps[0]][replayed].tobytes()

        def refused(code, text, fn):
            with pytest.raises(_ffi.T2DError) as ei:
                fn()
            assert ei.value.code == code and text in str(ei.value), str(ei.value)

        # stepping a pool whose table holds a model-5 row before any binding
        refused(_ffi.ERR_STATE, "t2d_replay_bind", lambda: pool.step(period))
        refused(_ffi.ERR_STATE, "t2d_replay_bind", lambda: pool.integrate(period))
        refused(_ffi.ERR_STATE, "t2d_replay_bind", lambda: pool.step_n(3, period))
        refused(_ffi.ERR_STATE, "t2d_replay_bind", lambda: pool.replay_apply())
        assert pool.step_count() == 0 and (pool.download(L.F_FRAME_MS) == 0).all()
        pool.replay_bind(src)
        good_step()

        def bind(buf=None, n=n_slots, t0=0, per=period, se=None, off=None, first=None, last=None):
            p_ = lambda a: None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.c_void_p)
            pool._ck(pool._lib.t2d_replay_bind(pool._h, (src._buf if buf is None else buf)._live(), n, t0, per, p_(se), p_(off),
                                               p_(first), p_(last)))

        full = np.zeros(n_env * A, np.int32), np.full(n_env * A, n_slots - 1, np.int32)
        cases = [
            ("max_agents", lambda: bind(_TrajBuffer(other, 4))),
            ("src_env", lambda: bind(se=np.r_[np.zeros(n_env - 1), n_env])),
            ("src_env", lambda: bind(se=np.r_[-1, np.zeros(n_env - 1)])),
            ("as many source envs", lambda: bind(_TrajBuffer(wide, 4), n=4)),
            ("n_slots", lambda: bind(n=n_slots + 1)),
            ("n_slots", lambda: bind(n=0)),
            ("period_ms", lambda: bind(per=0)),
            ("t0_ms", lambda: bind(t0=20)),
            ("offset_ms", lambda: bind(off=np.r_[np.zeros(n_env - 1), 20])),
            ("window", lambda: bind(first=full[0], last=np.r_[full[1][:-1], n_slots])),
            ("window", lambda: bind(first=np.r_[-1, full[0][1:]], last=full[1])),
            ("both window arrays", lambda: bind(first=full[0])),
        ]
        for text, fn in cases:
            refused(_ffi.ERR_INVALID, text, fn)
            good_step()       # ... on the binding that was there before: nothing was left half bound
        # first > last is legal
        bind(first=np.r_[1, full[0][1:]], last=np.r_[0, full[1][1:]])
        pool.replay_bind(src)
        # an interval off the grid: nothing stepped
        before = pool.step_count()
        for fn in (lambda: pool.step(period + 10), lambda: pool.integrate(period // 2), lambda: pool.step_n(2, period + 1)):
            refused(_ffi.ERR_INVALID, "multiple", fn)
        assert pool.step_count() == before and (pool.download(L.F_FRAME_MS) == steps[0] * period).all()
        good_step()
        # a source that is still bound cannot be destroyed
        refused(_ffi.ERR_STATE, "still replay", lambda: src._buf.close())
        good_step()
        pool.replay_unbind()
        refused(_ffi.ERR_STATE, "t2d_replay_bind", lambda: pool.step(period))
        pool.replay_bind(src)
        good_step()
        pool.replay_unbind()
        src.close()           # unbound: destroyed
        # ids above 5 are still unknown models
        bad = rows.copy()
        bad[1, L.P_MODEL] = 6
        refused(_ffi.ERR_INVALID, "unknown model", lambda: pool.set_param_table(bad))
    finally:
        pool.close()
        other.close()
        wide.close()


def test_destroying_the_stepped_pool_releases_the_source():
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.participant import replayed_row
    from tactics2d_amd.pool import ParticipantPool
    st = np.zeros((4, 2, 4, 6), np.float32)
    lib_pool, pool = ParticipantPool(2, 4), ParticipantPool(16, 4)
    src = ReplaySource.from_arrays(lib_pool, st, None, None, 0, 40)
    assert src.device_buffer().pool is lib_pool
    pool.set_param_table(replayed_row("small_car")[None])
    pool.replay_bind(src, np.arange(16) % 2)
    pool.close()
    src.close()          # no T2DError: the binding went with the pool
    lib_pool.close()


@pytest.mark.parametrize("scene", ["metric", "cfg2", "cfg3"])
def test_step_form_is_unfused_with_a_binding_and_unchanged_without_a_replayed_row(scene):
    from tactics2d_amd import scenarios as S
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.pool import ParticipantPool
    sc = {"metric": lambda: S.mixed(4096, 64, seed=3), "cfg2": lambda: S.parking(4096), "cfg3": lambda: S.highway(1024, 64)}[scene]()
    pool = ParticipantPool(sc.n_env, sc.A)
    try:
        sc.load(pool)
        forms = (pool.step_form(1), pool.step_form(8))
        assert "unfused" not in forms, forms
        # a binding alone changes nothing while no row of the table is replayed
        st = np.zeros((2, 1, sc.A, 6), np.float32)
        src = ReplaySource.from_arrays(pool, st, None, None, 0, 100)
        pool.replay_bind(src, np.zeros(sc.n_env, np.int32))
        assert (pool.step_form(1), pool.step_form(8)) == forms
        pool.step(100)
        # ... and a replayed row makes it a pool with helper kernels around the step
        if len(sc.rows) < 32:
            from tactics2d_amd.participant import replayed_row
            pool.set_param_table(np.concatenate([sc.rows, replayed_row("small_car")[None]]))
            assert (pool.step_form(1), pool.step_form(8)) == ("unfused", "unfused")
    finally:
        pool.close()
