"""Tile progress of every racing env in one launch (t2d_set_tracks / t2d_track_reset / t2d_track_upload / t2d_track_progress,
t2d_track.hip) against the restatement tests/track_ref.py.  No tolerance appears anywhere: tile_visiting, the count, the mask
words, the status bytes and the reward bits are the restatement's, evaluated on the state, status bytes, flags and step counter
the device holds after its own step launch.

The comparisons are kept from being empty by the bands of tests/track_scenes.py (shares of empty runs, runs of one tile, longer
runs and advancing steps of at least 1 % each, a crossing of the closing tile on every track, every way an episode ends);
tests/test_track.py checks them on the CPU rollout of the same scene, and the pool test below asserts them again on what the
device did.  Every test here needs the track symbols of libt2d_hip.so."""
import ctypes as C

import numpy as np
import pytest

import track_ref as R
import track_scenes as TS

pytestmark = pytest.mark.gpu

RULES = {"forward": R.RULE_FORWARD, "reference": R.RULE_REFERENCE}


class Mirror:
    """A pool loaded with a RaceScene, and the restatement beside it."""

    def __init__(self, oracle, sc, rule="forward", max_advance=8, tracks=None, set_of_env=None, check_off_road=False):
        from tactics2d_amd.pool import ParticipantPool
        self.O, self.sc = oracle, sc
        self.pool = ParticipantPool(sc.n_env, 1)
        sc.load(self.pool, rule, max_advance, check_off_road)
        if tracks is not None:      # the same tracks under another division into sets
            self.pool.set_tracks(tracks, set_of_env, 0, rule, max_advance)
            self.pool.set_track_state(sc.visiting, sc.visited)
        self.prog = sc.progress(RULES[rule], max_advance, check_off_road)
        self.drv = TS.Driver(sc)
        self.tid = np.zeros(sc.n_env, np.uint8)

    def state(self):
        from tactics2d_amd import layout as L
        p = self.pool
        return tuple(p.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED))

    def step(self, write_status=False):
        """one step launch with the driver's actions, one progress launch, everything compared; returns (j0, j1, advanced)"""
        from tactics2d_amd import layout as L
        p, sc = self.pool, self.sc
        p.set_actions(*self.drv.actions(*self.state()))
        p.step(100)
        x, y, h, _ = self.state()
        pst, flags, cnt = p.download(L.F_STATUS), p.download(L.F_FLAGS), p.download(L.F_CNT_STEP)
        rw0 = p.download(L.F_REWARD)
        Q, boxed = R.boxes(self.O, sc.rows, self.tid, x, y, h)
        before = self.prog.visiting.copy()
        restart = (self.prog.status[:, 2] | self.prog.status[:, 3]) != 0
        before[restart] = self.prog.start_visiting[restart]
        j0, j1 = self.prog.step(Q, boxed, pst, flags, cnt)
        p.track_progress(write_status)
        self.compare()
        got_st, got_rw = p.download(L.F_STATUS), p.download(L.F_REWARD)
        if write_status:
            assert np.array_equal(got_st, self.prog.status) and np.array_equal(got_rw.view(np.uint32), self.prog.reward.view(np.uint32))
        else:
            assert np.array_equal(got_st, pst) and np.array_equal(got_rw.view(np.uint32), rw0.view(np.uint32))
        return j0, j1, self.prog.visiting != before

    def compare(self, what=""):
        ts, g = self.pool.track_state(), self.prog
        for name, got, want in (("tile_visiting", ts["tile_visiting"], g.visiting.astype(np.int32)),
                                ("num_visited", ts["num_visited"], g.num_visited),
                                ("mask", ts["mask"], g.mask()), ("status", ts["status"], g.status),
                                ("reward bits", ts["reward"].view(np.uint32), g.reward.view(np.uint32))):
            bad = (got != want).reshape(len(got), -1).any(axis=1)
            assert not bad.any(), (what, name, int(bad.sum()), np.nonzero(bad)[0][:6].tolist(), got[bad][:3], want[bad][:3])

    def close(self):
        self.pool.close()


# --------------------------------------------------------------------------------------------- (a) the fixture drives
def test_the_fixture_drives_give_the_reference_answers_on_the_device(oracle):
    """tests/golden/racing_progress.npz (the reference's own _locate_agent / check_status / _get_rewards on scripted drives):
    the recorded pose goes into the pool, t2d_check_status and t2d_track_progress run, and tile_visiting, the mask, the status
    bytes and the reward bits are the recorded ones at every step of every drive -- and the restatement's"""
    import helpers as H
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool, unpack_track_mask
    fx = TS.FixtureDrives(H.load_npz("racing_tracks.npz"), H.load_npz("racing_progress.npz"))
    n_steps = 0
    for max_step in fx.max_steps:
        drives = fx.group(max_step)
        sc = fx.scene(drives, max_step)
        pool, prog = ParticipantPool(sc.n_env, 1), sc.progress(R.RULE_REFERENCE, 0)
        try:
            sc.load(pool, "reference", 0)
            tid = np.zeros(sc.n_env, np.uint8)
            for k in range(int(fx.length[drives].max())):
                x, y, h, alive = fx.poses(drives, k)
                for f, v in ((L.F_X, x), (L.F_Y, y), (L.F_HEADING, h)):
                    pool.upload(f, v)
                pool.check_status(100)
                pst, flags, cnt = pool.download(L.F_STATUS), pool.download(L.F_FLAGS), pool.download(L.F_CNT_STEP)
                pool.track_progress()
                Q, boxed = R.boxes(oracle, sc.rows, tid, x, y, h)
                prog.step(Q, boxed, pst, flags, cnt)
                ts, want = pool.track_state(), fx.expected(drives, k)
                T = want["visited"].shape[1]
                for name, got, exp in (("tile_visiting", ts["tile_visiting"], want["visiting"]),
                                       ("visited", unpack_track_mask(ts["mask"], T), want["visited"]), ("status", ts["status"], want["status"]),
                                       ("reward", ts["reward"].view(np.uint32), want["reward"].view(np.uint32)),
                                       ("num_visited", ts["num_visited"], want["visited"].sum(axis=1))):
                    bad = (np.asarray(got) != np.asarray(exp)).reshape(len(drives), -1).any(axis=1) & alive
                    assert not bad.any(), (name, k, [fx.names[d] for d in drives[bad]], np.asarray(got)[bad][:2], np.asarray(exp)[bad][:2])
                for name, got, exp in (("tile_visiting", ts["tile_visiting"], prog.visiting), ("mask", ts["mask"], prog.mask()),
                                       ("status", ts["status"], prog.status), ("reward", ts["reward"].view(np.uint32), prog.reward.view(np.uint32))):
                    assert np.array_equal(got, exp), (name, k)      # (ended drives too: both start again from the uploaded state)
                n_steps += int(alive.sum())
        finally:
            pool.close()
    assert n_steps == len(fx.g["pose"])


# ------------------------------------------------------------------------------------------------------ (b) the pool
@pytest.mark.parametrize("rule,max_advance", [("forward", 8), ("reference", 0)])
def test_a_pool_of_1024_envs_on_six_tracks_every_env_every_step(oracle, rule, max_advance):
    sc = TS.build(1024, seed=0)
    m = Mirror(oracle, sc, rule, max_advance)
    try:
        m.compare("after set_track_state")
        rows = [m.step() for _ in range(200)]
    finally:
        m.close()
    roll = dict(j0=np.stack([r[0] for r in rows]), j1=np.stack([r[1] for r in rows]), advanced=np.stack([r[2] for r in rows]))
    run = np.where(roll["j0"] < 0, 0, roll["j1"] - roll["j0"])
    shares = {k: float(v.mean()) for k, v in (("empty", run == 0), ("one", run == 1), ("more", run >= 2), ("advanced", roll["advanced"]))}
    print(rule, shares)
    assert all(s >= 0.01 for s in shares.values()), shares
    assert len(sc.tracks) >= 4 and sc.n_env >= 1024


def test_every_way_an_episode_ends_is_seen_on_the_device(oracle):
    """COMPLETED, time-exceeded, no-action and out-of-bound, each on some env of the pool and each with its reward"""
    sc = TS.build(256, seed=3)
    m = Mirror(oracle, sc, "forward", 8)
    seen = {}
    try:
        for _ in range(130):
            m.step()
            st, rw = m.prog.status, m.prog.reward
            for e in np.nonzero(st[:, 2] | st[:, 3])[0]:
                seen.setdefault((int(st[e, 0]), int(st[e, 1])), float(rw[e]))
    finally:
        m.close()
    assert {(R.COMPLETED, 1), (R.TIME_EXCEEDED, 1), (1, R.NO_ACTION), (1, R.OUT_BOUND)} <= set(seen), seen
    assert seen[(R.TIME_EXCEEDED, 1)] == -1.0 and seen[(1, R.OUT_BOUND)] == -5.0 and seen[(R.COMPLETED, 1)] > 0


def test_off_road_ends_an_episode_when_enabled(oracle):
    """the tiles installed as lane polygons (three short rings and the generated track with the non-convex tile) and
    check_off_road = 1: status 6 / reward -5 from the ego's off-lane flag, behind out-of-bound and ahead of COMPLETED, bit for
    bit the restatement's; the same pool with the option off never says so"""
    from tactics2d_amd import layout as L
    sc = TS.off_road_scene()
    m = Mirror(oracle, sc, "forward", 8, check_off_road=True)
    seen, both = {}, 0
    try:
        for _ in range(60):
            m.step()
            st, rw = m.prog.status, m.prog.reward
            flags = m.pool.download(L.F_FLAGS)
            both += int(((flags & L.FLAG_OUT_BOUND) != 0)[(flags & L.FLAG_OFF_LANE) != 0].sum())
            assert (st[((flags & L.FLAG_OUT_BOUND) != 0) & (st[:, 0] == 1), 1] != R.OFF_LANE).all()
            for e in np.nonzero(st[:, 2] | st[:, 3])[0]:
                seen.setdefault((int(st[e, 0]), int(st[e, 1])), float(rw[e]))
        off = m.prog.status[:, 1] == R.OFF_LANE
    finally:
        m.close()
    assert seen.get((1, R.OFF_LANE)) == -5.0 and (1, R.OUT_BOUND) in seen and both > 0, (seen, both)
    assert off[sc.n_tile > 300].any()
    m = Mirror(oracle, sc, "forward", 8, check_off_road=False)
    try:
        for _ in range(8):
            m.step()
            assert not (m.prog.status[:, 1] == R.OFF_LANE).any()
    finally:
        m.close()


# ----------------------------------------------------------------------------------------------------- (c) windows
@pytest.mark.parametrize("max_advance", [0, 1, 3, 8, 64, 600])
def test_max_advance_windows(oracle, max_advance):
    sc = TS.build(192, seed=5)
    m = Mirror(oracle, sc, "forward", max_advance)
    try:
        for _ in range(60):
            m.step()
    finally:
        m.close()


# ------------------------------------------------------------------------------------- (d) shared and per-env sets
def test_per_env_sets_give_what_shared_sets_give(oracle):
    sc = TS.build(96, seed=7)
    own = [sc.tracks[s] for s in sc.set_of_env]              # every env its own copy of its track
    a = Mirror(oracle, sc, "reference", 0)
    b = Mirror(oracle, sc, "reference", 0, tracks=own, set_of_env=np.arange(sc.n_env, dtype=np.int32))
    try:
        for _ in range(40):
            a.step(); b.step()
            ta, tb = a.pool.track_state(), b.pool.track_state()
            assert all(np.array_equal(ta[k].view(np.uint8), tb[k].view(np.uint8)) for k in ta)
    finally:
        a.close(); b.close()


# ------------------------------------------------------------------------ (e) write_status, restore, the start copy
def test_write_status_and_restore_bring_finished_episodes_back_to_the_start(oracle):
    from tactics2d_amd import layout as L
    sc = TS.build(256, seed=9)
    m = Mirror(oracle, sc, "forward", 8)
    n_back = 0
    try:
        for k in range(140):   # (the launch after a restore starts the env from the progress state the upload gave it: Mirror.compare)
            m.step(write_status=True)
            done = (m.prog.status[:, 2] | m.prog.status[:, 3]) != 0
            m.pool.restore(done_only=True)
            x, y, h, v = m.state()
            cnt, st = m.pool.download(L.F_CNT_STEP), m.pool.download(L.F_STATUS)
            assert np.array_equal(x[done], sc.x[done]) and np.array_equal(y[done], sc.y[done]) and np.array_equal(v[done], sc.speed[done])
            assert np.array_equal(h[done], sc.heading[done]) and (cnt[done] == 0).all() and (st[done] == (1, 1, 0, 0)).all()
            assert (st[~done] == m.prog.status[~done]).all()
            n_back += int(done.sum())
    finally:
        m.close()
    assert n_back >= 20, n_back


def test_track_reset_is_the_reference_reset_map(oracle):
    sc = TS.build(64, seed=11)
    m = Mirror(oracle, sc, "forward", 8)
    try:
        for _ in range(5):
            m.step()
        sel = np.arange(sc.n_env) % 3 == 0
        m.pool.track_reset(sel); m.prog.reset(sel)
        m.compare("after a masked reset")
        ts = m.pool.track_state()
        assert (ts["tile_visiting"][sel] == 0).all() and (ts["num_visited"][sel] == 1).all() and (ts["mask"][sel, 0] == 1).all()
        for _ in range(5):
            m.step()
        m.pool.track_reset(); m.prog.reset()
        m.compare("after a full reset")
    finally:
        m.close()


# ------------------------------------------------------------------------------------------------------ (f) errors
def test_errors():
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.pool import ParticipantPool
    lib = _ffi.lib()
    assert lib.t2d_track_progress(None, 0, None) == _ffi.ERR_INVALID
    assert lib.t2d_set_tracks(None, 0, None, None, None, 0, 0, 0, 0) == _ffi.ERR_INVALID
    assert lib.t2d_track_reset(None, None) == _ffi.ERR_INVALID and lib.t2d_track_upload(None, None, None, None) == _ffi.ERR_INVALID
    sc = TS.build(8, seed=1, tracks=[TS.centred_f32(TS.ellipse_ring(16, 26.0, 26.0))])
    pool = ParticipantPool(8, 1)
    try:
        with pytest.raises(_ffi.T2DError) as ei:      # progress before set_tracks
            pool.track_progress()
        assert ei.value.code == _ffi.ERR_STATE
        with pytest.raises(_ffi.T2DError) as ei:
            pool.track_reset()
        assert ei.value.code == _ffi.ERR_STATE
        ring = lambda n: np.float32(TS.ellipse_ring(n, 5.0 * n, 5.0 * n))
        with pytest.raises(_ffi.GeometryError):       # too many tiles
            pool.set_tracks([ring(L.MAX_TRACK_TILES + 1)])
        with pytest.raises(_ffi.T2DError) as ei:      # n_tile < 3
            pool.set_tracks([ring(16)[:2]])
        assert ei.value.code == _ffi.ERR_INVALID
        for kw in (dict(set_of_env=np.full(8, 1, np.int32)), dict(ego_index=1), dict(max_advance=-1)):
            with pytest.raises(_ffi.T2DError) as ei:
                pool.set_tracks([ring(16)], **kw)
            assert ei.value.code == _ffi.ERR_INVALID, kw
        with pytest.raises(ValueError):
            pool.set_tracks([ring(16)], rule="sideways")
        pool.set_tracks([ring(L.MAX_TRACK_TILES)])    # the capacity itself is accepted
        with pytest.raises(_ffi.T2DError) as ei:      # tracks, but no parameter table / reset yet
            pool.track_progress()
        assert ei.value.code == _ffi.ERR_STATE
        sc.load(pool)
        vis = np.zeros((8, 16), bool); vis[:, 0] = True
        with pytest.raises(_ffi.T2DError) as ei:      # tile_visiting outside the ring
            pool.set_track_state(np.full(8, 16), vis)
        assert ei.value.code == _ffi.ERR_INVALID
        beyond = np.zeros((8, 17), bool); beyond[:, 16] = True
        with pytest.raises(_ffi.T2DError) as ei:      # mask bits beyond n_tile
            pool.set_track_state(np.zeros(8), beyond)
        assert ei.value.code == _ffi.ERR_INVALID
        pool.set_track_state(np.full(8, 15), np.ones((8, 16), bool))   # a failing call left the tracks usable
        assert (pool.track_state()["num_visited"] == 16).all()
        pool.set_tracks(None)
        with pytest.raises(_ffi.T2DError):
            pool.track_progress()
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------ (g) launch counts
def test_one_launch_per_call_and_the_step_launches_what_it_launched_before():
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    sc = TS.build(64, seed=2)

    def stepping(pool):
        pool.profile_enable(True)
        pool.step(100); pool.step_n(8, 100); pool.integrate(100); pool.collide()
        return pool.profile_read(L.PROFILE_TRACK_PROGRESS)[1], [pool.profile_read(k)[1] for k in range(10)], pool.step_form()

    bare = ParticipantPool(sc.n_env, 1)
    pool = ParticipantPool(sc.n_env, 1)
    try:
        sc.load(bare)
        bare.set_tracks(None)
        n0, others0, form0 = stepping(bare)
        sc.load(pool)
        n1, others1, form1 = stepping(pool)
        print("launches per kernel id of step + step_n(8) + integrate + collide:", others1, form1)
        assert n0 == 0 and n1 == 0 and others0 == others1 and form0 == form1
        # what these four calls launch on a one-ego pool, by kernel id (t2d_profile_read): one integrate, one collide + status,
        # one fused (ego) step and one chained launch for the eight steps; nothing else -- as before this launch existed
        assert others1 == [1, 1, 1, 0, 0, 0, 0, 1, 0, 0] and form1 == "ego", (others1, form1)
        pool.profile_enable(True)
        pool.track_progress(); pool.track_progress(True); pool.track_progress()
        ms, n = pool.profile_read(L.PROFILE_TRACK_PROGRESS)
        assert n == 3 and ms > 0
        assert [pool.profile_read(k)[1] for k in range(10)] == [0] * 10
        pool.profile_enable(False)
    finally:
        pool.close(); bare.close()


# ----------------------------------------------------------------------------------------------------- VecRacingEnv
def _oracle_step(O, rows, state, accel, steer, boundary, cfg, cnt, frame, ep):
    E = len(accel)
    tid, act = np.zeros(E, np.uint8), np.ones(E, np.uint8)
    O.set_trig(1)
    o = O.integrate(rows, *state, accel, steer, tid, act, 100)
    O.set_trig(0)
    state = [np.float32(o[:, k]) for k in range(6)]
    flags, _ = O.collide(rows, E, 1, state[0], state[1], state[2], tid, act, None, boundary, None, None, 1)
    st, _, _ = O.status_ex(cfg, 1, flags, 100, cnt, frame, rows, state[0], state[1], state[2], tid, ep)
    return state, flags, st


@pytest.mark.parametrize("rule", ["forward", "reference"])
def test_vec_racing_env_against_the_oracle_step_and_the_restatement(oracle, rule):
    """reset / step / step_torch: the state bit for bit the deterministic oracle's (exact integrator), the progress,
    statuses and rewards the restatement's, for two tracks and 32 envs over 60 steps of random actions"""
    import torch
    from tactics2d_amd import mapgeom
    from tactics2d_amd.envs import VecRacingEnv
    E = 32
    env = VecRacingEnv(E, max_step=50, seed=4, n_tracks=2, progress_rule=rule)
    try:
        obs, infos = env.reset()
        pool = env.scenario_manager.pool
        pool.set_integrator_variant("exact")
        assert obs.shape == (E, 6) and (infos["tile_visiting"] == 0).all() and (infos["num_visited_tile"] == 1).all()
        assert np.array_equal(infos["num_tile"], np.array([len(env.tracks[e % 2]) for e in range(E)]))
        # the start pose is _reset_agent's on the shifted track
        for e in range(E):
            px, py, ph = env.generated[e % 2].start_pose()
            assert obs[e, 0] == np.float32(px) and obs[e, 1] == np.float32(py) and obs[e, 2] == np.float32(np.mod(ph, 2 * np.pi))
        rows = TS.medium_car_row()
        soe = np.arange(E) % 2
        prog = R.Progress(env.tracks, soe, RULES[rule], 8)
        boundary = np.float32([mapgeom.map_boundary(env.tracks[s].reshape(-1, 2), np.float32(env.generated[s].center_line)) for s in soe])
        cfg = oracle.make_config(max_step=50, check_no_action=1, no_action_max_step=100)
        cnt, frame, ep = np.zeros(E, np.int32), np.zeros(E, np.int32), oracle.EpisodeState(E)
        state = [obs[:, k].copy() for k in range(6)]
        rng = np.random.default_rng(0)
        for k in range(60):
            a = env.action_space.sample(rng, E)
            a[:, 1] = np.abs(a[:, 1]) / 2                                # (forward, within the action box: the cars leave tile 0)
            if k < 20 or k >= 40 or k % 2:     # (step, then step_torch and step in turn, then step: a device binding must not outlive its call)
                obs, reward, term, trunc, infos = env.step(a)
                got = dict(status=np.stack([infos["scenario_status"], infos["traffic_status"], term, trunc], 1), reward=reward,
                           tile_visiting=infos["tile_visiting"], num_visited=infos["num_visited_tile"])
            else:
                out = env.step_torch(torch.as_tensor(a, device="cuda"))
                torch.cuda.synchronize()
                obs = np.stack([out[c].cpu().numpy() for c in ("x", "y", "heading", "speed", "vx", "vy")], 1)
                got = {c: out[c].cpu().numpy() for c in ("status", "reward", "tile_visiting", "num_visited")}
            state, flags, st = _oracle_step(oracle, rows, state, a[:, 1].copy(), a[:, 0].copy(), boundary, cfg, cnt, frame, ep)
            assert np.array_equal(np.stack(state, 1).view(np.uint32), np.float32(obs).view(np.uint32)), k
            Q, boxed = R.boxes(oracle, rows, np.zeros(E, np.uint8), state[0], state[1], state[2])
            prog.step(Q, boxed, st, flags, cnt)
            assert np.array_equal(got["status"].astype(np.uint8), prog.status), k
            assert np.array_equal(np.float32(got["reward"]).view(np.uint32), prog.reward.view(np.uint32)), k
            assert np.array_equal(got["tile_visiting"], prog.visiting) and np.array_equal(got["num_visited"], prog.num_visited), k
        assert (prog.status[:, 0] == R.TIME_EXCEEDED).all()          # max_step = 50 has passed
    finally:
        env.close()


def test_vec_racing_env_with_the_off_road_check(oracle):
    """check_off_road=True on the generated track with a non-convex tile (np.random.seed(2)): the tiles go in as lane polygons,
    a car steered off the track ends OFF_LANE with reward -5, and every step is the restatement's on the oracle's flags"""
    from tactics2d_amd import layout as L, mapgeom
    from tactics2d_amd.envs import VecRacingEnv
    E = 8
    env = VecRacingEnv(E, max_step=200, seed=2, check_off_road=True)
    try:
        obs, infos = env.reset()
        assert infos["num_tile"][0] == 402
        pool = env.scenario_manager.pool
        rows = TS.medium_car_row()
        soe = np.zeros(E, int)
        prog = R.Progress(env.tracks, soe, R.RULE_FORWARD, 8, True)
        lanes = TS.lane_csr(env.tracks, soe)
        boundary = np.float32([mapgeom.map_boundary(env.tracks[0].reshape(-1, 2), np.float32(env.generated[0].center_line))] * E)
        tid, act = np.zeros(E, np.uint8), np.ones(E, np.uint8)
        steer = np.float32([-0.5, -0.3, -0.1, 0.0, 0.0, 0.1, 0.3, 0.5])   # the outer envs turn off the track, the middle ones go straight on
        ended = {}
        for k in range(30):
            a = np.stack([steer, np.full(E, 2.0, np.float32)], 1)
            obs, reward, term, trunc, infos = env.step(a)
            x, y, h = (np.float32(obs[:, c]) for c in range(3))
            flags, _ = oracle.collide(rows, E, 1, x, y, h, tid, act, None, boundary, None, lanes, 1)
            assert np.array_equal(pool.download(L.F_FLAGS), flags), k
            Q, boxed = R.boxes(oracle, rows, tid, x, y, h)
            prog.step(Q, boxed, _pool_status(flags, k + 1), flags, np.full(E, k + 1))
            assert np.array_equal(np.stack([infos["scenario_status"], infos["traffic_status"], term, trunc], 1).astype(np.uint8), prog.status), k
            assert np.array_equal(np.float32(reward).view(np.uint32), prog.reward.view(np.uint32)), k
            assert np.array_equal(infos["tile_visiting"], prog.visiting) and np.array_equal(infos["num_visited_tile"], prog.num_visited), k
            for e in np.nonzero(trunc)[0]:
                ended.setdefault(int(e), (int(infos["traffic_status"][e]), float(reward[e])))
        assert (R.OFF_LANE, -5.0) in ended.values() and len(ended) < E, ended
    finally:
        env.close()


def _pool_status(flags, cnt):
    """T2D_F_STATUS of a racing pool whose cars move (no no-action) well before max_step: out-of-bound or normal"""
    st = np.tile(np.uint8([1, 1, 0, 0]), (len(flags), 1))
    out = (flags & 4) != 0
    st[out] = (4, 1, 0, 1)
    return st


def test_vec_racing_env_auto_reset_and_discrete_actions(oracle):
    from tactics2d_amd.envs import InvalidAction, VecRacingEnv
    env = VecRacingEnv(16, max_step=5, continuous=False, auto_reset=True, seed=1)
    try:
        obs0, _ = env.reset()
        with pytest.raises(InvalidAction):
            env.step(np.full(16, 143))
        full_throttle = np.full(16, 12 * 11 + 5)          # steering 0, accel 2
        assert np.allclose(env._discrete_action[12 * 11 + 5], (0.0, 2.0))
        for k in range(6):
            obs, reward, term, trunc, infos = env.step(full_throttle)
        assert trunc.all() and (infos["scenario_status"] == R.TIME_EXCEEDED).all() and (reward == -1).all()
        assert np.array_equal(obs, obs0)                  # back at the start pose in the same call
        obs, reward, term, trunc, infos = env.step(full_throttle)
        assert not trunc.any() and (obs[:, 3] > 0).all()
    finally:
        env.close()
