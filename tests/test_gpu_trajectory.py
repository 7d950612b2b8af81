"""Device-resident trajectories (t2d_traj_*) and verify_states on the GPU (t2d_history.hip): the reference's verdicts of
tests/golden/verify_states.npz, recording beside t2d_step, both shape extremes of the verify kernel, growth, the reference's
trajectory rules replayed on device storage, and the error codes."""
import warnings

import numpy as np
import pytest

from test_verify_states import _cases, _replay_reference_trajectory, replay_trajectory_kats

pytestmark = pytest.mark.gpu


def _fields():
    from tactics2d_amd import layout as L
    return (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY)


def _models():
    """the twelve rows of the fixture as the package's model classes"""
    from tactics2d_amd.physics import PointMass, SingleTrackDrift, SingleTrackDynamics, SingleTrackKinematics
    car = dict(lf=4.284 / 2 - 0.880, lr=4.284 / 2 - 0.767, mass=1620.0, mass_height=1.449 / 2)
    return [
        SingleTrackKinematics(lf=1.262, lr=1.375, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)),
        SingleTrackKinematics(lf=1.262, lr=1.375, steer_range=(-0.524, 0.524), speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0)),
        SingleTrackKinematics(lf=1.0, lr=1.2, steer_range=0.6, speed_range=(0.0, 20.0), accel_range=3.0),
        SingleTrackKinematics(lf=1.262, lr=1.375, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44)),
        SingleTrackDynamics(lf=1.262, lr=1.375, mass=1620.0, mass_height=0.726, steer_range=(-0.524, 0.524),
                            speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)),
        PointMass(speed_range=(0.0, 7.0), accel_range=(0.0, 1.5)),
        PointMass(speed_range=(0.0, 7.0), accel_range=(0.3, 2.0)),
        PointMass(speed_range=(0.0, 7.0)),
        PointMass(speed_range=(0.0, 7.0), accel_range=(0.0, 1.5), backend="euler"),
        PointMass(speed_range=(0.0, 7.0), backend="euler"),
        SingleTrackDrift(**car, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)),
        SingleTrackDrift(**car, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44)),
    ]


def _oracle_composition(oracle, rows, type_id, active, frames, intervals):
    """verify_state of every frame k >= 1 against frame 0 (trig=1, the kernels' trig), AND-ed; inactive -> True.
    frames: list of (N, 6) arrays, intervals: int per frame (entry 0 unused)"""
    ok = np.ones(len(type_id), bool)
    last = frames[0].astype(np.float64)
    for f, iv in zip(frames[1:], intervals[1:]):
        ok &= oracle.verify_state(rows, type_id, last, f[:, :4].astype(np.float64), int(iv), trig=1)
    return ok | ~np.asarray(active, bool)


def test_model_verify_states_equals_the_reference_on_every_fixture_case():
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import DeviceTrajectory
    from tactics2d_amd.pool import ParticipantPool
    g = _cases()
    ms = _models()
    cols = [L.P_MODEL, L.P_RANGE_FLAGS, L.P_STEER_LO, L.P_STEER_HI, L.P_SPEED_LO, L.P_SPEED_HI, L.P_ACCEL_LO, L.P_ACCEL_HI,
            L.P_LR, L.P_WB]
    scratch = ParticipantPool(1, 1)
    try:
        scratch.set_param_table(g["rows"][:1])
        scratch.reset([0.0], [0.0], [0.0], [0.0], [0])
        for t, m in enumerate(ms):
            assert np.array_equal(m.param_row()[cols], g["rows"][t][cols]), t
        seen = np.zeros(12, int)
        for t in range(len(g["valid"])):
            m = ms[int(g["type_id"][t])]
            bt = _replay_reference_trajectory(g, t)
            want = bool(g["valid"][t])
            assert bool(m.verify_states(bt)[0]) == want, ("batched", t)
            dt = _replay_reference_trajectory(g, t, cls=lambda **kw: DeviceTrajectory(scratch, capacity=4, **kw))
            assert bool(m.verify_states(dt)[0]) == want, ("device", t)
            dt.close()
            seen[int(g["type_id"][t])] += 1
        assert (seen > 100).all()
    finally:
        scratch.close()
        for m in ms:
            m.close()


def _mixed_pool(n_env, A, seed=5):
    from tactics2d_amd import scenarios as S
    from tactics2d_amd.pool import ParticipantPool
    sc = S.mixed(n_env, A, seed=seed)
    pool = ParticipantPool(sc.n_env, sc.A, 0)
    sc.load(pool)
    return sc, pool


def test_recording_beside_the_step_is_exact_and_changes_nothing(oracle):
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import DeviceTrajectory
    sc, pool = _mixed_pool(4096, 64)
    _, twin = _mixed_pool(4096, 64)
    try:
        a0, a1 = sc.sample_actions(np.random.default_rng(1))
        for p in (pool, twin):
            p.set_actions(a0, a1)
        t10 = DeviceTrajectory(pool, 1, fps=10, capacity=64)
        stamps = [0] + list(np.cumsum(np.random.default_rng(2).choice([50, 100, 150], 32)))
        tun = DeviceTrajectory(pool, 2, fps=10, capacity=64)
        t10.record(pool, 0)
        tun.record(pool, stamps[0])
        after = [np.stack([pool.download(f) for f in _fields()], 1)]
        for k in range(1, 33):
            pool.step(100)
            t10.record(pool, 100 * k)
            tun.record(pool, int(stamps[k]))
            twin.step(100)
            after.append(np.stack([pool.download(f) for f in _fields()], 1))
        assert t10.stable_freq is True and tun.stable_freq is False
        for k in range(33):
            got = t10.get_state(100 * k)
            for c, name in enumerate(("x", "y", "heading")):
                assert np.array_equal(getattr(got, name).view(np.uint32), after[k][:, c].view(np.uint32)), (k, name)
            assert np.array_equal(got.speed.view(np.uint32), after[k][:, 3].view(np.uint32)), k
            assert np.array_equal(got.vx.view(np.uint32), after[k][:, 4].view(np.uint32)), k
        for f in _fields() + (L.F_FLAGS, L.F_STATUS, L.F_REWARD, L.F_RECORD, L.F_CNT_STEP):
            assert np.array_equal(pool.download(f).view(np.uint8), twin.download(f).view(np.uint8)), f
        active = sc.active.astype(bool)
        got = pool.verify_states(t10)
        want = _oracle_composition(oracle, sc.rows, sc.type_id, active, after, [0] + [100] * 32)
        assert np.array_equal(got, want), int((got != want).sum())
        got = pool.verify_states(tun)
        want = _oracle_composition(oracle, sc.rows, sc.type_id, active, after, [0] + [int(s - stamps[0]) for s in stamps[1:]])
        assert np.array_equal(got, want), int((got != want).sum())
        assert not want[active].all()
        t10.close(); tun.close()
    finally:
        pool.close()
        twin.close()


def _random_frames(rng, rows, type_id, n_frames, intervals, outliers=0.002):
    """frame 0 random; frame k a point-mass move of a random acceleration (about half of them inside [0, 1.5]) over interval k,
    or, for the vehicle rows, a small random displacement"""
    N = len(type_id)
    f0 = np.zeros((N, 6), np.float32)
    f0[:, 0:2] = rng.uniform(-100, 100, (N, 2)); f0[:, 2] = rng.uniform(0, 2 * np.pi, N); f0[:, 3] = rng.uniform(0, 10, N)
    f0[:, 4] = f0[:, 3] * np.cos(f0[:, 2]); f0[:, 5] = f0[:, 3] * np.sin(f0[:, 2])
    frames = [f0]
    for k in range(1, n_frames):
        dt = intervals[k] / 1000
        a = rng.uniform(0.05, 1.45, N) * np.where(rng.random(N) < outliers, 3.0, 1.0)
        th = rng.uniform(0, 2 * np.pi, N)
        f = f0.astype(np.float64).copy()
        f[:, 0] += f0[:, 4] * dt + 0.5 * a * np.cos(th) * dt * dt
        f[:, 1] += f0[:, 5] * dt + 0.5 * a * np.sin(th) * dt * dt
        f[:, 2] = np.mod(f0[:, 2] + rng.normal(0, 0.01, N), 2 * np.pi)
        f[:, 3] += rng.normal(0, 0.3, N)
        frames.append(f.astype(np.float32))
    return frames


@pytest.mark.parametrize("N,n_frames", [(262144, 32), (1, 4096)])
def test_verify_kernel_at_both_shape_extremes(oracle, N, n_frames):
    from tactics2d_amd.history import DeviceTrajectory
    from tactics2d_amd.physics import BatchedState
    from tactics2d_amd.pool import ParticipantPool
    g = _cases()
    rng = np.random.default_rng(N + n_frames)
    pool = ParticipantPool(N, 1)
    try:
        pool.set_param_table(g["rows"])
        type_id = rng.choice([5, 5, 6, 8, 0, 2, 4], N).astype(np.uint8) if N > 1 else np.array([5], np.uint8)
        active = rng.random(N) < 0.95 if N > 1 else np.ones(1, bool)
        pool.reset(np.zeros(N), np.zeros(N), np.zeros(N), np.zeros(N), type_id, active.astype(np.uint8))
        for uneven in (False, True):
            iv = [0] + (list(rng.choice([50, 100, 150], n_frames - 1)) if uneven else [100] * (n_frames - 1))
            stamps = np.cumsum(iv) if uneven else 100 * np.arange(n_frames)
            ivs = [0] + [int(s - stamps[0]) for s in stamps[1:]] if uneven else iv
            frames = _random_frames(rng, g["rows"], type_id, n_frames, ivs)
            if N == 1 and not uneven:
                frames[n_frames - 5] = frames[0].copy(); frames[n_frames - 5][:, 0] += 50.0   # one far frame near the end
            traj = DeviceTrajectory(pool, 0, fps=10, capacity=n_frames)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                for f, s in zip(frames, stamps):
                    traj.add_state(BatchedState(int(s), f[:, 0], f[:, 1], f[:, 2], f[:, 4], f[:, 5], speed=f[:, 3]))
            assert traj.stable_freq is (not uneven)
            got = pool.verify_states(traj)
            want = _oracle_composition(oracle, g["rows"], type_id, active, frames, ivs)
            assert np.array_equal(got, want), (uneven, int((got != want).sum()))
            if N > 1:
                assert 0.05 < want.mean() < 0.95
            elif not uneven:
                assert not want[0]
            if N == 1:   # and the all-valid trajectory of the same length: True
                good = DeviceTrajectory(pool, 0, fps=10, capacity=n_frames)
                fr = _random_frames(np.random.default_rng(9), g["rows"], type_id, n_frames, [0] + [100] * (n_frames - 1), 0.0)
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    for k, f in enumerate(fr):
                        good.add_state(BatchedState(100 * k, f[:, 0], f[:, 1], f[:, 2], f[:, 4], f[:, 5], speed=f[:, 3]))
                want = _oracle_composition(oracle, g["rows"], type_id, active, fr, [0] + [100] * (n_frames - 1))
                assert want[0] and np.array_equal(pool.verify_states(good), want)
                good.close()
            traj.close()
    finally:
        pool.close()


def test_growth_keeps_the_contents_and_column_views_have_the_right_shape():
    import torch
    from tactics2d_amd.history import DeviceTrajectory
    sc, pool = _mixed_pool(8, 64)
    try:
        a0, a1 = sc.sample_actions(np.random.default_rng(3))
        pool.set_actions(a0, a1)
        traj = DeviceTrajectory(pool, 0, fps=10, capacity=4)
        want = []
        for k in range(37):
            if k:
                pool.step(100)
            traj.record(pool, 100 * k)
            want.append(np.stack([pool.download(f) for f in _fields()]))
        assert traj.capacity == 64 and len(traj) == 37
        for k in (0, 3, 4, 5, 17, 36):
            s = traj.get_state(100 * k)
            assert np.array_equal(np.stack([s.x, s.y, s.heading, s.speed, s.vx, s.vy]), want[k]), k
        for c, name in enumerate(("x", "y", "heading", "speed", "vx", "vy")):
            v = torch.as_tensor(traj.column(name), device="cuda:0")
            assert tuple(v.shape) == (37, pool.n)
            assert np.array_equal(v.cpu().numpy(), np.stack([w[c] for w in want])), name
        sp = np.stack([w[3] for w in want]).astype(np.float64).mean(0)
        assert np.array_equal(traj.average_speed, sp)
        traj.close()
    finally:
        pool.close()


def test_trajectory_kats_on_device_storage():
    from tactics2d_amd.history import DeviceTrajectory
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(2, 1)
    made = []
    try:
        pool.set_param_table(_cases()["rows"][:1])
        pool.reset([0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0.0, 0.0], [0, 0])

        def make():
            t = DeviceTrajectory(pool, 3, capacity=2)
            made.append(t)
            return t
        replay_trajectory_kats(make)
        assert max(t.capacity for t in made) >= 8
    finally:
        pool.close()
    assert all(not t._buf._h for t in made)   # (closed with their pool)


def test_error_codes_and_exceptions():
    import ctypes as C
    import torch
    from tactics2d_amd import _ffi
    from tactics2d_amd.history import DeviceTrajectory, _TrajBuffer
    from tactics2d_amd.physics import BatchedState
    from tactics2d_amd.pool import ParticipantPool
    lib = _ffi.lib()
    bare = ParticipantPool(4, 1)            # no parameter table, no reset
    other = ParticipantPool(4, 1)
    try:
        buf = _TrajBuffer(bare, 2)
        h = buf._h
        assert lib.t2d_traj_record(h, 0, None) == _ffi.ERR_STATE
        out = torch.zeros(4, dtype=torch.uint8, device="cuda:0")
        slots, iv = np.zeros(1, np.int32), np.zeros(1, np.float64)
        p = lambda a: a.ctypes.data_as(C.c_void_p)
        assert lib.t2d_verify_states(h, 1, p(slots), p(iv), C.c_void_p(out.data_ptr()), None) == _ffi.ERR_STATE
        bare.set_param_table(_cases()["rows"][:1])
        assert lib.t2d_verify_states(h, 1, p(slots), p(iv), C.c_void_p(out.data_ptr()), None) == _ffi.ERR_STATE   # (no reset)
        bare.reset(np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4), np.zeros(4, np.uint8))
        assert lib.t2d_verify_states(h, 1, p(slots), p(iv), C.c_void_p(out.data_ptr()), None) == _ffi.OK
        assert lib.t2d_traj_record(h, 2, None) == _ffi.ERR_INVALID          # slot at capacity
        assert lib.t2d_traj_record(h, -1, None) == _ffi.ERR_INVALID
        assert lib.t2d_traj_read(h, 0, None) == _ffi.ERR_INVALID            # null pointer
        assert lib.t2d_traj_write(h, 5, p(np.zeros(24, np.float32))) == _ffi.ERR_INVALID
        assert lib.t2d_verify_states(h, 0, p(slots), p(iv), C.c_void_p(out.data_ptr()), None) == _ffi.ERR_INVALID
        assert lib.t2d_verify_states(h, 1, None, p(iv), C.c_void_p(out.data_ptr()), None) == _ffi.ERR_INVALID
        assert lib.t2d_verify_states(h, 1, p(np.array([2], np.int32)), p(iv), C.c_void_p(out.data_ptr()), None) == _ffi.ERR_INVALID
        assert lib.t2d_verify_states(h, 1, p(slots), p(iv), None, None) == _ffi.ERR_INVALID
        assert lib.t2d_traj_column(h, 6, C.byref(C.c_void_p()), C.byref(C.c_size_t())) == _ffi.ERR_INVALID
        assert lib.t2d_traj_create(bare._h, 0, C.byref(C.c_void_p())) == _ffi.ERR_INVALID
        assert lib.t2d_traj_record(None, 0, None) == _ffi.ERR_INVALID
        with pytest.raises(_ffi.T2DError) as ei:
            buf.record(7)
        assert ei.value.code == _ffi.ERR_INVALID and "slot" in str(ei.value)
        t = DeviceTrajectory(bare, 0, fps=10, capacity=2)
        with pytest.raises(ValueError):
            t.record(other, 0)                  # another pool
        with pytest.raises(ValueError):
            other.verify_states(t)
        with pytest.raises(IndexError):
            bare.verify_states(t)               # empty (frames[0])
        with pytest.raises(TypeError):
            bare.verify_states(DeviceTrajectory(bare, 0, capacity=1))   # stable, fps None (1000 / None)
        t.add_state(BatchedState(0, np.zeros(4)))
        assert bare.verify_states(t).all()      # one frame
        with pytest.raises(_ffi.T2DError) as ei:
            DeviceTrajectory(other, 0, capacity=1).record(other, 0)      # other: no table, no reset
        assert ei.value.code == _ffi.ERR_STATE
        buf.close()
    finally:
        bare.close()
        other.close()
