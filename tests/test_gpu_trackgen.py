"""Racing tracks generated on the device (t2d_generate_tracks / t2d_set_tracks_generated / t2d_tracks_regenerate,
t2d_trackgen.hip) against the specification tests/trackgen_ref.py through its fixture tests/golden/racing_trackgen.npz: bit for
bit, no tolerance anywhere.  Installed tracks are held against a pool that was given the same (downloaded) tracks through the
host path.  Every test here needs the generator's symbols of libt2d_hip.so."""
import zlib

import numpy as np
import pytest

import helpers as H

pytestmark = pytest.mark.gpu

N = 64


@pytest.fixture(scope="module")
def fx():
    return H.load_npz("racing_trackgen.npz")


@pytest.fixture(scope="module")
def batch(fx):
    """the fixture's 64 tracks from one launch, downloaded once"""
    from tactics2d_amd.generator import RacingTrackGenerator
    return RacingTrackGenerator().generate_batch(N, int(fx["seed"]))


def _crc(t):
    return zlib.crc32(np.ascontiguousarray(t, np.float32).tobytes())


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _same_track(fx, stream, tiles, n_tile, pose, boundary, what):
    """a generated record against the fixture's track of stream index `stream`"""
    assert int(n_tile) == int(fx["n_tile"][stream]) == len(tiles), (what, stream)
    assert _crc(tiles) == int(fx["crc"][stream]), (what, stream)
    assert np.array_equal(_bits(np.float64(pose)), _bits(fx["start_pose"][stream])), (what, stream)
    assert np.array_equal(_bits(np.float32(boundary)), _bits(fx["boundary"][stream])), (what, stream)


def test_the_batch_is_the_fixture_bit_for_bit(fx, batch):
    for name in ("n_checkpoint", "n_tile", "attempt", "flags"):
        assert np.array_equal(getattr(batch, name).astype(np.int64), fx[name].astype(np.int64)), name
    assert [_crc(t) for t in batch.tiles] == fx["crc"].tolist()
    for t in fx["full"]:
        assert np.array_equal(_bits(batch.tiles[t]), _bits(fx[f"tiles_{t}"])), int(t)
    assert np.array_equal(_bits(batch.start_pose), _bits(fx["start_pose"]))
    assert np.array_equal(_bits(batch.boundary), _bits(fx["boundary"]))
    assert np.array_equal(_bits(batch.start_line), _bits(fx["start_line"]))


def test_a_split_batch_gives_identical_bytes(fx, batch):
    from tactics2d_amd.generator import RacingTrackGenerator
    gen, seed = RacingTrackGenerator(), int(fx["seed"])
    parts = [gen.generate_batch(n, seed, first_track=first) for first, n in ((0, 1), (1, 3), (4, 60))]
    tiles = [t for p in parts for t in p.tiles]
    assert len(tiles) == N and all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(tiles, batch.tiles))
    for name in ("n_tile", "n_checkpoint", "attempt", "start_pose", "start_line", "boundary", "flags"):
        assert np.array_equal(_bits(np.concatenate([getattr(p, name) for p in parts])), _bits(getattr(batch, name))), name


def test_only_the_first_n_tile_records_of_a_slot_are_written(fx):
    """the capacity layout: a launch into NaN-filled memory leaves everything beyond n_tile untouched"""
    import torch
    from tactics2d_amd import _ffi, layout as L
    n, dev = 3, "cuda:0"
    tiles = torch.full((n, L.MAX_TRACK_TILES, 4, 2), float("nan"), device=dev)
    i32 = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
    pose, line, bound = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 2, 2), device=dev), torch.zeros((n, 4), device=dev)
    _ffi.check(_ffi.lib().t2d_generate_tracks(0, n, int(fx["seed"]), 0, 4.284, tiles.data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(),
                                              i32[2].data_ptr(), pose.data_ptr(), line.data_ptr(), bound.data_ptr(), i32[3].data_ptr(),
                                              torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    host = tiles.cpu().numpy()
    for t in range(n):
        k = int(fx["n_tile"][t])
        assert int(i32[0][t]) == k and _crc(host[t, :k]) == int(fx["crc"][t]) and np.isnan(host[t, k:]).all()


# ------------------------------------------------------------------------------------------------ installed tracks
def _manager(n_env, max_step):
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    from tactics2d_amd.traffic import BatchedScenarioManager
    length, width = VEHICLE_TEMPLATE["medium_car"][:2]
    m = BatchedScenarioManager(n_env, 1, max_step, 100)
    ego = vehicle_model("medium_car", "kinematics", steer_range=(-0.5, 0.5), accel_range=(-4.0, 2.0))
    m.configure(ego.param_row(L.SHAPE_OBB, length, width)[None], check_dynamic=False, check_off_lane=False, check_arrival=0,
                check_no_action=1, no_action_max_step=100, shaped_reward=0)
    return m


def _device_pool(n_env, seed, max_step=1000, **kw):
    """what VecRacingEnv(track_source="device").reset() does"""
    m = _manager(n_env, max_step)
    m.status_checklist["out_bound"].reset(np.zeros((n_env, 4), np.float32))
    z = np.zeros(n_env)
    m.reset(z, z, z, z, np.zeros(n_env, np.uint8))
    m.pool.set_tracks_generated(n_env, seed, **kw)
    return m


def _host_pool(gen, n_env, max_step=1000):
    """the same tracks (downloaded records `gen` of n_env sets) through the host path: boundary, reset, snapshot, set_tracks"""
    m = _manager(n_env, max_step)
    m.status_checklist["out_bound"].reset(np.float32(gen["boundary"]))
    pose = gen["start_pose"]
    z = np.zeros(n_env)
    m.reset(pose[:, 0], pose[:, 1], pose[:, 2], z, np.zeros(n_env, np.uint8))
    m.pool.set_tracks(gen["tiles"], np.arange(n_env, dtype=np.int32), 0, "forward", 8)
    return m


def _fields(pool):
    from tactics2d_amd import layout as L
    out = {f"F{f}": pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY, L.F_STATUS, L.F_REWARD, L.F_FLAGS,
                                               L.F_CNT_STEP)}
    out.update(pool.track_state())
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(_bits(a[k]) if a[k].dtype.kind == "f" else a[k], _bits(b[k]) if b[k].dtype.kind == "f" else b[k]), (what, k)


def _drive(pool, k, n_env):
    steer = np.float32(0.2 * np.sin(0.7 * k + np.arange(n_env)))
    pool.set_actions(np.full(n_env, 1.5, np.float32), steer)
    pool.step(100)
    pool.track_progress(True)


_STATE = ("F_X", "F_Y", "F_HEADING", "F_SPEED", "F_VX", "F_VY", "F_STATUS", "F_REWARD", "F_FLAGS", "F_CNT_STEP")


def _boundary_and_snapshot(d, h, fx, gen, n_env, what):
    """The env boundary and the episode snapshot of both pools, read through what they do -- the pool hands out neither.  The
    boundary: an ego at heading 0 whose box ends 0.01 m inside a side of its track's boundary is in bound, 0.01 m beyond it out
    of bound, at all four sides (the boundary's values are whole metres: a wrong one is at least a metre off; 0.01 m is some
    hundred fp32 ulps at these coordinates, below 1024 m).  The snapshot: a restore puts every state column where the host
    path's snapshot puts it, the ego on the fixture's start pose.  The pools' columns are put back afterwards, so the drive
    goes on where it was."""
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE
    length, width = VEHICLE_TEMPLATE["medium_car"][:2]
    saved = [{f: m.pool.download(getattr(L, f)) for f in _STATE} for m in (d, h)]
    b = np.float64(gen["boundary"])
    assert (b[:, 0] < -length).all() and (b[:, 1] > length).all() and (b[:, 2] < -length).all() and (b[:, 3] > length).all()
    # (side, x, y) with the box's end on the side: xmin, xmax, ymin, ymax
    ends = ((0, b[:, 0] + length / 2, 0 * b[:, 0]), (1, b[:, 1] - length / 2, 0 * b[:, 0]),
            (2, 0 * b[:, 0], b[:, 2] + width / 2), (3, 0 * b[:, 0], b[:, 3] - width / 2))
    for side, x, y in ends:
        outward = (-1.0, 1.0, -1.0, 1.0)[side]
        for off, want in ((-0.01, False), (0.01, True)):
            for m in (d, h):
                m.pool.upload(L.F_X, np.float32(x + (off * outward if side < 2 else 0.0)))
                m.pool.upload(L.F_Y, np.float32(y + (off * outward if side >= 2 else 0.0)))
                m.pool.upload(L.F_HEADING, np.zeros(n_env, np.float32))
                m.pool.check_status(100)
            fd, fh = d.pool.download(L.F_FLAGS), h.pool.download(L.F_FLAGS)
            assert np.array_equal(fd, fh) and (((fd & L.FLAG_OUT_BOUND) != 0) == want).all(), (what, side, off, fd, fh)
    for m in (d, h):
        m.pool.restore()
    fd, fh = _fields(d.pool), _fields(h.pool)
    _assert_same({k: v for k, v in fd.items() if k.startswith("F")}, {k: v for k, v in fh.items() if k.startswith("F")}, what + ": restored")
    pose = np.float32(fx["start_pose"][:n_env])
    for k, f in enumerate((L.F_X, L.F_Y, L.F_HEADING)):
        assert np.array_equal(_bits(d.pool.download(f)), _bits(pose[:, k])), (what, k)
    assert not d.pool.download(L.F_SPEED).any()
    for m, cols in zip((d, h), saved):
        for f, v in cols.items():
            m.pool.upload(getattr(L, f), v)


def test_an_installed_track_is_the_host_installed_one_in_every_field(fx):
    """set_tracks_generated on 5 envs against set_tracks + boundary + reset + snapshot with the downloaded tracks, after the
    install and after each of 10 steps: state columns, progress buffers and num_tile bit for bit; the env boundary through the
    out-bound event 0.01 m either side of each of its four sides, and the snapshot through a restore (_boundary_and_snapshot)"""
    from tactics2d_amd import layout as L
    E, seed = 5, int(fx["seed"])
    d = _device_pool(E, seed)
    gen = d.pool.generated_tracks()
    for e in range(E):
        _same_track(fx, e, gen["tiles"][e], gen["n_tile"][e], gen["start_pose"][e], gen["boundary"][e], "install")
    h = _host_pool(gen, E)
    try:
        assert np.array_equal(d.pool.track_n_tile, h.pool.track_n_tile) and np.array_equal(d.pool.track_n_tile, fx["n_tile"][:E])
        _assert_same(_fields(d.pool), _fields(h.pool), "after the install")
        _boundary_and_snapshot(d, h, fx, gen, E, "after the install")
        _assert_same(_fields(d.pool), _fields(h.pool), "after the install, columns put back")
        for k in range(10):
            for m in (d, h):
                _drive(m.pool, k, E)
            _assert_same(_fields(d.pool), _fields(h.pool), f"step {k}")
            _boundary_and_snapshot(d, h, fx, gen, E, f"step {k}")
        assert (d.pool.track_state()["num_visited"] > 1).any(), "nobody advanced: the comparison would be empty"
        assert (d.pool.download(L.F_SPEED) > 1.0).all(), "the columns were not put back: the drive started over"
    finally:
        d.close(); h.close()


def test_the_tail_of_a_slot_is_never_read(fx):
    """the slots' tails filled with NaN after the install: 20 steps of progress equal those on the same tiles installed
    through t2d_set_tracks (which holds no tail at all).  Both egos start at 12 m/s: from rest 20 steps of 0.1 s cover 3 m,
    one tile edge, and the march would never look past the tiles it began on; at 12 m/s they cover more than two 10 m tiles"""
    import torch
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import _DevArray
    E, seed = 4, int(fx["seed"])
    d = _device_pool(E, seed)
    gen = d.pool.generated_tracks()
    b, S = d.pool.generated_track_buffers()
    slots = torch.as_tensor(_DevArray(b["tiles"], (S, L.MAX_TRACK_TILES, 4, 2), "<f4", d.pool), device="cuda:0")
    for e in range(E):
        slots[e, int(gen["n_tile"][e]):] = float("nan")
    torch.cuda.synchronize()
    h = _host_pool(gen, E)
    try:
        for m in (d, h):
            m.pool.upload(L.F_SPEED, np.full(E, 12.0, np.float32))
        for k in range(20):
            for m in (d, h):
                _drive(m.pool, k, E)
            _assert_same(d.pool.track_state(), h.pool.track_state(), f"step {k}")
        assert (d.pool.track_state()["num_visited"] > 2).all()
    finally:
        d.close(); h.close()


def test_finished_episodes_move_on_to_the_track_of_their_next_stream(fx):
    """6 envs whose step counters start apart, so that they run out of time at different steps, two episodes each: after every
    finish the env's slot is the fixture's track of stream e + k * stride with its count, boundary and start pose; terminal
    status and reward are the finished episode's; the restore that follows starts at the new pose; the others' slots keep
    their bytes"""
    from tactics2d_amd import layout as L
    E, seed, max_step = 6, int(fx["seed"]), 7
    d = _device_pool(E, seed, max_step=max_step, regenerate=True)
    try:
        d.pool.upload(L.F_CNT_STEP, np.arange(E, dtype=np.int32))      # env e has e steps behind it
        episode = np.zeros(E, np.int64)
        before = d.pool.generated_tracks()
        finishes = 0
        for k in range(2 * max_step + 4):
            if (episode >= 2).all():
                break
            d.pool.set_actions(np.full(E, 1.0, np.float32), np.zeros(E, np.float32))
            d.pool.step(100)
            d.pool.track_progress(True)
            d.pool.regenerate_tracks()
            d.pool.restore(done_only=True)
            ts, gen = d.pool.track_state(), d.pool.generated_tracks()
            done = (ts["status"][:, 2] | ts["status"][:, 3]) != 0
            x, y, hd, v = (d.pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED))
            st, rw = ts["status"], ts["reward"]      # (the racing result is the track status: the restore clears T2D_F_STATUS)
            for e in range(E):
                if done[e]:
                    episode[e] += 1
                    finishes += 1
                    stream = e + episode[e] * E
                    _same_track(fx, stream, gen["tiles"][e], gen["n_tile"][e], gen["start_pose"][e], gen["boundary"][e], f"step {k} env {e}")
                    assert ts["num_tile"][e] == fx["n_tile"][stream]
                    # the finished episode's result stays readable: scenario TIME_EXCEEDED (3), traffic NORMAL, truncated, reward -1
                    assert st[e].tolist() == [3, 1, 0, 1] and rw[e] == -1.0, (k, e, st[e], rw[e])
                    assert (x[e], y[e], hd[e], v[e]) == tuple(np.float32(fx["start_pose"][stream]).tolist()) + (0.0,), (k, e)
                else:
                    assert np.array_equal(_bits(gen["tiles"][e]), _bits(before["tiles"][e])), (k, e)
                    assert st[e, 2] == 0 and st[e, 3] == 0
            assert np.array_equal(gen["episode"], episode)
            before = gen
        assert finishes == 2 * E and (episode == 2).all()
        d.pool.sync()      # (no track was flagged: the sticky word stays clear)
    finally:
        d.close()


def test_what_generated_tracks_refuse(fx):
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.envs import VecRacingEnv
    from tactics2d_amd.generator import RacingTrackGenerator
    with pytest.raises(ValueError):
        VecRacingEnv(4, track_source="device", check_off_road=True)
    with pytest.raises(ValueError):
        VecRacingEnv(4, track_source="device", new_track_per_episode=True)       # (needs auto_reset)
    with pytest.raises(ValueError):
        VecRacingEnv(4, new_track_per_episode=True, auto_reset=True)              # (needs the device generator)
    with pytest.raises(ValueError):
        RacingTrackGenerator().generate_batch(2, 0, first_track=-1)
    import torch
    buf = torch.zeros(L.MAX_TRACK_TILES * 8 + 64, device="cuda:0")      # tiles, start line and boundary are stored 16 bytes at a time
    i32 = torch.zeros(16, dtype=torch.int32, device="cuda:0")
    pose = torch.zeros(3, dtype=torch.float64, device="cuda:0")
    for skew in ((4, 0, 0), (0, 8, 0), (0, 0, 12)):
        tiles, line, bound = buf.data_ptr() + skew[0], buf.data_ptr() + L.MAX_TRACK_TILES * 32 + skew[1], buf.data_ptr() + L.MAX_TRACK_TILES * 32 + 64 + skew[2]
        rc = _ffi.lib().t2d_generate_tracks(0, 1, 0, 0, 4.284, tiles, i32.data_ptr(), i32.data_ptr() + 4, i32.data_ptr() + 8, pose.data_ptr(),
                                            line, bound, i32.data_ptr() + 12, None)
        assert rc == _ffi.ERR_INVALID, skew
    m = _manager(4, 100)
    try:
        m.status_checklist["out_bound"].reset(np.zeros((4, 4), np.float32))
        z = np.zeros(4)
        m.reset(z, z, z, z, np.zeros(4, np.uint8))
        pool = m.pool
        with pytest.raises(ValueError):
            pool.set_tracks_generated(4, 0, check_off_road=True)
        with pytest.raises(_ffi.T2DError) as ei:     # regeneration needs a set per env
            pool.set_tracks_generated(2, 0, set_of_env=np.int32([0, 1, 0, 1]), regenerate=True)
        assert ei.value.code == _ffi.ERR_INVALID
        with pytest.raises(_ffi.T2DError) as ei:
            pool.set_tracks_generated(4, 0, track_stride=3, regenerate=True)
        assert ei.value.code == _ffi.ERR_INVALID
        with pytest.raises(_ffi.T2DError) as ei:     # no tracks yet
            pool.regenerate_tracks()
        assert ei.value.code == _ffi.ERR_STATE
        pool.set_tracks_generated(2, int(fx["seed"]), set_of_env=np.int32([0, 1, 0, 1]))      # shared sets: fine without regeneration
        assert pool.track_n_tile.tolist() == fx["n_tile"][[0, 1, 0, 1]].tolist()
        assert pool.track_state()["num_tile"].tolist() == fx["n_tile"][[0, 1, 0, 1]].tolist()
        with pytest.raises(_ffi.T2DError) as ei:
            pool.regenerate_tracks()
        assert ei.value.code == _ffi.ERR_STATE
    finally:
        m.close()


def test_the_camera_shows_the_new_track_after_an_auto_reset(fx):
    """VecRacingEnv(track_source="device", new_track_per_episode=True, observation="camera"), 4 envs: the class image of the step
    that ended every episode equals a render of a fresh pool given the new tracks through the host path"""
    import torch
    from tactics2d_amd.envs import VecRacingEnv, CAMERA_WINDOW
    from tactics2d_amd.sensor import BEVCamera
    E, max_step = 4, 3
    env = VecRacingEnv(E, max_step=max_step, auto_reset=True, seed=int(fx["seed"]), track_source="device", new_track_per_episode=True,
                       observation="camera")
    h = None
    try:
        obs, infos = env.reset()
        assert obs.shape == (E, 200, 200, 3) and infos["num_tile"].tolist() == fx["n_tile"][:E].tolist()
        first = env.camera.render_numpy()["image_class"]
        act = torch.zeros((E, 2), device="cuda:0")
        act[:, 1] = 1.0
        out = None
        for k in range(max_step + 2):
            out = env.step_torch(act)
            torch.cuda.synchronize()
            if out["status"][:, 3].bool().all():
                break
        assert out["status"][:, 3].bool().all(), "no episode ended"
        gen = env.scenario_manager.pool.generated_tracks()
        for e in range(E):
            _same_track(fx, e + E, gen["tiles"][e], gen["n_tile"][e], gen["start_pose"][e], gen["boundary"][e], "camera")
        assert out["num_tile"].cpu().numpy().tolist() == fx["n_tile"][E:2 * E].tolist()
        got = out["image_class"].cpu().numpy()
        h = _host_pool(gen, E)
        cam = BEVCamera(h.pool, (30, 30, 50, 10), CAMERA_WINDOW, 0, True, ("tracks", "participants", "arrows"))
        want = cam.render_numpy()["image_class"]
        assert np.array_equal(got, want)
        assert not np.array_equal(got, first), "the image did not change: the comparison shows nothing"
    finally:
        env.close()
        if h is not None:
            h.close()
