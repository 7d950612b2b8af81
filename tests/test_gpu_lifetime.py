"""Who owns the library's device and pinned host memory: every allocation goes through the one owning buffer type of
tactics2d_amd/csrc/t2d_devbuf.h, whose four live counters (device bytes, device blocks, pinned bytes, pinned blocks;
tactics2d_amd.debug.memory()) are the library's own bookkeeping -- every comparison here is exact equality.  Pools come from
tactics2d_amd.debug.pool, at the smallest shapes that reach every allocation."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

E, A = 4, 4
N = E * A
ROUTES = [[np.float32([[0, 0], [40, 0]]), np.float32([[0, 2], [40, 2]])]]      # one set of two 2-vertex routes
ROUTES_B = [[np.float32([[0, 1], [30, 1]]), np.float32([[0, 3], [30, 3]])]]
CAMERA_RANGE = (10.0, 10.0, 10.0, 10.0)
CAMERA_LAYERS = 1 | 8 | 16 | 32    # static, target, participants, arrows: what a pool without lanes (and, at times, tracks) can draw


def _tiles():
    """one host track of the minimum tile count (three quads round the origin)"""
    a = np.linspace(0, 2 * np.pi, 4)
    inner = np.stack([20 * np.cos(a), 20 * np.sin(a)], -1)
    outer = np.stack([30 * np.cos(a), 30 * np.sin(a)], -1)
    return np.float32([[inner[k], outer[k], outer[k + 1], inner[k + 1]] for k in range(3)])


def _row():
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    ego = vehicle_model("medium_car", "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0), steer_range=(-0.524, 0.524))
    return ego.param_row(L.SHAPE_OBB, *VEHICLE_TEMPLATE["medium_car"][:2])[None]


def _base(D):
    """a 4 x 4 pool with a parameter table, geometry with a boundary, targets and their headings, a reset and a snapshot"""
    p = D.pool(E, A)
    p.set_param_table(_row())
    square = np.float32([[60, 60], [64, 60], [64, 64], [60, 64]])
    p.set_static_geometry((np.arange(E + 1, dtype=np.int32), 4 * np.arange(E + 1, dtype=np.int32), np.tile(square, (E, 1))),
                          np.tile(np.float32([-100, 100, -100, 100]), (E, 1)))
    p.set_target_areas(np.tile(np.float64([30, 30, 32, 30, 32, 35, 30, 35]), (E, 1)))
    p.set_target_headings(np.zeros(E))
    p.set_status_config()
    z = np.zeros(N, np.float32)
    p.reset(np.tile(np.float32([0, 8, 16, 24]), E), np.tile(np.float32([0, 0.5, 1.5, 4]), E), z, z, np.zeros(N, np.uint8))
    p.snapshot()
    return p


def _placement(D, p):
    """an identity placement map (the pool's step launch has one workgroup per env, per two envs, or one in all)"""
    from tactics2d_amd._ffi import T2DError
    for n in (E, E // 2, 1):
        try:
            D.set_step_placement(p, np.arange(n, dtype=np.uint32))
            return
        except T2DError:
            continue
    raise AssertionError("no placement map of 4, 2 or 1 workgroups was accepted")


class _Replay:
    """a trajectory of capacity 4 on `p` with one record, one verify_states, and a replay source made of it"""
    def __init__(self, p):
        from tactics2d_amd.history import DeviceTrajectory, ReplaySource
        self.traj = DeviceTrajectory(p, "t", fps=10, capacity=4)
        self.traj.record(p, 0)
        assert p.verify_states(self.traj).shape == (N,)
        self.source = ReplaySource.from_device(self.traj, 0, 100)

    def close(self):
        self.traj.close()


def _launches(torch, p, act):
    """the launches that make a pool allocate buffers of its own on first use, and what they wrote"""
    p.lidar_scan()
    p.lidar_scan_all()
    p.camera_render()
    p.off_route()
    p.track_progress()
    p.rs_plan()
    p.rs_follow(None, act.data_ptr())
    dist, off = p.off_route_all()
    out = dict(dist=dist, off=off, lidar_all=p.lidar_all(), **{k: v.cpu().numpy() for k, v in p.camera_views().items()})
    out.update({"track_" + k: v for k, v in p.track_state().items()})
    return out


def _final(torch, D, p, act, n_beams=8):
    """configuration C: everything that allocates, then the launches"""
    from tactics2d_amd.planner import RSFollower, RSPlanner
    p.set_idm(np.array([[10.0, 1.5, 2.0, 1.0, 3.0, 4.0, 1.875, np.inf]]), np.tile(np.uint8([255, 0, 0, 0]), E))
    p.lidar_config(n_beams, 20.0)
    p.frame_config(n_frames=2)
    p.camera_config(16, 8, CAMERA_RANGE, layers=CAMERA_LAYERS)
    p.set_routes(ROUTES, None, np.tile(np.int32([0, 1, 0, -1]), E), 0.5)
    p.set_tracks_generated(E, 0, regenerate=True)   # (seed 0: the tracks of tests/golden/racing_trackgen.npz, none of them flagged)
    RSFollower(p, RSPlanner(p, "medium_car", steer_hi=0.524))
    return _launches(torch, p, act)


def _everything(torch, D):
    """every subsystem that allocates, on a 4 x 4 pool and (the generated parking scenes) a 4 x 1 pool; returns what to close,
    in order, and the number of subsystems configured"""
    m0 = D.memory()
    p = _base(D)
    fresh = D.memory()
    act = torch.zeros((E, 2), dtype=torch.float32, device="cuda")
    p.set_tracks([_tiles()], None, 0)          # host tracks first, then (in _final) the generated ones
    p.track_progress()
    _final(torch, D, p, act)
    fr = p.step_host(np.zeros((N, 2), np.float32))
    assert fr is not None
    p.set_step_chaining(2)                      # (the chained form whatever the pool's size: it carries the checkpoint)
    p.step_n(4, 100)
    _placement(D, p)
    rep = _Replay(p)
    p.replay_bind(rep.source)
    p.sync()
    # param table, geometry, targets, headings, snapshot, IDM, lidar, scan_all, frame, camera, routes, off_route, tracks, planner,
    # follower, step_n, placement, trajectory, verify_states, replay
    n_subsystems = 20
    assert D.memory()[1] - fresh[1] >= n_subsystems - 5, (D.memory(), fresh)   # (five of them were configured before `fresh`)
    assert D.memory()[1] - m0[1] >= n_subsystems
    assert D.memory()[3] - m0[3] >= 3           # two host frames and the action staging buffer
    q = D.pool(E, 1)
    q.set_param_table(_row())
    before_scenes = D.memory()
    q.parking_scenes(3, regenerate=True)
    q.lidar_config(8, 20.0)
    q.lidar_scan()
    q.step(100)
    q.sync()
    assert D.memory()[1] - before_scenes[1] >= 4
    return [p, rep, q]   # (the pool lets go of the trajectory it replays, then both go)


def test_everything_comes_back():
    """create, configure every subsystem that allocates, close: the four counters return to their first reading -- twice"""
    import torch
    from tactics2d_amd import debug as D
    start = D.memory()
    for cycle in range(2):
        for thing in _everything(torch, D):
            thing.close()
        assert D.memory() == start, (cycle, D.memory(), start)


def test_reconfiguring_costs_what_configuring_costs():
    """a pool that went through other configurations first holds exactly what a pool configured straight away holds"""
    import torch
    from tactics2d_amd import debug as D
    from tactics2d_amd import layout as L
    act = torch.zeros((E, 2), dtype=torch.float32, device="cuda")
    deltas, outs = [], []
    for detour in (True, False):
        m0 = D.memory()
        p = _base(D)
        rep = _Replay(p)
        if detour:
            p.lidar_config(8, 20.0)
            p.lidar_scan()
            p.lidar_scan_all()
            p.camera_config(16, 8, CAMERA_RANGE, layers=CAMERA_LAYERS)
            p.camera_render()
            p.camera_config(8, 8, CAMERA_RANGE, layers=CAMERA_LAYERS, format=L.CAMERA_FORMAT_CLASS)
            p.camera_render()
            p.camera_config(0, 0, None)
            p.set_routes(ROUTES_B, None, 0, 0.5)
            p.off_route()
            p.set_routes(ROUTES, None, 1, 0.25)
            p.clear_routes()
            p.set_tracks([_tiles()], None, 0)
            p.track_progress()
            p.replay_bind(rep.source)
            p.replay_unbind()
        outs.append(_final(torch, D, p, act, n_beams=12))
        p.replay_bind(rep.source)
        p.sync()
        now = D.memory()
        deltas.append(tuple(b - a for a, b in zip(m0, now)))
        p.replay_unbind()
        rep.close()
        p.close()
        assert D.memory() == m0
    assert deltas[0] == deltas[1], deltas
    for k in outs[0]:
        assert np.array_equal(outs[0][k], outs[1][k], equal_nan=True), k


def test_a_refused_call_changes_nothing():
    """calls that fail their argument checks return their error code, move no counter and leave the installation whole"""
    import torch
    from tactics2d_amd import debug as D
    from tactics2d_amd import _ffi, layout as L
    act = torch.zeros((E, 2), dtype=torch.float32, device="cuda")
    p = _base(D)
    try:
        _final(torch, D, p, act)
        p.set_tracks([_tiles()], None, 0)
        p.rs_follow_reset()
        before = _launches(torch, p, act)
        m = D.memory()
        for bad in (lambda: p.set_routes(ROUTES, None, 2, 0.5),                                   # route 2 of a set of two
                    lambda: p.set_tracks([_tiles()], np.int32([0, 0, 1, 0]), 0),                   # set 1 of one
                    lambda: p.camera_config(L.CAMERA_MAX_SIDE + 1, 8, CAMERA_RANGE, layers=CAMERA_LAYERS)):
            with pytest.raises(_ffi.T2DError) as ei:
                bad()
            assert ei.value.code == _ffi.ERR_INVALID
            assert D.memory() == m
        p.rs_follow_reset()
        p.track_reset()
        after = _launches(torch, p, act)
        assert D.memory() == m
        for k in ("dist", "off", "image", "image_class", "track_tile_visiting", "track_num_visited", "track_mask", "track_status",
                  "track_reward"):
            assert np.array_equal(before[k], after[k], equal_nan=True), k
    finally:
        p.close()


def test_generated_tracks_regenerate_after_the_lidar_and_the_camera_are_configured_again():
    """t2d_tracks_regenerate compares the pointers it took at the install with the pool's boundary array and snapshot: calls that
    leave those alone must not reallocate them"""
    import torch
    from tactics2d_amd import debug as D
    act = torch.zeros((E, 2), dtype=torch.float32, device="cuda")
    p = _base(D)
    try:
        _final(torch, D, p, act)
        m = D.memory()
        p.lidar_config(8, 20.0)
        p.camera_config(16, 8, CAMERA_RANGE, layers=CAMERA_LAYERS)
        assert D.memory() == m
        p.track_progress(True)
        p.regenerate_tracks()
        p.sync()
    finally:
        p.close()
