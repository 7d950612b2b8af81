"""The BEV camera of every env in one launch (t2d_camera_config / _set_palette / _set_style / _render / _buffers,
t2d_camera.hip) against the fp64 restatement tests/camera_ref.py.

The class image must equal the restatement at every pixel whose centre is at least EDGE_MARGIN = 1e-3 m from every element
edge.  The margin is derived, not fitted: pixels are 0.13 - 0.3 m, an fp32 ulp at the tracks' few-hundred-metre coordinates is
about 3e-5 m, and a pixel centre and an edge test go through a handful of roundings (offset, rotation, two products of the
crossing test).  At most MAX_EXCLUDED = 0.5 % of an image may be left out that way; on the rest there is no mismatch at all."""
import ctypes as C

import numpy as np
import pytest

import camera_ref as R
import track_scenes as TS
from tactics2d_amd import layout as L, sensor

pytestmark = pytest.mark.gpu

EDGE_MARGIN = 1e-3
MAX_EXCLUDED = 0.005


# ------------------------------------------------------------------------------------------------------------ helpers
def expected(env, pose, cam, **kw):
    """camera_ref's class image and edge distances of one env: pose = (x, y, heading) of the bound participant"""
    return R.render_pose(R.elements(**env, **kw), cam.window_size, cam.perception_range, *[float(v) for v in pose], cam.heading_up,
                         dist_cap=0.05)


def check_image(got, want, dist, what):
    keep = dist >= EDGE_MARGIN
    excluded = 1.0 - keep.mean()
    bad = (got != want) & keep
    assert excluded <= MAX_EXCLUDED, (what, excluded)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4], want[bad][:4])
    return excluded


def participants_of(sc, x, y, h, e, class_of_type):
    A = sc.A
    out = []
    for a in range(A):
        i = e * A + a
        t = int(sc.type_id[i])
        out.append((float(x[i]), float(y[i]), float(h[i]), int(sc.rows[t, L.P_SHAPE]), float(np.float32(sc.rows[t, L.P_LENGTH])),
                    float(np.float32(sc.rows[t, L.P_WIDTH])), bool(sc.active[i]), int(class_of_type[t])))
    return out


def csr_env(csr, e):
    if csr is None:
        return []
    eo, vo, xy = csr
    return [np.float64(xy[vo[p]:vo[p + 1]]) for p in range(eo[e], eo[e + 1])]


def poses(pool):
    return tuple(pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING))


def class_table(sc):
    from tactics2d_amd.participant import CYCLIST_TEMPLATE
    c = np.full(L.MAX_TYPES, L.CAMERA_CLASS_VEHICLE, np.uint8)
    for t, name in enumerate(sc.type_names):
        if sc.rows[t, L.P_SHAPE] == L.SHAPE_CIRCLE:
            c[t] = L.CAMERA_CLASS_PEDESTRIAN
        elif name.split(":")[0] in CYCLIST_TEMPLATE:
            c[t] = L.CAMERA_CLASS_CYCLIST
    return c


def scene_pool(sc):
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    return pool


def check_scene(sc, pool, cam, envs, what, tracks=None, set_of_env=None, class_of_type=None, static=True, lanes=True, target=True):
    cls_of = class_table(sc) if class_of_type is None else class_of_type
    img = cam.render_numpy()
    x, y, h = poses(pool)
    worst = 0.0
    for e in envs:
        env = dict(target=sc.target[e] if (target and sc.target is not None) else None, static=csr_env(sc.static, e) if static else [],
                   lanes=csr_env(sc.lanes, e) if lanes else [], tiles=np.float64(tracks[set_of_env[e]]) if tracks is not None else [],
                   participants=participants_of(sc, x, y, h, e, cls_of))
        b = e * sc.A + cam.bind_id
        want, dist = expected(env, (x[b], y[b], h[b]), cam, arrows=bool(cam.layers & L.CAMERA_LAYER_ARROWS))
        worst = max(worst, check_image(img["image_class"][e], want, dist, (what, e)))
        assert np.array_equal(img["image"][e], cam.palette[img["image_class"][e]]), (what, e)
    return img, worst


class _RaceAsScene:
    """what check_scene reads of a scene, for n_env racing envs of one medium_car each"""

    def __init__(self, rs=None, n_env=None):
        self.n_env, self.A, self.rows, self.type_names = rs.n_env if rs is not None else n_env, 1, TS.medium_car_row(), ["medium_car"]
        self.type_id, self.active = np.zeros(self.n_env, np.uint8), np.ones(self.n_env, np.uint8)
        self.static = self.lanes = self.target = None


# ------------------------------------------------------------------------------------------- (a) parity with camera_ref
def test_fixture_scenes_render_as_the_definition():
    """every scene of tests/golden/camera.npz (the geometry BEVCamera listed) through the C ABI: tiles as a track, obstacles as
    static geometry, lanes as lane geometry, the participants as the pool's"""
    import test_camera as TC
    from tactics2d_amd.participant import pedestrian_row, vehicle_row
    from tactics2d_amd.pool import ParticipantPool
    FX = TC.FX
    for s in range(TC.N_SCENE):
        name = str(FX["scene_name"][s])
        ks = [k for k in range(FX["scene_elem_off"][s], FX["scene_elem_off"][s + 1]) if FX["elem_drawn"][k]]
        geo = lambda k: np.float32(FX["elem_xy"][FX["elem_vert_off"][k]:FX["elem_vert_off"][k + 1]])
        lanes = [geo(k) for k in ks if FX["elem_class"][k] == L.CAMERA_CLASS_LANE]
        static = [geo(k) for k in ks if FX["elem_class"][k] == L.CAMERA_CLASS_OBSTACLE]
        target = [geo(k) for k in ks if FX["elem_class"][k] == L.CAMERA_CLASS_TARGET]
        bodies = [k for k in ks if FX["elem_class"][k] in (L.CAMERA_CLASS_VEHICLE, L.CAMERA_CLASS_CYCLIST, L.CAMERA_CLASS_PEDESTRIAN)]
        rows, cls_of, parts = [], np.full(L.MAX_TYPES, L.CAMERA_CLASS_VEHICLE, np.uint8), []
        for t, k in enumerate(bodies):
            if FX["elem_shape"][k]:
                row = pedestrian_row("adult_male")
                row[L.P_LENGTH] = row[L.P_WIDTH] = 2 * FX["elem_radius"][k]
            else:
                row = vehicle_row("medium_car")
                g = geo(k)
                row[L.P_LENGTH], row[L.P_WIDTH] = 2 * g[0][0], 2 * g[1][1]
            rows.append(row)
            cls_of[t] = FX["elem_class"][k]
            parts.append((np.float32(FX["elem_pos"][k][0]), np.float32(FX["elem_pos"][k][1]), np.float32(FX["elem_rot"][k])))
        bind = [t for t, p in enumerate(parts) if p[0] == np.float32(FX["sensor"][s][0]) and p[1] == np.float32(FX["sensor"][s][1])][0]
        A = len(parts)
        pool = ParticipantPool(1, A)
        try:
            pool.set_param_table(np.array(rows))
            racing = name.startswith("racing")
            csr = lambda polys: (np.int32([0, len(polys)]), np.int32(np.concatenate([[0], np.cumsum([len(q) for q in polys])])), np.concatenate(polys))
            pool.set_static_geometry(csr(static) if static else None, None)
            pool.set_lane_geometry(csr(lanes) if lanes and not racing else None)
            pool.set_target_areas(np.float32(target[0])[None] if target else None)
            p = np.array(parts, np.float32)
            pool.reset(p[:, 0], p[:, 1], p[:, 2], np.zeros(A), np.arange(A, dtype=np.uint8))
            if racing:   # (tiles may be non-convex: they go in as a track, which the camera draws undivided)
                pool.set_tracks([np.array(lanes)], None, 0)
            layers = ["participants", "arrows"] + (["static"] if static else []) + (["target"] if target else []) + \
                     (["tracks"] if racing else ["lanes"] if lanes else [])
            W, H = (int(v) for v in FX["wsize"][s])
            cam = sensor.BEVCamera(pool, tuple(FX["prange"][s]), (W, H), bind, bool(FX["yaw"][s] != 0.0), layers)
            cam.set_style(cls_of)
            img = cam.render_numpy()
            x, y, h = poses(pool)
            env = dict(target=target[0] if target else None, static=static, lanes=[] if racing else lanes, tiles=lanes if racing else [],
                       participants=[(x[a], y[a], h[a], int(rows[a][L.P_SHAPE]), float(np.float32(rows[a][L.P_LENGTH])),
                                      float(np.float32(rows[a][L.P_WIDTH])), True, int(cls_of[a])) for a in range(A)])
            want, dist = expected(env, (x[bind], y[bind], h[bind]), cam)
            ex = check_image(img["image_class"][0], want, dist, name)
            assert np.array_equal(img["image"][0], sensor.PALETTE[img["image_class"][0]])
            # ... and it is the image the reference's own listing defines (fp64, from the fixture's doubles): same classes
            # away from the edges -- the margin here is the fp32 rounding of the poses that went into the pool
            W_, H_ = cam.window_size
            win = (FX["xlim"][s][0], FX["xlim"][s][1], FX["ylim"][s][0], FX["ylim"][s][1])
            ref, rdist = R.render(TC.fixture_elements(s), (W_, H_), win, FX["sensor"][s], float(FX["yaw"][s]), dist_cap=0.05)
            keep = rdist >= 2 * EDGE_MARGIN
            assert keep.mean() >= 1 - 2 * MAX_EXCLUDED and np.array_equal(img["image_class"][0][keep], ref[keep]), name
            print(f"{name}: {100 * ex:.3f} % excluded, classes {np.unique(want).tolist()}")
            assert len(np.unique(want)) >= 3
        finally:
            pool.close()


def test_random_racing_envs_render_as_the_definition():
    rs = TS.build(n_env=48, seed=5)
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(rs.n_env, 1)
    try:
        rs.load(pool)
        cam = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"))
        img, worst = check_scene(_RaceAsScene(rs), pool, cam, range(rs.n_env), "racing", tracks=rs.tracks, set_of_env=rs.set_of_env)
        print(f"racing: worst excluded share {100 * worst:.3f} %")
        seen = np.unique(img["image_class"])
        assert {L.CAMERA_CLASS_BACKGROUND, L.CAMERA_CLASS_LANE, L.CAMERA_CLASS_HEADING_ARROW} <= set(seen.tolist())
        # the body of a medium_car resolves to z 1: under the lane; it shows where the car hangs over the track's edge
        assert (img["image_class"] == L.CAMERA_CLASS_LANE).mean() > 0.05
    finally:
        pool.close()


def test_random_parking_envs_render_as_the_definition():
    from tactics2d_amd import scenarios
    sc = scenarios.parking(40, seed0=11)
    pool = scene_pool(sc)
    try:
        cam = sensor.BEVCamera(pool, (20, 20, 20, 20), (200, 200), 0, True, ("static", "target", "participants", "arrows"))
        img, worst = check_scene(sc, pool, cam, range(sc.n_env), "parking")
        print(f"parking: worst excluded share {100 * worst:.3f} %")
        for c in (L.CAMERA_CLASS_OBSTACLE, L.CAMERA_CLASS_TARGET, L.CAMERA_CLASS_VEHICLE, L.CAMERA_CLASS_HEADING_ARROW):
            assert (img["image_class"] == c).any(), c
    finally:
        pool.close()


def test_generated_parking_scenes_render_as_the_definition():
    """scene mode: the obstacles are the generated lots' live quads on the device"""
    from tactics2d_amd.envs import VecParkingEnv
    env = VecParkingEnv(24, scene_source="generator", seed=3, observation="camera")
    try:
        from tactics2d_amd.participant import VEHICLE_TEMPLATE
        length, width = VEHICLE_TEMPLATE["medium_car"][:2]
        obs, _ = env.reset()
        g = env.generated
        pool = env.scenario_manager.pool
        cls = env.camera.render_numpy()["image_class"]
        x, y, h = poses(pool)
        for e in range(24):
            el = dict(target=g.target[e], static=[np.float64(g.quads[e, q]) for q in range(g.n_quads[e]) if g.quad_id[e, q] >= 0],
                      participants=[(x[e], y[e], h[e], L.SHAPE_OBB, float(np.float32(length)), float(np.float32(width)), True,
                                     L.CAMERA_CLASS_VEHICLE)])
            want, dist = expected(el, (x[e], y[e], h[e]), env.camera)
            check_image(cls[e], want, dist, ("generated", e))
            assert np.array_equal(obs[e], sensor.PALETTE[cls[e]])
    finally:
        env.close()


@pytest.mark.parametrize("which", ["intersection", "highway64"])
def test_random_traffic_envs_render_as_the_definition(which):
    """lanes, static obstacles, cars, cyclists and pedestrians; 64 participants per env; a bind_slot other than 0; north-up"""
    from tactics2d_amd import scenarios
    sc = scenarios.intersection(12, A=32, seed=4) if which == "intersection" else scenarios.highway(6, A=64, seed=9)
    sc.active = sc.active.copy()
    sc.active[3::7] = 0                      # inactive participants are not listed
    bind = 5 if which == "intersection" else 17
    sc.active[bind::sc.A] = 1
    pool = scene_pool(sc)
    try:
        layers = ["participants", "arrows"] + (["static"] if sc.static is not None else []) + (["lanes"] if sc.lanes is not None else [])
        for heading_up, prange in ((True, (25, 25, 35, 15)), (False, (30, 30, 30, 30))):
            cam = sensor.BEVCamera(pool, prange, (200, 200), bind, heading_up, layers)
            cam.set_style(class_table(sc))
            img, worst = check_scene(sc, pool, cam, range(sc.n_env), (which, heading_up))
            print(f"{which} heading_up={heading_up}: worst excluded share {100 * worst:.3f} %, classes {np.unique(img['image_class']).tolist()}")
            assert (img["image_class"] == L.CAMERA_CLASS_HEADING_ARROW).any()
            assert sc.lanes is None or (img["image_class"] == L.CAMERA_CLASS_LANE).any()
        assert (sc.active == 0).any()   # (inactive participants were in the scene, and the definition does not list them)
    finally:
        pool.close()


# ---------------------------------------------------------------------------------------------------------- (b) palette
def test_rgb_is_the_palette_applied_to_the_class_image():
    rs = TS.build(n_env=16, seed=2)
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(rs.n_env, 1)
    try:
        rs.load(pool)
        cam = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"))
        a = cam.render_numpy()
        assert np.array_equal(a["image"], sensor.PALETTE[a["image_class"]]) and a["image"].shape == (16, 200, 200, 3)
        pal = np.arange(24, dtype=np.uint8).reshape(8, 3) * 9 + 1
        cam.set_palette(pal)
        b = cam.render_numpy()
        assert np.array_equal(b["image_class"], a["image_class"]) and np.array_equal(b["image"], pal[b["image_class"]])
        # a width that is no multiple of four takes the byte-store path: same classes as the definition
        cam2 = sensor.BEVCamera(pool, (30, 30, 50, 10), (150, 90), 0, True, ("tracks", "participants", "arrows"))
        check_scene(_RaceAsScene(rs), pool, cam2, range(4), "odd width", tracks=rs.tracks, set_of_env=rs.set_of_env)
        # class only / rgb only, and caller-owned images
        import torch
        cam3 = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"), rgb=False)
        v = cam3.render()
        assert set(v) == {"image_class"}
        mine = torch.zeros((16, 200, 200), dtype=torch.uint8, device="cuda")
        pool.camera_render(None, mine.data_ptr(), None)
        pool.sync()
        assert torch.equal(mine, v["image_class"]) and np.array_equal(mine.cpu().numpy(), a["image_class"])
        # the naive form (every pixel tests every element) gives the same image
        cam4 = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"), naive=True)
        assert np.array_equal(cam4.render_numpy()["image_class"], a["image_class"])
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------- (c) geometry coverage
def test_4096_racing_envs_on_shared_tracks_and_windows_off_the_map():
    rs = TS.build(n_env=4096, seed=1)
    assert len(rs.tracks) < rs.n_env
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(rs.n_env, 1)
    try:
        rs.load(pool)
        # some cars far outside their map: wholly off (1e4 m away) and partly off (40 m beyond the boundary)
        x, y, h = poses(pool)
        x = x.copy()
        x[100::512] += 1e4
        x[37::512] = rs.boundary[37::512, 1] + 40.0
        pool.upload(L.F_X, x)
        cam = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"))
        rng = np.random.default_rng(0)
        sample = sorted(set(rng.choice(rs.n_env, 20, replace=False).tolist()) | {100, 612, 37, 549, 0, 4095})
        img, worst = check_scene(_RaceAsScene(rs), pool, cam, sample, "4096", tracks=rs.tracks, set_of_env=rs.set_of_env)
        cls = img["image_class"]
        assert cls.shape == (4096, 200, 200)
        far = cls[100::512]
        assert not (far == L.CAMERA_CLASS_LANE).any() and (far == L.CAMERA_CLASS_BACKGROUND).mean() > 0.99   # only the car itself
        # every env was written: no image is left at the allocation's initial content -- each shows its own car's arrow
        assert ((cls == L.CAMERA_CLASS_HEADING_ARROW).reshape(4096, -1).sum(axis=1) > 0).all()
        # envs on the same track at the same pose give the same image
        pool.upload(L.F_X, np.full(4096, x[0], np.float32)); pool.upload(L.F_Y, np.full(4096, y[0], np.float32))
        pool.upload(L.F_HEADING, np.full(4096, h[0], np.float32))
        cls = cam.render_numpy()["image_class"]
        S = len(rs.tracks)
        assert (cls[::S] == cls[0]).all()
    finally:
        pool.close()


def test_a_non_finite_pose_gives_background_and_does_not_fault():
    rs = TS.build(n_env=8, seed=3)
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(rs.n_env, 1)
    try:
        rs.load(pool)
        x, y, h = poses(pool)
        x = x.copy(); x[2] = np.nan; x[5] = np.inf
        pool.upload(L.F_X, x)
        cam = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"))
        cls = cam.render_numpy()["image_class"]
        assert (cls[[2, 5]] == L.CAMERA_CLASS_BACKGROUND).all() and (cls[0] != L.CAMERA_CLASS_BACKGROUND).any()
    finally:
        pool.close()


# -------------------------------------------------------------------------------------------------- (d) env-level behaviour
def test_racing_env_hands_out_the_declared_observation():
    import torch
    from tactics2d_amd.envs import VecRacingEnv
    env = VecRacingEnv(6, max_step=5, auto_reset=True, seed=2, n_tracks=2, observation="camera")
    try:
        assert env.observation_space.shape == (200, 200, 3) and env.observation_space.dtype == np.uint8
        obs0, _ = env.reset()
        assert obs0.shape == (6, 200, 200, 3) and obs0.dtype == np.uint8 and env.observation_space.contains(obs0[0])
        a = np.tile(np.float32([0.1, 1.5]), (6, 1))
        obs, rew, term, trunc, info = env.step(a)
        assert obs.shape == (6, 200, 200, 3) and not np.array_equal(obs, obs0)
        pool = env.scenario_manager.pool
        # the image shows the pose the returned state shows
        cls = env.camera.render_numpy()["image_class"]
        assert np.array_equal(obs, sensor.PALETTE[cls])
        # step_torch: views, rendered behind the progress / restore launches; max_step = 5 ends every episode at step 5
        act = torch.tensor(a, device="cuda")
        out = env.step_torch(act)
        ptr = out["image"].data_ptr()
        first = out["image"].clone()
        for _ in range(8):
            out = env.step_torch(act)
            torch.cuda.synchronize()
            assert out["image"].data_ptr() == ptr                # the same memory every step: a view, no copy
            if out["status"][:, 3].all():
                break
            assert not torch.equal(out["image"], first)          # ... with new content
        assert out["image"].shape == (6, 200, 200, 3) and out["image_class"].shape == (6, 200, 200)
        assert out["status"][:, 3].all()                         # TIME_EXCEEDED: truncated, and auto-reset put the cars back
        assert np.array_equal(out["image"].cpu().numpy(), obs0)  # ... so the image shows the start pose the state shows
        check_scene(_RaceAsScene(n_env=6), pool, env.camera, range(6), "racing env", tracks=env.tracks, set_of_env=env.track_of_env)
    finally:
        env.close()


def test_parking_env_hands_out_the_declared_observation():
    import torch
    from tactics2d_amd.envs import VecParkingEnv
    env = VecParkingEnv(5, seed=1, observation="camera")
    try:
        obs0, info = env.reset()
        assert obs0.shape == (5, 200, 200, 3) and obs0.dtype == np.uint8
        obs, rew, term, trunc, info = env.step(np.tile(np.float32([0.2, 1.0]), (5, 1)))
        assert obs.shape == (5, 200, 200, 3) and info["state"]["x"].shape == (5,)
        out = env.step_torch(torch.tensor(np.tile(np.float32([0.2, 1.0]), (5, 1)), device="cuda"))
        torch.cuda.synchronize()
        assert out["image"].shape == (5, 200, 200, 3) and out["lidar"].shape[0] == 5
        assert (out["image_class"] == L.CAMERA_CLASS_OBSTACLE).any() and (out["image_class"] == L.CAMERA_CLASS_TARGET).any()
        # the default observation is untouched
        env2 = VecParkingEnv(2, seed=1)
        o2, _ = env2.reset()
        assert o2.shape == (2, 6) and env2.camera is None
        env2.close()
    finally:
        env.close()


# ------------------------------------------------------------------------------------------------------------ (e) errors
def test_error_paths_return_their_status_codes():
    from tactics2d_amd import _ffi
    from tactics2d_amd.pool import ParticipantPool
    rs = TS.build(n_env=4, seed=0)
    pool = ParticipantPool(4, 1)
    try:
        def code(fn, *a, **k):
            with pytest.raises(_ffi.T2DError) as ei:
                fn(*a, **k)
            return ei.value.code
        ok = ((30, 30, 50, 10), 0, True, L.CAMERA_LAYER_TRACKS | L.CAMERA_LAYER_PARTICIPANTS)
        # not configured
        assert code(pool.camera_render) == _ffi.ERR_STATE
        assert code(pool.camera_buffers) == _ffi.ERR_STATE
        assert code(pool.camera_set_palette, sensor.PALETTE) == _ffi.ERR_STATE
        assert code(pool.camera_set_style) == _ffi.ERR_STATE
        # sizes, ranges, slots, layers, formats
        assert code(pool.camera_config, 200, 0, *ok) == _ffi.ERR_INVALID
        assert code(pool.camera_config, -1, 200, *ok) == _ffi.ERR_INVALID
        assert code(pool.camera_config, L.CAMERA_MAX_SIDE + 1, 200, *ok) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, (30, -30, 50, 10), *ok[1:]) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, (30, 30, np.nan, 10), *ok[1:]) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, ok[0], 1, True, ok[3]) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, ok[0], 0, True, 0) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, ok[0], 0, True, 64) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, *ok, 0) == _ffi.ERR_INVALID
        assert code(pool.camera_config, 200, 200, *ok, 8) == _ffi.ERR_INVALID
        assert code(pool.camera_buffers) == _ffi.ERR_STATE            # (none of the failed calls configured anything)
        # configured, but the pool has no parameter table / reset yet
        pool.camera_config(200, 200, *ok)
        assert code(pool.camera_render) == _ffi.ERR_STATE
        rs.load(pool)
        pool.camera_render()
        b = pool.camera_buffers()
        assert b["image_class"][1] == 4 * 200 * 200 and b["image"][1] == 3 * 4 * 200 * 200
        # a layer whose geometry was never set
        for layer in (L.CAMERA_LAYER_STATIC, L.CAMERA_LAYER_LANES, L.CAMERA_LAYER_TARGET):
            pool.camera_config(200, 200, ok[0], 0, True, layer | L.CAMERA_LAYER_PARTICIPANTS)
            assert code(pool.camera_render) == _ffi.ERR_STATE, layer
        pool.set_tracks(None)
        pool.camera_config(200, 200, *ok)
        assert code(pool.camera_render) == _ffi.ERR_STATE
        # palette / style arguments, a misaligned image
        assert code(pool.camera_set_palette, np.zeros((9, 3), np.uint8)) == _ffi.ERR_INVALID
        bad = np.full(L.MAX_TYPES, L.CAMERA_CLASS_LANE, np.uint8)
        assert code(pool.camera_set_style, bad) == _ffi.ERR_INVALID
        assert code(pool.camera_set_style, None, np.zeros(L.CAMERA_N_CLASS, np.uint8)) == _ffi.ERR_INVALID
        pool.camera_config(200, 200, ok[0], 0, True, L.CAMERA_LAYER_PARTICIPANTS)
        assert code(pool.camera_render, None, b["image_class"][0] + 1, None) == _ffi.ERR_INVALID
        pool.camera_render()
        # width = 0 removes the camera
        pool.camera_config(0, 0, None)
        assert code(pool.camera_render) == _ffi.ERR_STATE
        lib = _ffi.lib()
        assert lib.t2d_camera_render(None, None, None, None) == _ffi.ERR_INVALID
        assert lib.t2d_camera_buffers(pool._h, None, None, None, None) == _ffi.ERR_INVALID
    finally:
        pool.close()


def test_profile_counts_the_camera_launch():
    rs = TS.build(n_env=8, seed=0)
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(8, 1)
    try:
        rs.load(pool)
        cam = sensor.BEVCamera(pool, (30, 30, 50, 10), (200, 200), 0, True, ("tracks", "participants", "arrows"))
        pool._ck(pool._lib.t2d_profile_enable(pool._h, 1))
        for _ in range(3):
            cam.render()
        ms, n = C.c_double(), C.c_int64()
        pool._ck(pool._lib.t2d_profile_read(pool._h, L.PROFILE_CAMERA, C.byref(ms), C.byref(n)))
        assert n.value == 3 and ms.value > 0
        pool._ck(pool._lib.t2d_profile_enable(pool._h, 0))
    finally:
        pool.close()
