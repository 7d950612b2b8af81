"""t2d_occupancy_grid / ParticipantPool.occupancy_grid / sensor.OccupancyGrid on the device against the specification
tests/occupancy_ref.py (which tests/test_occupancy_ref.py holds against exact rational arithmetic): mask and weights equal it BIT FOR
BIT IN EVERY CELL, in the product form and in the naive form; then the chain the grid exists for -- two walls with a gap, installed in a
pool, through Dijkstra and hybrid A* and into a route -- and VecParkingEnv(occupancy=...)."""
from fractions import Fraction

import numpy as np
import pytest

import occupancy_ref as R
import occupancy_scenes as S
from tactics2d_amd import layout as L

pytestmark = pytest.mark.gpu

# the participant types of the scenes: (shape, length, width)
TYPES = ((L.SHAPE_OBB, 4.0, 2.0), (L.SHAPE_OBB, 2.5, 1.0), (L.SHAPE_CIRCLE, 0.75, 0.75), (L.SHAPE_CIRCLE, 1.5, 1.5))
GRIDS = ((5, 7), (16, 16), (33, 70))


def type_rows():
    from tactics2d_amd.participant import pedestrian_row, vehicle_row
    rows = []
    for shape, length, width in TYPES:
        row = pedestrian_row("adult_male") if shape == L.SHAPE_CIRCLE else vehicle_row("medium_car")
        row[L.P_LENGTH], row[L.P_WIDTH] = length, width
        rows.append(row)
    return np.array(rows)


def as_installed(ring):
    """t2d_set_static_geometry keeps a ring counter-clockwise: a clockwise one is reversed (vertex i <-> n - 1 - i)"""
    v = np.asarray(ring, np.float32).reshape(-1, 2)
    x, y = v[:, 0].astype(np.float64), v[:, 1].astype(np.float64)
    return v[::-1].copy() if float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y)) < 0 else v


def build_scene(seed, n_env=5, A=5, span=20.0):
    """n_env envs about a window [0, span]^2 placed near (120, -150): env 0 has 260 small rings (a second batch of candidates),
    env 1 none at all, the others a few random ones; A participants each (slot 0 the ego), one inactive with a NaN pose."""
    rng = np.random.default_rng(seed)
    base = np.array([120.0, -150.0])
    rings = []
    for e in range(n_env):
        n = 260 if e == 0 else 0 if e == 1 else int(rng.integers(2, 7))
        size = 0.4 if e == 0 else 2.5
        rings.append([S.convex_ring(rng, base + rng.uniform(-0.2, 1.2, 2) * span, size * rng.uniform(0.5, 1.0)) for _ in range(n)])
    n = n_env * A
    xy = base + rng.uniform(-0.1, 1.1, (n, 2)) * span
    x, y, h = np.float32(xy[:, 0]), np.float32(xy[:, 1]), np.float32(rng.uniform(-7, 7, n))
    tid = rng.integers(0, len(TYPES), n).astype(np.uint8)
    tid[::A] = 0
    tid[1::A] = 2   # (every env has a disc)
    active = np.ones(n, np.uint8)
    active[2 * A + 3] = 0   # env 2, slot 3: inactive ...
    return dict(n_env=n_env, A=A, base=base, span=span, rings=rings, x=x, y=y, h=h, tid=tid, active=active)


def load(sc, nan_inactive=True):
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.traffic import polygons_to_csr
    pool = ParticipantPool(sc["n_env"], sc["A"])
    pool.set_param_table(type_rows())
    pool.set_static_geometry(polygons_to_csr(sc["rings"]))
    pool.set_status_config(max_step=100)
    pool.reset(sc["x"], sc["y"], sc["h"], np.zeros_like(sc["x"]), sc["tid"], sc["active"])
    if nan_inactive:   # ... and its pose is not finite: never looked at
        x = sc["x"].copy()
        x[2 * sc["A"] + 3] = np.nan
        pool.upload(L.F_X, x)
        sc = dict(sc, x=x)
    return pool, sc


def participants_of(sc, e, x=None, y=None, h=None):
    x, y, h = sc["x"] if x is None else x, sc["y"] if y is None else y, sc["h"] if h is None else h
    out = []
    for a in range(sc["A"]):
        i = e * sc["A"] + a
        shape, length, width = TYPES[int(sc["tid"][i])]
        out.append((x[i], y[i], h[i], shape, length, width, int(sc["active"][i])))
    return out


def spec(sc, H, W, cs, origin, inflate, include, exclude, x=None):
    masks, status = [], []
    for e in range(sc["n_env"]):
        m, s = R.occupancy(H, W, cs, origin, inflate, [as_installed(r) for r in sc["rings"][e]], participants_of(sc, e, x), include, exclude)
        masks.append(m)
        status.append(s)
    return np.array(masks), np.array(status)


def check(g, want_mask, want_status, H, W, free_weight=1.0):
    mask, weight = g.mask.cpu().numpy(), g.weight.cpu().numpy()
    assert mask.shape == want_mask.shape and weight.shape == want_mask.shape
    bad = np.argwhere(mask != want_mask)
    assert not len(bad), (len(bad), bad[:5].tolist())
    assert np.array_equal(weight.view(np.uint64), R.weights(want_mask, free_weight).view(np.uint64))
    assert g.status.cpu().tolist() == want_status.tolist()
    assert g.hw.cpu().tolist() == [[H, W]] * len(want_mask)


@pytest.fixture(scope="module")
def scene_pool():
    pool, sc = load(build_scene(5))
    yield pool, sc
    pool.close()


# ------------------------------------------------------------------------------------------- parity with the specification
@pytest.mark.parametrize("H,W", GRIDS)
@pytest.mark.parametrize("naive", (False, True), ids=("product", "naive"))
def test_caller_polygons_and_participants_equal_the_specification_bit_for_bit(scene_pool, H, W, naive):
    """ego excluded (the default), a disc in every env, an inactive participant with a NaN pose, 260 rings in env 0, none in env 1"""
    pool, sc = scene_pool
    cs = sc["span"] / max(H, W)
    origin = (float(sc["base"][0]) + 0.37, float(sc["base"][1]) + 0.11)
    for inflate in (0.0, 0.3, 1.0):
        g = pool.occupancy_grid(H, W, cs, origin, inflate, include_participants=True, naive=naive)
        want, status = spec(sc, H, W, cs, origin, inflate, True, 0)
        assert (status == R.OK).all() and want.any() and not want.all()
        check(g, want, status, H, W)
        assert g.cell_size == cs and g.origin == origin and g.planner_kwargs() == dict(cell_size=cs, origin=origin)


def test_exclude_slot_minus_one_lists_the_ego_and_static_only_lists_no_participant(scene_pool):
    pool, sc = scene_pool
    H, W, cs, origin = 33, 70, 0.3, (float(sc["base"][0]) - 0.4, float(sc["base"][1]) + 5.2)
    with_ego = pool.occupancy_grid(H, W, cs, origin, 0.3, include_participants=True, exclude_slot=-1, free_weight=2.5)
    want, status = spec(sc, H, W, cs, origin, 0.3, True, -1)
    check(with_ego, want, status, H, W, 2.5)
    without = pool.occupancy_grid(H, W, cs, origin, 0.3, include_participants=True, exclude_slot=0)
    assert int(with_ego.mask.sum()) > int(without.mask.sum())
    static = pool.occupancy_grid(H, W, cs, origin, 0.3)
    want, status = spec(sc, H, W, cs, origin, 0.3, False, -1)
    check(static, want, status, H, W)
    assert not want[1].any()   # the env without obstacles is all free


def test_an_active_participant_with_a_non_finite_pose_makes_its_row_invalid_and_no_other():
    pool, sc = load(build_scene(6))
    try:
        x = sc["x"].copy()
        x[3 * sc["A"] + 2] = np.inf   # env 3, slot 2: active
        pool.upload(L.F_X, x)
        H, W, cs, origin = 16, 16, 1.25, (float(sc["base"][0]), float(sc["base"][1]))
        for naive in (False, True):
            g = pool.occupancy_grid(H, W, cs, origin, 0.3, include_participants=True, naive=naive)
            want, status = spec(sc, H, W, cs, origin, 0.3, True, 0, x)
            assert status.tolist() == [R.OK, R.OK, R.OK, R.INVALID, R.OK] and want[3].all() and not want[2].all()
            check(g, want, status, H, W)
        # the same slot excluded, or participants not listed: the pose is never looked at
        g = pool.occupancy_grid(H, W, cs, origin, 0.3, include_participants=True, exclude_slot=2)
        assert g.status.cpu().tolist() == [R.OK] * 5
        g = pool.occupancy_grid(H, W, cs, origin, 0.3)
        assert g.status.cpu().tolist() == [R.OK] * 5
    finally:
        pool.close()


def test_windows_off_the_scene_and_far_larger_than_the_scene(scene_pool):
    pool, sc = scene_pool
    bx, by = float(sc["base"][0]), float(sc["base"][1])
    off = pool.occupancy_grid(16, 16, 0.5, (bx + 500.0, by - 500.0), 1.0, include_participants=True, exclude_slot=-1)
    assert not off.mask.any() and bool((off.weight == 1.0).all()) and off.status.cpu().tolist() == [R.OK] * 5
    H, W, cs, origin = 33, 70, 4.0, (bx - 100.0, by - 50.0)   # 280 m x 132 m about a 20 m scene
    big = pool.occupancy_grid(H, W, cs, origin, 0.3, include_participants=True, exclude_slot=-1)
    want, status = spec(sc, H, W, cs, origin, 0.3, True, -1)
    check(big, want, status, H, W)
    rim = np.ones((H, W), bool)
    rim[1:-1, 1:-1] = False
    assert want[0].any() and not want[:, rim].any()


def test_caller_owned_outputs_are_written_in_place_and_either_may_be_null(scene_pool):
    import torch
    pool, sc = scene_pool
    H, W, cs, origin = 5, 7, 3.0, (float(sc["base"][0]), float(sc["base"][1]))
    want, status = spec(sc, H, W, cs, origin, 0.0, False, -1)
    weight = torch.full((sc["n_env"], H, W), -7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((sc["n_env"], H, W), 9, dtype=torch.uint8, device="cuda")
    g = pool.occupancy_grid(H, W, cs, origin, weight=weight, mask=mask)
    assert g.weight is weight and g.mask is mask
    check(g, want, status, H, W)
    # the C ABI with one output, and with neither hw nor status
    call = lambda w, m: pool._lib.t2d_occupancy_grid(pool._h, H, W, cs, origin[0], origin[1], 0.0, 0, -1, 1.0, w, m, None, None, 0, None)
    weight.fill_(-7.0)
    mask.fill_(9)
    assert call(weight.data_ptr(), None) == 0
    pool.sync()
    assert np.array_equal(weight.cpu().numpy(), R.weights(want)) and bool((mask == 9).all())
    weight.fill_(-7.0)
    assert call(None, mask.data_ptr()) == 0
    pool.sync()
    assert np.array_equal(mask.cpu().numpy(), want) and bool((weight == -7.0).all())
    with pytest.raises(ValueError):
        pool.occupancy_grid(H, W, cs, origin, weight=weight[:, :, :5])
    with pytest.raises(ValueError):
        pool.occupancy_grid(H, W, cs, origin, mask=mask.to(torch.int32))


def test_every_invalid_argument_launches_nothing(scene_pool):
    import torch
    from tactics2d_amd._ffi import ERR_INVALID, T2DError
    pool, sc = scene_pool
    n = sc["n_env"]
    weight = torch.full((n, 8, 8), -7.0, dtype=torch.float64, device="cuda")
    mask = torch.full((n, 8, 8), 9, dtype=torch.uint8, device="cuda")
    hw = torch.full((n, 2), -1, dtype=torch.int32, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    good = dict(H=8, W=8, cs=1.0, ox=0.0, oy=0.0, inflate=0.5, inc=1, exc=0, fw=1.0, w=weight.data_ptr(), m=mask.data_ptr(),
                hw=hw.data_ptr(), st=status.data_ptr(), fmt=0)
    nan, inf = float("nan"), float("inf")
    bad = [dict(H=0), dict(W=0), dict(H=-3), dict(cs=0.0), dict(cs=-1.0), dict(cs=nan), dict(cs=inf), dict(cs=1e-151), dict(cs=1e151),
           dict(inflate=-0.1), dict(inflate=nan), dict(inflate=inf), dict(inflate=1e151), dict(ox=nan), dict(oy=inf), dict(exc=-2),
           dict(exc=sc["A"]), dict(w=None, m=None), dict(w=weight.data_ptr() + 8), dict(m=mask.data_ptr() + 1),
           dict(hw=hw.data_ptr() + 2), dict(st=status.data_ptr() + 1), dict(fw=-1.0), dict(fw=nan), dict(fw=inf), dict(fmt=2)]
    pool.profile_enable(True)
    for change in bad:
        a = dict(good, **change)
        rc = pool._lib.t2d_occupancy_grid(pool._h, a["H"], a["W"], a["cs"], a["ox"], a["oy"], a["inflate"], a["inc"], a["exc"], a["fw"],
                                          a["w"], a["m"], a["hw"], a["st"], a["fmt"], None)
        assert rc == ERR_INVALID, change
    pool.sync()
    assert pool.profile_read(L.PROFILE_OCCUPANCY)[1] == 0
    assert bool((weight == -7.0).all()) and bool((mask == 9).all()) and bool((hw == -1).all()) and bool((status == -1).all())
    with pytest.raises(T2DError):
        pool.occupancy_grid(0, 8, 1.0, (0.0, 0.0))
    pool.occupancy_grid(8, 8, 1.0, (0.0, 0.0), weight=weight, mask=mask)
    pool.sync()
    assert pool.profile_read(L.PROFILE_OCCUPANCY)[1] == 1 and bool((mask != 9).all())
    pool.profile_enable(False)


def test_contact_scenes_on_the_device():
    """the dyadic contact scenes of the specification's own test, one env each: touching and exactly `inflate` away are occupied,
    one fp32 ulp beyond is not"""
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.traffic import polygons_to_csr
    scenes = S.contact_scenes()
    by_inflate = {}
    for sc in scenes:
        by_inflate.setdefault(sc["inflate"], []).append(sc)
    for inflate, group in by_inflate.items():
        pool = ParticipantPool(len(group), 1)
        try:
            pool.set_static_geometry(polygons_to_csr([sc["rings"] for sc in group]))
            sc0 = group[0]
            for naive in (False, True):
                g = pool.occupancy_grid(sc0["H"], sc0["W"], sc0["cell_size"], sc0["origin"], inflate, naive=naive)
                mask = g.mask.cpu().numpy()
                for e, sc in enumerate(group):
                    want, _ = R.occupancy(sc["H"], sc["W"], sc["cell_size"], sc["origin"], inflate, [as_installed(r) for r in sc["rings"]])
                    assert np.array_equal(mask[e], want), sc["name"]
                    assert bool(mask[e][sc["cell"]]) == sc["occupied"], sc["name"]
        finally:
            pool.close()


def test_generated_parking_scenes_list_their_live_quads():
    """scene mode: the live quads of a generated lot (slots whose quad_id is negative are not listed: the slots past n_quads here --
    the library offers no way to clear an id inside a live scene from outside), with the ego's box, in the shared parking window"""
    import torch
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_row
    from tactics2d_amd.sensor import OccupancyGrid, parking_window
    n = 6
    pool = ParticipantPool(n, 1)
    try:
        pool.set_param_table(vehicle_row("medium_car")[None])
        pool.set_status_config(max_step=100)
        size = VEHICLE_TEMPLATE["medium_car"][:2]
        pool.parking_scenes(3, 0.5, size)
        scenes = pool.get_parking_scenes()
        x0, x1, y0, y1 = parking_window(size)
        assert scenes.quads[scenes.quad_id >= 0][..., 0].min() >= x0 and scenes.quads[scenes.quad_id >= 0][..., 0].max() <= x1
        assert scenes.quads[scenes.quad_id >= 0][..., 1].min() >= y0 and scenes.quads[scenes.quad_id >= 0][..., 1].max() <= y1
        holes = (scenes.quad_id[:, :] < 0) & (np.arange(scenes.quads.shape[1])[None] < scenes.n_quads[:, None])
        grid = OccupancyGrid(pool, 33, 70, 0.5, inflate=0.3, include_participants=True, exclude_slot=-1, vehicle_size=size)
        x, y, h = (pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING))
        for naive in (False, True):
            grid.naive = naive
            v = grid.render()
            assert v["occupancy"] is grid.weight and v["occupancy_mask"] is grid.mask
            mask = v["occupancy_mask"].cpu().numpy()
            for e in range(n):
                rings = [scenes.quads[e, q] for q in range(int(scenes.n_quads[e])) if scenes.quad_id[e, q] >= 0]
                ego = [(x[e], y[e], h[e], L.SHAPE_OBB, size[0], size[1], 1)]
                want, st = R.occupancy(33, 70, 0.5, grid.origin, 0.3, rings, ego, True, -1)
                assert st == R.OK and want.any() and np.array_equal(mask[e], want), (e, naive, int(holes[e].sum()))
        assert grid.planner_kwargs() == dict(cell_size=0.5, origin=grid.origin)
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------------ the chain end to end
CS, INFLATE, SIDE = 0.5, 0.5, 24   # a window of 24 x 24 cells over [0, 12]^2
ORIGIN = (0.25, 0.25)


def walls(gap):
    lo, hi = 6.0 - gap / 2, 6.0 + gap / 2
    return [np.float32([(5.5, 0.0), (6.5, 0.0), (6.5, lo), (5.5, lo)]), np.float32([(5.5, hi), (6.5, hi), (6.5, 12.0), (5.5, 12.0)])]


def wall_distance2(px, py, ring):
    """exact squared distance of a point and an axis-aligned wall"""
    xs, ys = [Fraction(float(v)) for v in ring[:, 0]], [Fraction(float(v)) for v in ring[:, 1]]
    px, py = Fraction(float(px)), Fraction(float(py))
    dx, dy = max(min(xs) - px, px - max(xs), 0), max(min(ys) - py, py - max(ys), 0)
    return dx * dx + dy * dy


def wall_pool(gaps):
    from tactics2d_amd.participant import vehicle_row
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.traffic import polygons_to_csr
    n = len(gaps)
    pool = ParticipantPool(n, 1)
    pool.set_param_table(vehicle_row("medium_car")[None])
    pool.set_static_geometry(polygons_to_csr([walls(g) for g in gaps]))
    pool.set_status_config(max_step=100)
    z = np.zeros(n, np.float32)
    pool.reset(z + 2.0, z + 6.0, z, z, np.zeros(n, np.uint8))
    return pool


def test_two_walls_with_a_gap_through_dijkstra_hybrid_astar_and_into_a_route():
    """gaps 4 m and 3.25 m are wider than 2 inflate + 2 cells = 2 m: a path, clear of both walls by more than inflate; 0.75 m is
    narrower than 2 inflate = 1 m: none"""
    from tactics2d_amd import search
    from tactics2d_amd.sensor import OccupancyGrid
    gaps = (4.0, 0.75, 3.25)
    pool = wall_pool(gaps)
    try:
        grid = OccupancyGrid(pool, SIDE, SIDE, CS, ORIGIN, inflate=INFLATE)
        v = grid.render()
        weight = v["occupancy"]
        want = np.array([R.occupancy(SIDE, SIDE, CS, ORIGIN, INFLATE, walls(g))[0] for g in gaps])
        assert np.array_equal(v["occupancy_mask"].cpu().numpy(), want)
        cell = lambda x, y: int(round((y - ORIGIN[1]) / CS)) * SIDE + int(round((x - ORIGIN[0]) / CS))
        src, tgt = np.int32([cell(2.25, 6.25)] * 3), np.int32([cell(10.25, 6.25)] * 3)
        dj = search.Dijkstra.plan_batch(weight, src, tgt, connectivity=8)
        starts, targets = np.float64([[2.0, 6.0, 0.0]] * 3), np.float64([[10.0, 6.0, 0.0]] * 3)
        hy = search.HybridAStar.plan_batch(starts, targets, [0.0, 12.0, 0.0, 12.0], weight, max_iter=20000, **grid.planner_kwargs())
        assert dj.status.cpu().tolist() == [search.FOUND, search.NO_PATH, search.FOUND]
        hs, hl = hy.status.cpu().tolist(), hy.path_len.cpu().tolist()
        assert hs[0] == L.HYBRID_FOUND and hs[2] == L.HYBRID_FOUND and hs[1] != L.HYBRID_FOUND and hl[1] == 0
        limit = Fraction(INFLATE) ** 2
        for e in (0, 2):
            cells = dj.path[e, :int(dj.path_len[e])].cpu().numpy()
            pts = [(ORIGIN[0] + (c % SIDE) * CS, ORIGIN[1] + (c // SIDE) * CS) for c in cells]
            pts += [tuple(p) for p in hy.path[e, :hl[e], :2].cpu().numpy()]
            assert len(cells) >= 16 and hl[e] >= 8
            for px, py in pts:
                for ring in walls(gaps[e]):
                    assert wall_distance2(px, py, ring) > limit, (e, px, py)
        # the hybrid path as the route traffic follows
        cap = 40
        pool.set_routes([[np.float32([[float(k), -50.0 - e] for k in range(cap)])] for e in range(3)], np.arange(3), 0, 1.5)
        count = pool.polyline_routes(hy.path, hy.path_len)
        pool.sync()
        assert count.cpu().tolist() == [min(hl[0], cap), 0, min(hl[2], cap)]
        verts = pool.route_vertices().cpu().numpy().reshape(3, cap, 2)
        assert np.array_equal(verts[0, :hl[0]], np.float32(hy.path[0, :hl[0], :2].cpu().numpy())) and (verts[1, :, 1] == -51.0).all()
    finally:
        pool.close()


def test_vec_parking_env_carries_the_grid_of_the_state_it_returns():
    import torch
    from tactics2d_amd.envs import VecParkingEnv
    from tactics2d_amd.participant import VEHICLE_TEMPLATE
    n, H, W, cs, inflate = 4, 33, 70, 0.5, 0.3
    size = VEHICLE_TEMPLATE["medium_car"][:2]
    plain = VecParkingEnv(n, scene_source="generator", seed=5)
    plain.reset()
    act = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    act[:, 1] = 1.0
    keys = set(plain.step_torch(act))
    assert "occupancy" not in keys and "occupancy_mask" not in keys
    env = VecParkingEnv(n, scene_source="generator", seed=5,
                        occupancy=dict(H=H, W=W, cell_size=cs, inflate=inflate, include_participants=True, exclude_slot=-1))

    def want_now():
        pool = env.scenario_manager.pool
        pool.sync()
        scenes = pool.get_parking_scenes()
        x, y, h = (pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING))
        out = []
        for e in range(n):
            rings = [scenes.quads[e, q] for q in range(int(scenes.n_quads[e])) if scenes.quad_id[e, q] >= 0]
            out.append(R.occupancy(H, W, cs, env.occupancy_grid.origin, inflate, rings, [(x[e], y[e], h[e], L.SHAPE_OBB, size[0], size[1], 1)], True, -1)[0])
        return np.array(out), scenes

    env.reset()
    first, scenes0 = want_now()
    assert np.array_equal(env.occupancy_grid.mask.cpu().numpy(), first)
    for _ in range(3):
        out = env.step_torch(act)
    assert set(out) == keys | {"occupancy", "occupancy_mask"}
    assert out["occupancy"].dtype == torch.float64 and tuple(out["occupancy"].shape) == (n, H, W)
    assert out["occupancy"].data_ptr() == env.occupancy_grid.weight.data_ptr()   # zero-copy: the grid's own buffer
    moved, _ = want_now()
    assert np.array_equal(out["occupancy_mask"].cpu().numpy(), moved)
    assert np.array_equal(out["occupancy"].cpu().numpy().view(np.uint64), R.weights(moved).view(np.uint64))
    env.reset(seed=6)   # new lots: the grid is of them
    fresh, scenes1 = want_now()
    assert not np.array_equal(scenes0.quads, scenes1.quads)
    assert np.array_equal(env.occupancy_grid.mask.cpu().numpy(), fresh) and not np.array_equal(fresh, first)
