"""The lidar scan of EVERY participant of every env in one launch (t2d_lidar_scan_all, lidar_all_kernel).

The yardstick is the one tests/test_lidar.py holds the ego scan to: `oracle.lidar(..., ego_index=j, ..., trig=0)`, stacked over
j into [n_env, A, n_beams] by `stacked_oracle` below; the kernel must equal it bit for bit.  No tolerance appears in a GPU test.

The bands of the bit-identity tests (share of finite beams over the rows of active sensors strictly between 0.02 and 0.98;
hits for a sensor j != 0 in at least half of the envs) were checked with the CPU oracle alone before these tests were written:

    scene (participants as obstacles)   (360, 20 m)   (120, 12 m)   (1024, 35 m)    envs with hits at some j != 0
    mixed(96, 64, seed=6)        on       0.267         0.221         0.312           1.00
    mixed(96, 64, seed=6)        off      0.066         0.045         0.088           0.67
    intersection(100, 32, seed=3) on      0.323         0.239         0.415           1.00
    intersection(100, 32, seed=3) off     0.176         0.114         0.271           1.00
    highway(64, 64, seed=2)      on       0.299         0.241         0.357           1.00
    parking(700, seed0=9)        (A = 1)  inside the band at all three; no sensor j != 0 exists, that condition is vacuous

so no listed scene needed another range or seed."""
import ctypes as C

import numpy as np
import pytest

import helpers as H

CONFIGS = [(360, 20.0, None), (120, 12.0, None), (1024, 35.0, None), (120, 20.0, 360)]   # beams, range, subsample_of


def stacked_oracle(oracle, rows, n_env, A, x, y, heading, type_id, active, static, part, beams, max_range, subsample_of=None,
                   trig=0):
    """oracle.lidar with every participant j as the sensor -> float32 [n_env, A, beams].  subsample_of = N: every
    (N / beams)-th beam of the N-beam scan (the same angles as pool.lidar_config(beams, ..., subsample_of=N))."""
    full = beams if subsample_of is None else subsample_of
    out = np.stack([oracle.lidar(rows, n_env, A, j, x, y, heading, type_id, active, static, int(part), full, max_range, trig=trig)
                    for j in range(A)], 1)
    return np.ascontiguousarray(out[:, :, ::full // beams])


def _stacked_scene(oracle, sc, part, beams, max_range, sub=None, x=None, y=None, h=None, active=None):
    return stacked_oracle(oracle, sc.rows, sc.n_env, sc.A, sc.x if x is None else x, sc.y if y is None else y,
                          sc.heading if h is None else h, sc.type_id, sc.active if active is None else active, sc.static,
                          part, beams, max_range, sub)


def _same_bits(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype == np.float32, (got.shape, want.shape)
    diff = got.view(np.uint32) != want.view(np.uint32)
    assert not diff.any(), (int(diff.sum()), np.argwhere(diff)[:5].tolist())


def _bands(want, active, A):
    """the conditions that keep a bit-identity test from passing on empty scans"""
    act = np.asarray(active).reshape(want.shape[0], A).astype(bool)
    fin = np.isfinite(want)
    rate = fin[act].mean()
    print(f"finite share over active sensors {rate:.4f}")
    assert 0.02 < rate < 0.98, rate
    if A > 1:
        envs = fin[:, 1:, :].any(axis=(1, 2)).mean()
        print(f"envs with hits at a sensor j != 0: {envs:.3f}")
        assert envs >= 0.5, envs


def _scene(name):
    from tactics2d_amd import scenarios as S
    return {"mixed": lambda: S.mixed(96, 64, seed=6), "intersection": lambda: S.intersection(100, 32, seed=3),
            "highway": lambda: S.highway(64, 64, seed=2), "parking": lambda: S.parking(700, seed0=9)}[name]()


# ------------------------------------------------------------------------------------------------------ CPU
def _rings_of_env(sc, e, sensor, with_participants, oracle, trig):
    eo, vo, xy = sc.static if sc.static is not None else (np.zeros(sc.n_env + 1, int), np.zeros(1, int), np.zeros((0, 2)))
    rings = [np.float64(xy[vo[p]:vo[p + 1]]) for p in range(eo[e], eo[e + 1])]
    if with_participants:
        for j in range(sc.A):
            i = e * sc.A + j
            r = sc.rows[sc.type_id[i]]
            if j != sensor and sc.active[i] and r[18] == 0:
                rings.append(oracle.pose_obb(sc.x[i], sc.y[i], sc.heading[i], r[19], r[20], trig))
    return rings


def test_stacked_oracle_follows_the_numpy_restatement_off_the_ego_index(oracle):
    """The yardstick is valid for sensors j != 0: the stacked C oracle (trig = 1, libm) against oracle/lidar_ref.py -- the
    restatement pinned to the reference's own statements by tests/golden/lidar.npz -- for every active sensor, participants
    as obstacles: the same finite / inf pattern and distances within 2e-6 (the bound tests/test_lidar.py uses for j = 0)."""
    from oracle import lidar_ref
    from tactics2d_amd import scenarios as S
    for sc in (S.mixed(9, 64, seed=4), S.intersection(6, 32, seed=8)):
        out = stacked_oracle(oracle, sc.rows, sc.n_env, sc.A, sc.x, sc.y, sc.heading, sc.type_id, sc.active, sc.static, 1, 360,
                             20.0, trig=1)
        mism = 0; worst = 0.0; hits = 0; sensors = 0
        for e in range(sc.n_env):
            for j in range(sc.A):
                i = e * sc.A + j
                if not sc.active[i]:
                    assert np.isinf(out[e, j]).all()
                    continue
                sensors += 1
                ref = lidar_ref.scan((float(sc.x[i]), float(sc.y[i]), float(sc.heading[i])), _rings_of_env(sc, e, j, 1, oracle, 1),
                                     20.0, 360)
                fin = np.isfinite(ref)
                mism += int((np.isfinite(out[e, j]) != fin).sum())
                both = fin & np.isfinite(out[e, j])
                hits += int(both.sum())
                if both.any():
                    worst = max(worst, float(np.abs(out[e, j][both] - ref[both]).max()))
        print(sc.name, "sensors", sensors, "mismatched beams", mism, "worst", worst, "hits", hits)
        assert mism == 0 and worst < 2e-6 and hits > 300 * sc.A // 2, (sc.name, mism, worst, hits)


def test_the_interface_is_there():
    from tactics2d_amd import _ffi
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.traffic import BatchedScenarioManager
    vp = C.c_void_p
    assert _ffi.SYMBOLS["t2d_lidar_scan_all"] == (C.c_int, [vp, vp, vp])
    assert _ffi.SYMBOLS["t2d_lidar_all_buffer"] == (C.c_int, [vp, C.POINTER(vp), C.POINTER(C.c_size_t)])
    for name in ("lidar_scan_all", "lidar_all"):
        assert callable(getattr(ParticipantPool, name))
    assert callable(BatchedScenarioManager.get_lidar_observation)


# ------------------------------------------------------------------------------------------------------ GPU
def _loaded(sc):
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    return pool


def _poses(pool):
    from tactics2d_amd import layout as L
    x, y, h = (pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING))
    active = ((pool.download(L.F_IDS) >> 16) & 0xff).astype(np.uint8)
    return x, y, h, active


@pytest.mark.gpu
@pytest.mark.parametrize("scene,part", [("mixed", True), ("mixed", False), ("intersection", True), ("intersection", False),
                                        ("highway", True), ("parking", False)])
def test_gpu_lidar_all_is_bit_identical_to_the_stacked_oracle(oracle, scene, part):
    """every (env, participant) row, four beam configurations, then again after three steps with auto-reset armed"""
    sc = _scene(scene)
    pool = _loaded(sc)
    for beams, rng_max, sub in CONFIGS:
        pool.lidar_config(beams, rng_max, part, subsample_of=sub)
        pool.lidar_scan_all()
        got = pool.lidar_all()
        want = _stacked_scene(oracle, sc, part, beams, rng_max, sub)
        assert got.shape == (sc.n_env, sc.A, beams)
        _same_bits(got, want)
        _bands(want, sc.active, sc.A)
    pool.set_auto_reset(True)
    rng = np.random.default_rng(0)
    for _ in range(3):
        pool.set_actions(*sc.sample_actions(rng)); pool.step(100)
    pool.lidar_config(360, 20.0, part)
    pool.lidar_scan_all()
    got = pool.lidar_all()
    x, y, h, active = _poses(pool)
    want = _stacked_scene(oracle, sc, part, 360, 20.0, None, x, y, h, active)
    _same_bits(got, want)
    _bands(want, active, sc.A)
    pool.close()


@pytest.mark.gpu
def test_gpu_lidar_all_without_any_obstacle_is_all_inf(oracle):
    """a highway env has no static polygon: without the participants as obstacles no beam of any sensor returns"""
    sc = _scene("highway")
    pool = _loaded(sc)
    pool.lidar_config(360, 20.0, False)
    pool.lidar_scan_all()
    got = pool.lidar_all()
    pool.close()
    assert got.shape == (sc.n_env, sc.A, 360) and np.isposinf(got).all()


@pytest.mark.gpu
@pytest.mark.parametrize("ego", [0, 5])
def test_gpu_lidar_all_row_of_the_ego_equals_the_ego_scan_and_leaves_the_status_alone(oracle, ego):
    from tactics2d_amd import layout as L
    sc = _scene("mixed")
    rng = np.random.default_rng(3)
    acts = [sc.sample_actions(rng) for _ in range(2)]

    def run(with_scan):
        pool = _loaded(sc)
        pool.set_status_config(**dict(sc.status, ego_index=ego))
        pool.lidar_config(360, 20.0, True)
        cfg0 = bytes(pool.status_config)
        pool.set_actions(*acts[0]); pool.step(100)
        rows = None
        if with_scan:
            pool.lidar_scan()
            one = pool.download(L.F_LIDAR)
            pool.lidar_scan_all()
            rows = (one, pool.lidar_all())
            pool.lidar_scan()   # (the ego scan after the all-scan: still the ego's)
            assert np.array_equal(pool.download(L.F_LIDAR).view(np.uint32), one.view(np.uint32))
        assert bytes(pool.status_config) == cfg0
        pool.set_actions(*acts[1]); pool.step(100)
        st = tuple(pool.download(f) for f in (L.F_STATUS, L.F_REWARD, L.F_CNT_STEP, L.F_ENV_FLAGS, L.F_X))
        pool.close()
        return rows, st

    (one, every), st_scan = run(True)
    _, st_plain = run(False)
    _same_bits(np.ascontiguousarray(every[:, ego, :]), one)
    _bands(every, sc.active, sc.A)
    for a, b in zip(st_scan, st_plain):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.gpu
def test_gpu_lidar_all_inactive_and_non_finite_sensors(oracle):
    """rows of inactive participants are all +inf; a participant with a NaN x has an all-+inf row and is no obstacle to
    anybody else; every other row still equals the oracle (pedestrians are sensors, and no obstacles)"""
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    rng = np.random.default_rng(77)
    n_env, A = 48, 24
    sc = H.random_scene(rng, n_env, A, (60.0, 30.0), n_static=5, with_peds=True, inactive_frac=0.15)
    pool = ParticipantPool(n_env, A)
    pool.set_param_table(sc["rows"])
    pool.set_static_geometry(sc["static"], sc["boundary"], sc["boundary_valid"])
    pool.reset(sc["x"], sc["y"], sc["heading"], np.zeros(n_env * A, np.float32), sc["type_id"], active=sc["active"])
    pool.lidar_config(360, 20.0, True)

    def check(x):
        pool.lidar_scan_all()
        got = pool.lidar_all()
        want = stacked_oracle(oracle, sc["rows"], n_env, A, x, sc["y"], sc["heading"], sc["type_id"], sc["active"], sc["static"],
                              1, 360, 20.0)
        _same_bits(got, want)
        _bands(want, sc["active"], A)
        return got

    got = check(sc["x"])
    act = sc["active"].reshape(n_env, A).astype(bool)
    assert (~act).sum() > 50 and np.isposinf(got[~act]).all()
    peds = (sc["rows"][sc["type_id"], 18] == 1).reshape(n_env, A) & act
    assert peds.sum() > 50 and np.isfinite(got[peds]).any()
    # NaN x for one active box participant per env that somebody sees
    x = sc["x"].copy()
    boxes = (sc["rows"][sc["type_id"], 18] == 0).reshape(n_env, A) & act
    victims = [e * A + int(np.nonzero(boxes[e])[0][0]) for e in range(n_env) if boxes[e].any()]
    x[victims] = np.nan
    pool.upload(L.F_X, x)
    got2 = check(x)
    assert np.isposinf(got2.reshape(n_env * A, 360)[victims]).all()
    assert (got2.view(np.uint32) != got.view(np.uint32)).any(axis=2).sum() > len(victims)   # others lost an obstacle
    pool.close()


def _limit_scene(rng, n_env, A, n_static_verts):
    """A participants (boxes, a few inactive) among octagons (+ one smaller polygon) of n_static_verts vertices per env"""
    rows = H.shape_rows(False)
    N = n_env * A
    ext = (90.0, 60.0)
    per_env = []
    for _ in range(n_env):
        polys, left = [], n_static_verts
        while left > 0:
            k = 8 if left >= 11 or left == 8 else (left if left <= 8 else left - 3)
            ang = 2 * np.pi * (np.arange(k) + rng.uniform(0, 0.3, k)) / k
            r = rng.uniform(0.8, 2.0)
            c = [rng.uniform(-ext[0] / 2, ext[0] / 2), rng.uniform(-ext[1] / 2, ext[1] / 2)]
            polys.append(np.float32(np.stack([r * np.cos(ang), 0.7 * r * np.sin(ang)], 1) + c))
            left -= k
        per_env.append(polys)
    return dict(rows=rows, n_env=n_env, A=A, x=rng.uniform(-ext[0] / 2, ext[0] / 2, N).astype(np.float32),
                y=rng.uniform(-ext[1] / 2, ext[1] / 2, N).astype(np.float32), heading=rng.uniform(0, 6.3, N).astype(np.float32),
                type_id=rng.integers(0, len(rows), N).astype(np.uint8), active=(rng.uniform(size=N) >= 0.05).astype(np.uint8),
                static=H.to_csr(per_env))


@pytest.mark.gpu
def test_gpu_lidar_all_at_the_limits(oracle):
    """max_agents = T2D_MAX_AGENTS = 256 with the participants as obstacles (1024 edge slots) and as many static vertices as
    the lidar's LDS check still lets through at 360 beams -- (40 B per slot) * slots + 16 B * 360 + 2048 <= 60 KiB: 1340
    slots, i.e. 316 static vertices --: equal to the oracle.  One vertex more: T2D_ERR_GEOMETRY where the configuration is
    installed, and from either scan."""
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.pool import ParticipantPool
    A, beams = L.MAX_AGENTS, 360
    assert A == 256
    n_max = (60 * 1024 - 2048 - 16 * beams) // 40 - 4 * A
    assert n_max == 316
    n_env = 3
    sc = _limit_scene(np.random.default_rng(5), n_env, A, n_max)
    assert np.diff(sc["static"][1][sc["static"][0]]).tolist() == [n_max] * n_env
    pool = ParticipantPool(n_env, A)
    pool.set_param_table(sc["rows"])
    pool.set_static_geometry(sc["static"], None, None)
    pool.reset(sc["x"], sc["y"], sc["heading"], np.zeros(n_env * A, np.float32), sc["type_id"], active=sc["active"])
    pool.lidar_config(beams, 20.0, True)
    pool.lidar_scan_all()
    got = pool.lidar_all()
    want = stacked_oracle(oracle, sc["rows"], n_env, A, sc["x"], sc["y"], sc["heading"], sc["type_id"], sc["active"], sc["static"],
                          1, beams, 20.0)
    _same_bits(got, want)
    _bands(want, sc["active"], A)
    pool.lidar_scan()
    _same_bits(pool.download(L.F_LIDAR), np.ascontiguousarray(want[:, 0, :]))
    # one vertex more
    sc1 = _limit_scene(np.random.default_rng(5), n_env, A, n_max + 1)
    with pytest.raises(_ffi.GeometryError) as ei:
        pool.set_static_geometry(sc1["static"], None, None)
    assert ei.value.code == _ffi.ERR_GEOMETRY
    for scan in (pool.lidar_scan, pool.lidar_scan_all):
        with pytest.raises(_ffi.GeometryError) as ei:
            scan()
        assert ei.value.code == _ffi.ERR_GEOMETRY and "too many obstacle edges" in str(ei.value)
    pool.close()


@pytest.mark.gpu
def test_gpu_lidar_all_destinations_and_ordering(oracle):
    import torch
    from tactics2d_amd import _ffi
    sc = _scene("intersection")
    pool = _loaded(sc)
    pool.lidar_config(360, 20.0, True)
    with pytest.raises(_ffi.T2DError) as ei:   # no NULL-destination scan yet
        pool.lidar_all_buffer()
    assert ei.value.code == _ffi.ERR_STATE
    # into a caller's tensor on a stream of its own, right behind the step on that stream: no sync in between
    obs = torch.zeros((sc.n_env, sc.A, 360), dtype=torch.float32, device="cuda")
    st = torch.cuda.Stream()
    st.wait_stream(torch.cuda.current_stream())
    pool.set_actions(*sc.sample_actions(np.random.default_rng(1)))
    pool.step(100, st.cuda_stream)
    pool.lidar_scan_all(obs.data_ptr(), st.cuda_stream)
    st.synchronize()
    with pytest.raises(_ffi.T2DError):   # a caller-owned destination does not create the pool's buffer
        pool.lidar_all_buffer()
    x, y, h, active = _poses(pool)
    assert (x != sc.x).any()
    want = _stacked_scene(oracle, sc, True, 360, 20.0, None, x, y, h, active)
    _same_bits(obs.cpu().numpy(), want)
    _bands(want, active, sc.A)
    # the pool's own buffer follows the configuration
    pool.lidar_scan_all()
    ptr, nb = pool.lidar_all_buffer()
    assert ptr and nb == sc.n_env * sc.A * 360 * 4
    _same_bits(pool.lidar_all(), want)
    pool.lidar_config(120, 12.0, True)
    pool.lidar_scan_all()
    ptr, nb = pool.lidar_all_buffer()
    assert ptr and nb == sc.n_env * sc.A * 120 * 4
    _same_bits(pool.lidar_all(), _stacked_scene(oracle, sc, True, 120, 12.0, None, x, y, h, active))
    pool.close()


@pytest.mark.gpu
def test_gpu_scenario_manager_lidar_observation(oracle):
    import torch
    from tactics2d_amd.traffic import BatchedScenarioManager
    sc = _scene("mixed")
    m = BatchedScenarioManager(sc.n_env, sc.A, step_size=100)
    sc.load(m.pool)
    m.pool.lidar_config(120, 12.0, True)
    want = _stacked_scene(oracle, sc, True, 120, 12.0)
    _bands(want, sc.active, sc.A)
    got = m.get_lidar_observation()
    assert isinstance(got, np.ndarray)
    _same_bits(got, want)
    out = torch.zeros((sc.n_env, sc.A, 120), dtype=torch.float32, device="cuda")
    assert m.get_lidar_observation(out) is out
    torch.cuda.synchronize()
    _same_bits(out.cpu().numpy(), want)
    with pytest.raises(ValueError):
        m.get_lidar_observation(torch.zeros((sc.n_env, sc.A, 360), dtype=torch.float32, device="cuda"))
    assert m.get_observation().shape == (sc.n_env, 6)
    m.close()
