"""What t2d_off_route, t2d_pid_actions and t2d_pursuit_actions share -- the route set staged in LDS, the launch shape, a lane's
prologue (t2d_scripted_dev.h) -- and what t2d_set_idm, t2d_set_pid and t2d_set_pursuit share -- one order, one rule "a participant
has one controller", one uninstall (t2d_api.hip) -- at the shapes where shared code can go wrong although each copy was right.

Staging: the small scenes of the other files stage one two-vertex route, so neither staging loop takes a second trip.  Here a
pool of 2 x 3 (a 64-lane block) whose env 0 uses a set of 64 routes of 3 vertices -- 192 vertices and 65 table entries: both
loops wrap -- with its participants on routes 0, 31 and 63, and whose env 1 uses a set of one two-vertex route (fewer vertices
than lanes); and a pool of 1 x 65 (a 128-lane block with a single lane in its second wave) under PID lon_mode 2 and pursuit ACC,
participant 64 parked between 30 and 31: the leader of 30 sits in the other wave, and so does 64's own.  One participant per
pool is inactive, for the NaN slot of the (x, y) staging.  The comparisons are the ones of test_gpu_off_route.py (bit-equal),
test_gpu_pid.py and test_gpu_pursuit.py (their _check: bit-equal where those files hold it, 1e-9 elsewhere), against
tests/route_ref.py, pid_ref.py and pursuit_ref.py, the leaders and the IDM law from the C oracle.  The scenes are checked with
the references alone first (_not_vacuous): nobody lands in NONFINITE or NO_ROUTE, every active participant gets an action.
"""
import numpy as np
import pytest

import pid_ref as PR
import pursuit_ref as UR
import route_ref as RR
import test_gpu_off_route as TO
import test_gpu_pid as TP
import test_gpu_pursuit as TU

pytestmark = pytest.mark.gpu
STRAIGHT = np.float32([[-1024, 0], [1024, 0]])
RULE = (1.875, np.inf)   # lane_half_width, horizon of the leader rule, for IDM and ACC alike


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------------- the scenes (no GPU)
def _controllers(lon_idm):
    from tactics2d_amd.controller import IDMController, PIDController
    idm = IDMController(lane_half_width=RULE[0], horizon=RULE[1]).row()
    pid = PIDController(dt=0.1, longitudinal="idm" if lon_idm else "pid").row()     # cross-track + IDM / speed PID, wheel base of the type
    pur = TU.US.ring_controller().row("acc")
    pur[UR.LANE_HALF_WIDTH], pur[UR.HORIZON] = RULE
    return idm, pid, pur


def stride_scene():
    """2 x 3: env 0 on routes 0, 31, 63 of a 64-route set, env 1 on a one-route set; participant 4 inactive"""
    many = [np.float32([[0, 4 * r], [30, 4 * r], [60, 4 * r + 3]]) for r in range(64)]
    sets = [many, [np.float32([[0, 0], [50, 0]])]]
    route_of = np.int32([0, 31, 63, 0, 0, 0])
    x = np.float32([41.0, 12.5, 47.25, 10.0, 20.0, 31.0])
    y = np.float32([1.75, 124.4, 254.0, 0.3, -0.8, 0.2])
    h = np.float32([0.1, -0.05, 0.12, 0.02, 0.0, -0.03])
    v = np.float32([5.0, 6.5, 4.0, 7.0, 3.0, 5.5])
    a = np.float32([0.2, -0.4, 0.0, 0.5, 0.1, -0.3])
    active = np.uint8([1, 1, 1, 1, 0, 1])
    return dict(n_env=2, A=3, sets=sets, set_of_env=np.int32([0, 1]), route_of=route_of, x=x, y=y, h=h, v=v, a=a, active=active,
                thr=np.float32([0.5, 0.5, 0.5, 0.25, 0.5, 0.25]), ts=np.float32([6, 6, 6, 6, 6, 6]), lon_idm=False)


def wave_scene():
    """1 x 65 in one lane heading east, 8 m apart, participant 64 between 30 and 31; participant 10 inactive"""
    n = 65
    x = np.float32(8.0 * np.arange(n))
    x[64] = 8.0 * 30 + 4.0
    rng = np.random.default_rng(65)
    y = np.float32(rng.normal(0, 0.3, n))
    h = np.float32(rng.normal(0, 0.02, n))
    v = np.float32(rng.uniform(3, 9, n))
    a = np.float32(rng.uniform(-1, 1, n))
    active = np.ones(n, np.uint8)
    active[10] = 0
    sets = [[np.float32([[-10, 0], [300, 0], [700, 1]])]]
    return dict(n_env=1, A=n, sets=sets, set_of_env=np.int32([0]), route_of=np.zeros(n, np.int32), x=x, y=y, h=h, v=v, a=a, active=active,
                thr=np.full(n, 0.25, np.float32), ts=np.float32(rng.uniform(3, 9, n)), lon_idm=True)


def references(sc, oracle):
    """what the three launches must leave behind on scene `sc`: (off-route, pid, pursuit), from the numpy references alone"""
    n_env, A = sc["n_env"], sc["A"]
    n = n_env * A
    idm, pid, pur = _controllers(sc["lon_idm"])
    x, y, h, v, a, active = (sc[k] for k in ("x", "y", "h", "v", "a", "active"))
    wb = np.full(n, TP._types()[2])
    flat, base = [], []
    for routes in sc["sets"]:
        base.append(len(flat)); flat += list(routes)
    index = np.asarray(base)[sc["set_of_env"][np.arange(n) // A]] + sc["route_of"]
    off = RR.evaluate_sets(sc["sets"], sc["set_of_env"], sc["route_of"], A, x, y, sc["thr"], active)
    z = np.zeros(n, np.float32)
    _, _, lead = oracle.idm(idm[None], np.zeros(n, np.uint8), n_env, A, x, y, h, v, active, z, z)
    idm_accel = None
    if sc["lon_idm"]:
        idm_accel = np.zeros(n)
        for i in range(n):
            j = (i // A) * A + max(int(lead[i]), 0)
            idm_accel[i] = oracle.idm_accel(idm, np.float64(v[i]), lead[i] >= 0, np.float64(x[j]) - np.float64(x[i]),
                                            np.float64(y[j]) - np.float64(y[i]), np.float64(v[j]), trig=1)
    pidw = PR.evaluate(np.repeat(pid[None], n, 0), np.ones(n, bool), np.zeros((n, 6)), x, y, h, v, active, sc["ts"],
                       *RR.pad_routes(flat, index), wb, None, None, idm_accel, lead if sc["lon_idm"] else None)
    purw = UR.evaluate(np.repeat(pur[None], n, 0), np.ones(n, bool), x, y, h, v, a, active, sc["ts"], flat, index, wb, None, lead, A)
    return off, pidw, purw, lead


def _not_vacuous(sc, off, pidw, purw, lead):
    """nobody in a flagged case; every active participant measured, acted on, and (bar the head of a platoon) led"""
    on = sc["active"] != 0
    assert (~on).sum() == 1
    assert np.isfinite(off[0][on]).all() and np.isnan(off[0][~on]).all() and off[1][on].any() and not off[1][on].all()
    assert not (pidw["events"] & (PR.NONFINITE | PR.NO_ROUTE | PR.BAD_WHEEL_BASE)).any() and np.isfinite(pidw["action"][on]).all()
    assert not (purw["events"] & (UR.NONFINITE | UR.NO_ROUTE)).any() and np.isfinite(purw["action"][on]).all()
    assert np.isnan(pidw["action"][~on]).all() and np.isnan(purw["action"][~on]).all()
    assert (pidw["segment"][on] >= 0).all() and (purw["segment"][on] >= 0).all() and (off[2][on] != 0).any()
    assert (lead[on] >= 0).any() and (purw["leader"][on] == lead[on]).all()
    if sc["A"] == 65:
        assert (lead[on] >= 0).sum() == on.sum() - 1                                 # everybody but the head of the platoon
        assert lead[30] == 64 and lead[64] == 31 and lead[9] == 11                   # across the wave boundary; past the inactive one
        assert (pidw["leader"][on] == lead[on]).all()


def _load(sc):
    from tactics2d_amd import layout as L
    idm, pid, pur = _controllers(sc["lon_idm"])
    n = sc["n_env"] * sc["A"]
    pool = TP._pool(sc["n_env"], sc["A"], sc["x"], sc["y"], sc["h"], sc["v"], sc["active"])
    pool.upload(L.F_APPLIED0, sc["a"])
    pool.set_routes(sc["sets"], sc["set_of_env"], sc["route_of"], sc["thr"])
    return pool, n, idm, pid, pur


@pytest.mark.parametrize("scene", [stride_scene, wave_scene])
def test_staging_strides_and_a_lone_lane_in_the_second_wave(torch, oracle, scene):
    from tactics2d_amd import layout as L
    sc = scene()
    off, pidw, purw, lead = references(sc, oracle)
    _not_vacuous(sc, off, pidw, purw, lead)
    pool, n, idm, pid, pur = _load(sc)
    TO._same(pool.off_route_host(), off, "off_route")
    if sc["lon_idm"]:
        pool.set_idm(idm[None], np.full(n, L.IDM_NONE, np.uint8))
    pool.set_pid(pid[None], np.zeros(n, np.uint8), sc["ts"], np.zeros(n, np.int32))
    got, rec, st = TP._run(torch, pool)
    print("pid: largest |action - pid_ref|", np.nanmax(np.abs(rec["action"] - pidw["action"])))
    TP._check(got, rec, st, pidw, None if not sc["lon_idm"] else np.zeros(n, bool), "pid")
    assert TP._same(rec["action"][:, 0], pidw["action"][:, 0])                          # (the cross-track kind: no transcendental)
    pool.set_pid(None)
    pool.set_pursuit(pur[None], np.zeros(n, np.uint8), sc["ts"])
    got, rec = TU._run(torch, pool)
    print("pursuit: largest |action - pursuit_ref|", np.nanmax(np.abs(rec["action"] - purw["action"])))
    TU._check(got, rec, purw, "pursuit")
    pool.close()


# ---------------------------------------------------------------------------------------------------- the setters
FAMILIES = ("idm", "pid", "pursuit")


def _small(make_pool=None):
    """2 x 3 on a straight route east through y = 0, nobody controlled yet"""
    rng = np.random.default_rng(23)
    x, y = np.float32(np.tile([0.0, 9.0, 19.0], 2) + rng.uniform(-1, 1, 6)), np.float32(rng.normal(0, 0.4, 6))
    h, v = np.float32(rng.normal(0, 0.05, 6)), np.float32(rng.uniform(3, 9, 6))
    pool = TP._pool(2, 3, x, y, h, v) if make_pool is None else make_pool(x, y, h, v)
    pool.set_routes([[STRAIGHT]], None, 0, 0.0)
    return pool


def _only(i, none=255):
    return np.where(np.arange(6) == i, 0, none).astype(np.uint8)


def _install(pool, family, ctrl):
    idm, pid, pur = _controllers(False)
    if family == "idm":
        pool.set_idm(idm[None], ctrl)
    elif family == "pid":
        pool.set_pid(pid[None], ctrl, 6.0)
    else:
        pool.set_pursuit(pur[None], ctrl, 6.0)


def _uninstall(pool, family):
    {"idm": lambda: pool.set_idm(None, None), "pid": lambda: pool.set_pid(None), "pursuit": lambda: pool.set_pursuit(None)}[family]()


def _launch(torch, pool, family):
    """one launch of the family from a fresh controller state -> everything it wrote, as bytes"""
    from tactics2d_amd import layout as L
    if family == "idm":
        pool.idm_actions()
        pool.sync()
        return pool.download(L.F_ACT0).tobytes() + pool.download(L.F_ACT1).tobytes() + pool.download(L.F_LEADER).tobytes()
    if family == "pid":
        pool.pid_state(np.zeros((6, L.PID_STATE_WORDS)))
        got, rec, st = TP._run(torch, pool)
        return got.tobytes() + b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in sorted(rec)) + st.tobytes()
    got, rec = TU._run(torch, pool)
    return got.tobytes() + b"".join(np.ascontiguousarray(rec[k]).tobytes() for k in sorted(rec))


def _actions(torch, pool, family):
    """the family's *_actions call alone"""
    t = torch.zeros((6, 2), dtype=torch.float32, device="cuda")
    {"idm": pool.idm_actions, "pid": lambda: pool.pid_actions(None, t.data_ptr()),
     "pursuit": lambda: pool.pursuit_actions(None, t.data_ptr())}[family]()
    pool.sync()


def _raises(code, call):
    from tactics2d_amd import _ffi
    with pytest.raises(_ffi.T2DError) as ei:
        call()
    assert ei.value.code == code


@pytest.mark.parametrize("first,second", [(a, b) for a in FAMILIES for b in FAMILIES if a != b])
def test_one_controller_per_participant_in_every_ordered_pair(torch, first, second):
    from tactics2d_amd import _ffi
    pool = _small()
    _install(pool, first, _only(1))
    before = _launch(torch, pool, first)
    _raises(_ffi.ERR_INVALID, lambda: _install(pool, second, _only(1)))
    assert _launch(torch, pool, first) == before
    _raises(_ffi.ERR_STATE, lambda: _actions(torch, pool, second))
    _install(pool, second, _only(2))                                                    # another participant: accepted
    assert _launch(torch, pool, first) == before
    pool.close()


def test_a_refused_set_idm_changes_nothing(torch):
    from tactics2d_amd import _ffi, layout as L
    idm, pid, pur = _controllers(False)
    pool = _small()
    ctrl = np.uint8([0, L.IDM_NONE, 1, 0, 1, 0])
    two = np.stack([idm, idm])
    two[1, L.IDM_DESIRED_SPEED] = 4.0
    pool.set_idm(two, ctrl)
    pool.set_pid(pid[None], _only(1), 6.0)
    before = _launch(torch, pool, "idm")
    bad = two.copy()
    bad[1, L.IDM_COMF_DECEL] = 0.0
    for rows, cid in ((bad, ctrl),                                                      # a bad row
                      (two[:1], ctrl),                                                  # ctrl_id 1 without a row
                      (two, np.uint8([0, 0, 1, 0, 1, 0]))):                             # participant 1 is PID-controlled
        _raises(_ffi.ERR_INVALID, lambda: pool.set_idm(rows, cid))
        assert _launch(torch, pool, "idm") == before
    pool.close()


def test_uninstall_frees_and_a_reinstall_gives_the_first_bits(torch):
    from tactics2d_amd import debug as D
    pool = _small(lambda x, y, h, v: _debug_pool(D, x, y, h, v))
    m0 = D.memory()
    for k, family in enumerate(FAMILIES):
        _install(pool, family, _only(k))
    first = {family: _launch(torch, pool, family) for family in FAMILIES}
    assert D.memory()[0] > m0[0]
    for family in FAMILIES:
        _uninstall(pool, family)
    assert D.memory() == m0
    for k, family in enumerate(FAMILIES):
        _install(pool, family, _only(k))
    for family in FAMILIES:
        assert _launch(torch, pool, family) == first[family], family
    pool.close()


def _debug_pool(D, x, y, h, v):
    rows, ty, _ = TP._types()
    pool = D.pool(2, 3)
    pool.set_param_table(rows)
    pool.set_status_config(max_step=100000)
    pool.reset(x, y, h, v, np.full(6, ty, np.uint8), None)
    return pool
