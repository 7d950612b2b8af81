"""A pool that is reset or reconfigured must equal a fresh one (DESIGN.md "what a reset and a re-installation guarantee").

Almost every other GPU test builds a new pool, configures it once and resets it once: device buffers from alloc_zeroed, host
bookkeeping at its defaults.  Here a pool is taken through a history H and then brought to a configuration C
(tests/reuse_scenes.py), and `observe` -- one fixed sequence: the seeded action rows, the installed controllers' launches, one
exact step, collide, the scans, off_route -- must give
  (a) bit for bit what it gives on a NEW pool that was only ever given C (every array by its bytes, NaN included; the step forms
      too; reuse_scenes.NOT_COMPARED lists what is documented to differ), and
  (b) on that fresh twin, the project's reference for the decisive output (oracle collide / lidar, pursuit_ref, pid_ref,
      route_ref), so that two pools wrong in the same way do not pass.
That the reference's answer for C differs from its answer for the configuration or state before it is asserted on the CPU, in
tests/test_reuse_scenes.py.
"""
import numpy as np
import pytest

import helpers as H
import pursuit_ref as UR
import reuse_scenes as RS
import route_ref as RR

pytestmark = pytest.mark.gpu
TOL = 1e-9   # results through the library's own transcendental functions against numpy's (tests/test_gpu_pid.py)
PER_PARTICIPANT = ("rows", "pursuit_record", "pid_record", "pid_state", "x", "y", "heading", "speed", "vx", "vy", "applied0", "applied1",
                   "flags", "ids", "leader", "off_dist", "off_verdict", "scan_all")
PER_ENV = ("env_flags", "status", "reward", "iou", "cnt_no_action", "cnt_step", "frame_ms", "record", "scan")


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


# ---------------------------------------------------------------------------------------------------- configure and observe
def uninstall(pool):
    pool.set_pursuit(None)
    pool.set_pid(None)
    pool.set_idm(None, None)


def install(pool, C):
    if C["routes"] is None:
        pool.clear_routes()
    else:
        r = C["routes"]
        pool.set_routes(r["sets"], r["set_of_env"], r["route_of"], r["thr"])
    if C["idm"] is not None:
        pool.set_idm(*C["idm"])
    if C["pid"] is not None:
        pool.set_pid(*C["pid"])
    if C["pursuit"] is not None:
        pool.set_pursuit(*C["pursuit"])
    if C["lidar"] is not None:
        pool.lidar_config(C["lidar"]["n_beams"], C["lidar"]["max_range"], C["lidar"]["include_participants"])


def reset(pool, C, env_mask=None):
    pool.reset(C["x"], C["y"], C["heading"], C["speed"], C["type_id"], C["active"], vx=C.get("vx"), vy=C.get("vy"), env_mask=env_mask)


def configure(pool, C):
    """bring a pool -- new or used -- to C"""
    uninstall(pool)
    pool.set_param_table(C["rows"])
    pool.set_static_geometry(C["static"], C["boundary"], C["boundary_valid"])
    pool.set_lane_geometry(C["lanes"])
    pool.set_target_areas(C.get("target"))
    pool.set_status_config(**C["status"])
    pool.set_integrator_variant("exact")
    reset(pool, C)
    install(pool, C)


def fresh(C):
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(C["n_env"], C["A"])
    configure(pool, C)
    return pool


def control(torch, pool, C):
    """the seeded rows through the installed PID and pursuit launches -> (the action tensor, dict of what they left)"""
    from tactics2d_amd import layout as L
    n = pool.n
    out = {}
    act = torch.as_tensor(np.ascontiguousarray(C["act"]), device="cuda").clone()
    recs = {}
    if C["pid"] is not None:
        recs["pid_record"] = torch.zeros((n, L.PID_RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
        pool.pid_actions(act.data_ptr(), act.data_ptr(), recs["pid_record"].data_ptr())
    if C["pursuit"] is not None:
        recs["pursuit_record"] = torch.zeros((n, L.PURSUIT_RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
        pool.pursuit_actions(act.data_ptr(), act.data_ptr(), recs["pursuit_record"].data_ptr())
    pool.sync()
    out["rows"] = act.cpu().numpy()
    for k, t in recs.items():
        out[k] = t.cpu().numpy()
    if C["pid"] is not None:
        out["pid_state"] = pool.pid_state()
    return act, out


def step_and_download(torch, pool, C, act, out):
    from tactics2d_amd import layout as L
    p = act.data_ptr()
    pool.bind_actions(p + 4, p, stride=2)
    pool.step(100)
    pool.collide()
    if C["lidar"] is not None:
        pool.lidar_scan()
        if C["lidar"].get("all"):
            pool.lidar_scan_all()
    pool.sync()
    pool.bind_actions(None, None)
    names = dict(x=L.F_X, y=L.F_Y, heading=L.F_HEADING, speed=L.F_SPEED, vx=L.F_VX, vy=L.F_VY, applied0=L.F_APPLIED0, applied1=L.F_APPLIED1,
                 flags=L.F_FLAGS, env_flags=L.F_ENV_FLAGS, status=L.F_STATUS, reward=L.F_REWARD, iou=L.F_IOU,
                 cnt_no_action=L.F_CNT_NO_ACTION, cnt_step=L.F_CNT_STEP, frame_ms=L.F_FRAME_MS, ids=L.F_IDS)   # test_gpu_ego._fields()
    for k, f in names.items():
        out[k] = pool.download(f)
    out["step_count"] = int(pool.step_count())
    out["record_slot"] = (out["step_count"] - 1) % L.RECORD_RING
    out["record"] = pool.download(L.F_RECORD)[out["record_slot"]]
    if C["idm"] is not None:
        out["leader"] = pool.download(L.F_LEADER)
    if C["lidar"] is not None:
        out["scan"] = pool.download(L.F_LIDAR)
        if C["lidar"].get("all"):
            out["scan_all"] = pool.lidar_all().reshape(pool.n, -1)
    if C["routes"] is not None:
        d, o = pool.off_route_host()
        out["off_dist"], out["off_verdict"] = np.asarray(d).reshape(-1), np.asarray(o).reshape(-1)
    if C["pid"] is not None:
        out["pid_state"] = pool.pid_state()
    out["form1"], out["form4"] = pool.step_form(1), pool.step_form(4)
    return out


def observe(torch, pool, C):
    act, out = control(torch, pool, C)
    return step_and_download(torch, pool, C, act, out)


def _env_slice(key, v, C, envs):
    if key in PER_PARTICIPANT:
        return v.reshape((C["n_env"], C["A"]) + v.shape[1:])[envs]
    assert key in PER_ENV, key
    return v[envs]


def same(got, want, C, what, envs=None, skip=()):
    """(a): every output by its bytes"""
    assert set(got) == set(want), (what, set(got) ^ set(want))
    for k in sorted(got):
        if k in RS.NOT_COMPARED or k in skip:
            continue
        g, w = got[k], want[k]
        if isinstance(g, str):
            assert g == w, (what, k, g, w)
            continue
        if envs is not None:
            g, w = _env_slice(k, g, C, envs), _env_slice(k, w, C, envs)
        g, w = np.ascontiguousarray(g), np.ascontiguousarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero((g.reshape(len(g), -1).view(np.uint8) != w.reshape(len(w), -1).view(np.uint8)).any(1))
            raise AssertionError(f"{what}: {k} differs in rows {bad[:8].tolist()} ({len(bad)} of {len(g)}): {g[bad[:3]]} != {w[bad[:3]]}")


def history(torch, pool, C, n_steps=RS.HISTORY_STEPS):
    for _ in range(n_steps):
        observe(torch, pool, C)


def _pursuit_record(r):
    i32 = r.view(np.int32).reshape(len(r), -1)
    return dict(leader=i32[:, 12], events=i32[:, 13].view(np.uint32), action=r[:, 7:9])


def _pid_record(r):
    i32 = r.view(np.int32).reshape(len(r), -1)
    return dict(events=i32[:, 6].view(np.uint32), action=r[:, 4:6])


# ---------------------------------------------------------------------------------------------------- (b) the anchors
def anchor_controllers(oracle, C, obs, envs=None, pid_state=None):
    """the controller rows of a launch at C's reset state against pid_ref and pursuit_ref with accel_last = 0 for everybody (the
    leader's front.accel included): cruise bit for bit, ACC and the steering within TOL"""
    st = RS.state_of(C)
    n = len(st)
    pick = np.ones(n, bool) if envs is None else np.isin(np.arange(n) // C["A"], envs)
    rows_in = C["act"]
    if C["pid"] is not None:
        want = RS.pid_want(C, st, pid_state, rows_in)
        rec = _pid_record(obs["pid_record"])
        on = pick & (C["pid"][1] != 255)
        ev = rec["events"] & ~np.uint32(4)   # (PID_RESET: the launch after an ended episode says so)
        assert (ev[on] == want["events"][on]).all(), (ev[on], want["events"][on])
        live = on & (C["active"] != 0)
        assert live.any() and np.isfinite(want["action"][live]).all()
        assert np.abs(rec["action"][live] - want["action"][live]).max() <= TOL
        rows_in = want["rows"]
    if C["pursuit"] is not None:
        want = RS.pursuit_want(oracle, C, st, np.zeros(n, np.float32), rows_in)
        rec = _pursuit_record(obs["pursuit_record"])
        cid = C["pursuit"][1]
        on = pick & (cid != 255)
        live = on & (C["active"] != 0)
        assert (rec["events"][on] == want["events"][on]).all() and (rec["leader"][on] == want["leader"][on]).all()
        assert live.any() and np.isfinite(want["action"][live]).all()
        cruise = live & ((C["pursuit"][0][np.where(cid == 255, 0, cid), UR.LON_MODE] == 0) | (want["leader"] < 0))
        assert cruise.any()
        assert (rec["action"][cruise, 1] == want["action"][cruise, 1]).all(), \
            (np.flatnonzero(rec["action"][:, 1] != want["action"][:, 1]), rec["action"][cruise, 1], want["action"][cruise, 1])
        assert np.abs(rec["action"][live] - want["action"][live]).max() <= TOL
        got = obs["rows"]
        assert (got[live].view(np.uint32) == rec["action"][live].astype(np.float32).view(np.uint32)).all()
        return want
    return None


def anchor_flags(oracle, C, obs):
    sc = dict(rows=C["rows"], n_env=C["n_env"], A=C["A"], x=obs["x"], y=obs["y"], heading=obs["heading"], type_id=C["type_id"],
              active=C["active"], static=C["static"], boundary=C["boundary"], boundary_valid=C["boundary_valid"], lanes=C["lanes"])
    flags, env_flags = H.oracle_collide(oracle, sc)
    assert np.array_equal(obs["flags"], flags), np.flatnonzero(obs["flags"] != flags)[:8]
    assert np.array_equal(obs["env_flags"], env_flags)
    return flags


def anchor_off_route(C, obs):
    r = C["routes"]
    soe = np.zeros(C["n_env"], int) if r["set_of_env"] is None else r["set_of_env"]
    thr = np.broadcast_to(np.float32(r["thr"]), (len(obs["x"]),))
    d, off, _ = RR.evaluate_sets(r["sets"], soe, r["route_of"], C["A"], obs["x"], obs["y"], thr, C["active"])
    assert (obs["off_dist"].view(np.uint32) == d.view(np.uint32)).all() and (obs["off_verdict"].astype(np.uint8) == off).all()


# ---------------------------------------------------------------------------------------------------- 1. a second full reset
def test_second_full_reset(torch, oracle):
    C1, C2 = RS.traffic(0), RS.second_reset()
    pool = fresh(C1)
    history(torch, pool, C1)
    configure(pool, C2)
    twin = fresh(C2)
    got, want = observe(torch, pool, C2), observe(torch, twin, C2)
    pool.close(); twin.close()
    same(got, want, C2, "second reset")
    anchor_controllers(oracle, C2, want)
    anchor_controllers(oracle, C2, got)      # the first launch after the reset: accel_last = 0 for every controlled participant
    anchor_flags(oracle, C2, want)
    anchor_off_route(C2, want)
    assert want["form1"] == "step"


def test_second_reset_alone_keeps_the_installation(torch, oracle):
    """t2d_reset with nothing re-installed: the controllers, routes and geometry stay; the state is the new episode's"""
    C1 = RS.traffic(0)
    C2 = dict(C1, **{k: RS.second_reset()[k] for k in RS.RESET_KEYS})
    pool = fresh(C1)
    history(torch, pool, C1)
    reset(pool, C2)
    twin = fresh(C2)
    got, want = observe(torch, pool, C2), observe(torch, twin, C2)
    pool.close(); twin.close()
    same(got, want, C2, "second reset, nothing re-installed")
    anchor_controllers(oracle, C2, got)


# ---------------------------------------------------------------------------------------------------- 2. a masked reset
def test_masked_reset(torch, oracle):
    from tactics2d_amd import layout as L
    C1 = RS.traffic(0)
    mask, Cm = RS.masked(C1, RS.second_reset())
    sel, rest = np.flatnonzero(mask), np.flatnonzero(mask == 0)
    pool, alongside = fresh(C1), fresh(C1)
    for p in (pool, alongside):
        history(torch, p, C1)
    pid_before = pool.pid_state()
    reset(pool, Cm, env_mask=mask)
    # a masked reset is not controller.reset(): the PID state of the selected envs stays
    assert (pool.pid_state() == pid_before).all() and pid_before[np.repeat(mask, C1["A"]).astype(bool)].any()
    assert (pool.download(L.F_CNT_STEP) == np.where(mask, 0, RS.HISTORY_STEPS)).all()
    twin = fresh(Cm)
    twin.pid_state(pid_before)
    got, want, undisturbed = observe(torch, pool, Cm), observe(torch, twin, Cm), observe(torch, alongside, C1)
    for p in (pool, twin, alongside):
        p.close()
    same(got, want, Cm, "masked reset: selected envs", envs=sel)
    same(got, undisturbed, Cm, "masked reset: unselected envs", envs=rest)
    anchor_controllers(oracle, Cm, got, envs=sel, pid_state=pid_before)     # pursuit's accel_last of the selected envs is 0
    anchor_flags(oracle, Cm, want)


# ---------------------------------------------------------------------------------------------------- 3. restore and auto-reset
FORMS = RS.RESTORE_FORMS
VERDICT = ("rows", "pursuit_record", "pid_record", "flags", "env_flags", "status", "reward", "applied0", "applied1", "leader", "record")
STATE = ("x", "y", "heading", "speed", "vx", "vy", "ids", "cnt_step", "frame_ms", "pid_state")


def _masked_pid_events(obs):
    o = dict(obs)
    if "pid_record" in o:
        r = o["pid_record"].copy()
        r.view(np.int32).reshape(len(r), -1)[:, 6] &= ~4   # PID_RESET
        o["pid_record"] = r
    return o


@pytest.mark.parametrize("mode", ["restore", "restore_done_only", "auto_reset"])
@pytest.mark.parametrize("form", list(FORMS))
def test_restore_and_auto_reset(torch, oracle, form, mode):
    """max_step = 4: every env exceeds its time in step 5; the ego of env 1 stands in a static square and ends in every step.
    Pursuit is launched ahead of every step.  In the first step of every new episode the pursuit rows are pursuit_ref's with
    accel_last = 0, and everything the step leaves equals a fresh pool's first step from the snapshot's poses."""
    from tactics2d_amd import layout as L
    C = RS.traffic(3, max_step=4, stuck_env=1, **FORMS[form])
    n_env, A = C["n_env"], C["A"]
    pool, twin = fresh(C), fresh(C)
    if form == "step_split":
        pool.set_split_step(True); twin.set_split_step(True)
    assert pool.step_form(1) == form and twin.step_form(1) == form
    pool.snapshot()
    if mode == "auto_reset":
        pool.set_auto_reset(True)
    first = _masked_pid_events(observe(torch, twin, C))
    twin.close()
    anchor_controllers(oracle, C, first)
    anchor_flags(oracle, C, first)
    start = RS.state_of(C)
    ended, restarts = np.zeros(n_env, bool), 0
    for k in range(7):
        new = np.flatnonzero(pool.download(L.F_CNT_STEP) == 0)
        if mode == "restore" and k > 0:
            new = new[:0]     # (nothing is put back until the one t2d_restore below)
        act, out = control(torch, pool, C)
        if len(new):
            anchor_controllers(oracle, C, out, envs=new)
        got = _masked_pid_events(step_and_download(torch, pool, C, act, out))
        done = (got["status"][:, 2] | got["status"][:, 3]) != 0
        ended |= done
        same(got, first, C, f"{form} {mode} step {k}: what a new episode's first step leaves", envs=new,
             skip=set(got) - set(VERDICT))
        kept = new if mode != "auto_reset" else new[~done[new]]
        same(got, first, C, f"{form} {mode} step {k}: state after a new episode's first step", envs=kept, skip=set(got) - set(STATE))
        if mode == "auto_reset" and done.any():
            back = np.repeat(done, A)
            for c, key in enumerate(("x", "y", "heading", "speed", "vx", "vy")):
                assert (got[key][back].view(np.uint32) == start[back, c].view(np.uint32)).all(), (form, k, key)
            assert (got["cnt_step"][done] == 0).all()
        restarts += len(new) if k > 0 else 0
        if mode == "restore_done_only" and done.any():
            m = torch.as_tensor(done.astype(np.uint8), device="cuda")
            if C["pid"] is not None:
                pool.pid_reset(m.data_ptr())          # controller.reset() of the envs the caller puts back
                pool.sync()
            pool.restore(done_only=True)
    assert ended.sum() >= 3 and ended[1]
    if mode == "restore":
        pool.restore()
        if C["pid"] is not None:
            pool.pid_reset()
        got = _masked_pid_events(observe(torch, pool, C))
        same(got, first, C, f"{form}: after t2d_restore")
        anchor_controllers(oracle, C, got)
    else:
        assert restarts >= 3 + 5     # env 1 in every step, the others after their time limit
    pool.close()


# ---------------------------------------------------------------------------------------------------- 12. controller hand-over
def test_controller_hand_over(torch, oracle):
    """the same participants (slots 0 .. 2) go IDM -> PID -> pursuit -> none, each uninstalled before the next is installed"""
    base = RS.traffic(5)
    n = base["n_env"] * base["A"]
    slot = np.arange(n) % base["A"]
    cid = np.where(slot <= 2, 0, 255).astype(np.uint8)
    idm, pid, cruise, acc = RS.controllers()
    ts = base["pursuit"][2]
    stages = [("idm", dict(idm=(idm[None], cid), pid=None, pursuit=None)), ("pid", dict(idm=None, pid=(pid[None], cid, ts), pursuit=None)),
              ("pursuit", dict(idm=None, pid=None, pursuit=(np.stack([cruise, acc]), np.where(slot <= 1, 0, np.where(slot == 2, 1, 255)).astype(np.uint8), ts))),
              ("none", dict(idm=None, pid=None, pursuit=None))]
    pool = fresh(dict(base, **stages[0][1]))
    prev = None
    for name, ctl in stages:
        C = dict(base, **ctl)
        if prev is not None:
            from tactics2d_amd import _ffi
            if name != "none":      # the one-controller rule: the new family is refused while the old one holds the participants
                with pytest.raises(_ffi.T2DError):
                    install(pool, dict(C, routes=base["routes"], lidar=None))
            uninstall(pool)
            reset(pool, C)
            install(pool, C)
        twin = fresh(C)
        got, want = observe(torch, pool, C), observe(torch, twin, C)
        twin.close()
        same(got, want, C, f"hand-over to {name}")
        anchor_controllers(oracle, C, want)
        anchor_flags(oracle, C, want)
        if name == "idm":
            z = np.zeros(n, np.float32)
            st = RS.state_of(C)
            a0, a1, lead = oracle.idm(idm[None], cid, C["n_env"], C["A"], st[:, 0], st[:, 1], st[:, 2], st[:, 3], C["active"], z, z)
            on = (cid != 255) & (C["active"] != 0)
            assert (want["leader"][on] == lead[on]).all()
        history(torch, pool, C, 3)
        prev = name
    pool.close()


# ---------------------------------------------------------------------------------------------------- 4. the geometry ladder
COUNTERS = ("cnt_step", "frame_ms", "reward", "record", "cnt_no_action", "status")   # what moves with every step without a reset


@pytest.mark.parametrize("kind", RS.GEO_KINDS)
@pytest.mark.parametrize("shape", RS.GEO_SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_geometry_ladder(torch, oracle, shape, kind):
    """LDS record -> a record more than half full -> HBM grid tier -> LDS record -> none, on one live pool.  At these shapes a
    workgroup is one wave from the start (envs_per_workgroup, t2d_geometry_host.hip); the rung that narrows the workgroups is
    test_geometry_narrows_the_workgroups."""
    ladder = RS.geometry_ladder(shape, kind)
    pool = fresh(ladder[0][1])
    for k, (stage, C) in enumerate(ladder):
        if k:
            configure(pool, C)
        twin = fresh(C)
        got, want = observe(torch, pool, C), observe(torch, twin, C)
        twin.close()
        same(got, want, C, f"{kind} {stage}")
        flags = anchor_flags(oracle, C, want)
        assert want["form1"] == ("unfused" if stage == "big" else "step"), (stage, want["form1"])
        assert (want["x"] == C["x"]).all() and (want["y"] == C["y"]).all()                  # (parked: the positions are the reset's)
        if stage == "big" and kind != "static":
            assert flags[1] & 8                                                             # 5 km outside the grid: off-lane
        history(torch, pool, C, 2)
    pool.close()


def test_geometry_narrows_the_workgroups(torch, oracle):
    """2100 x 8: two waves per workgroup (16 envs) while the record allows it.  G_mid fits the 32 KiB record only at 8 envs per
    workgroup: t2d_set_*_geometry halves the workgroups (rebuild_geo), the launch shape changes, and G_small widens them again."""
    ladder = RS.narrowing_ladder()
    pool = fresh(ladder[0][1])
    n_env = ladder[0][1]["n_env"]
    for k, (stage, C) in enumerate(ladder):
        if k:
            configure(pool, C)
        twin = fresh(C)
        got, want = observe(torch, pool, C), observe(torch, twin, C)
        bytes_per_launch = twin.geometry_bytes_per_launch()
        assert pool.geometry_bytes_per_launch() == bytes_per_launch
        twin.close()
        same(got, want, C, f"narrowing {stage}")
        anchor_flags(oracle, C, want)
        assert want["form1"] == "step"
        if stage == "mid":      # more records of at most 32 KiB than there are 16-env workgroups: the workgroups are narrower
            assert bytes_per_launch > (n_env + 15) // 16 * 32768, bytes_per_launch
        history(torch, pool, C, 1)
    pool.close()


# ---------------------------------------------------------------------------------------------------- 5. the parameter table
@pytest.mark.parametrize("name", ["circle_row", "drift_row", "long_vehicles"])
def test_parameter_table_replaced_then_reset(torch, oracle, name):
    ladder = RS.table_ladders()[name]
    pool = fresh(ladder[0][1])
    for k, (stage, C, form) in enumerate(ladder):
        if k:
            configure(pool, C)
        twin = fresh(C)
        got, want = observe(torch, pool, C), observe(torch, twin, C)
        twin.close()
        same(got, want, C, f"{name}: {stage}")
        assert want["form1"] == form, (name, stage, want["form1"])
        anchor_flags(oracle, C, want)
        if C["pursuit"] is not None:
            anchor_controllers(oracle, C, got)
        history(torch, pool, C, 2)
    pool.close()


# ---------------------------------------------------------------------------------------------------- 6. the lidar
def _anchor_scans(oracle, C, obs):
    import test_lidar_all as TLA
    l = C["lidar"]
    want = RS.lidar_want(oracle, C, obs["x"], obs["y"], obs["heading"])
    assert np.array_equal(obs["scan"].view(np.uint32), want.view(np.uint32)), int((obs["scan"].view(np.uint32) != want.view(np.uint32)).sum())
    every = TLA.stacked_oracle(oracle, C["rows"], C["n_env"], C["A"], obs["x"], obs["y"], obs["heading"], C["type_id"], C["active"], C["static"],
                               l["include_participants"], l["n_beams"], l["max_range"])
    on = C["active"] != 0
    got = obs["scan_all"].reshape(every.shape)
    assert np.array_equal(got.view(np.uint32).reshape(len(on), -1)[on], every.view(np.uint32).reshape(len(on), -1)[on])
    assert np.isinf(got.reshape(len(on), -1)[~on]).all()


def test_lidar_reconfigured_on_a_live_pool(torch, oracle):
    """only the sensor's configuration or the statics change between the rungs -- no reset: the counters move on and are left out;
    the last rung is followed by a reset, after which everything is compared"""
    ladder = RS.lidar_ladder()
    pool = fresh(ladder[0][1])
    prev = ladder[0][1]
    for k, (stage, C) in enumerate(ladder):
        if C["lidar"] != prev["lidar"]:
            pool.lidar_config(C["lidar"]["n_beams"], C["lidar"]["max_range"], C["lidar"]["include_participants"])
        if C["static"] is not prev["static"]:
            pool.set_static_geometry(C["static"], C["boundary"], C["boundary_valid"])
        twin = fresh(C)
        got, want = observe(torch, pool, C), observe(torch, twin, C)
        twin.close()
        same(got, want, C, f"lidar: {stage}", skip=COUNTERS)
        _anchor_scans(oracle, C, want)
        anchor_flags(oracle, C, want)
        prev = C
    reset(pool, C)
    twin = fresh(C)
    same(observe(torch, pool, C), observe(torch, twin, C), C, "lidar: after a reset")
    twin.close(); pool.close()


# ---------------------------------------------------------------------------------------------------- 8. the routes
def test_routes_replaced_on_a_live_pool(torch, oracle):
    from tactics2d_amd import _ffi
    ladder = RS.route_ladder()
    pool = fresh(ladder[0][1])
    for k, (stage, C) in enumerate(ladder):
        if k:
            history(torch, pool, ladder[k - 1][1], 2)
            r = C["routes"]
            if stage == "assignment":
                pool.set_route_assignment(r["route_of"], None)
            else:
                pool.set_routes(r["sets"], r["set_of_env"], r["route_of"], r["thr"])
            reset(pool, C)
        twin = fresh(C)
        got, want = observe(torch, pool, C), observe(torch, twin, C)
        twin.close()
        same(got, want, C, f"routes: {stage}")
        anchor_off_route(C, want)
        anchor_controllers(oracle, C, want)
    # routes gone under installed PID / pursuit rows that steer by them: the launches are refused, and work again once routes are back
    pool.clear_routes()
    act = torch.zeros((pool.n, 2), dtype=torch.float32, device="cuda")
    for call in (pool.pid_actions, pool.pursuit_actions):
        with pytest.raises(_ffi.T2DError) as ei:
            call(None, act.data_ptr())
        assert ei.value.code == _ffi.ERR_STATE
    C = ladder[0][1]
    r = C["routes"]
    pool.set_routes(r["sets"], r["set_of_env"], r["route_of"], r["thr"])
    reset(pool, C)
    twin = fresh(C)
    same(observe(torch, pool, C), observe(torch, twin, C), C, "routes: back after clear_routes")
    twin.close(); pool.close()


# ---------------------------------------------------------------------------------------------------- 11. the actions
def _plain_step(pool, C):
    from tactics2d_amd import layout as L
    pool.step(100)
    pool.sync()
    return {k: pool.download(f) for k, f in dict(x=L.F_X, y=L.F_Y, heading=L.F_HEADING, speed=L.F_SPEED, vx=L.F_VX, vy=L.F_VY, applied0=L.F_APPLIED0,
                                                applied1=L.F_APPLIED1, flags=L.F_FLAGS, env_flags=L.F_ENV_FLAGS, status=L.F_STATUS,
                                                reward=L.F_REWARD, cnt_step=L.F_CNT_STEP).items()}


def test_action_bindings_replaced(torch):
    """bound to T1 -> bound to T2 at stride 2 -> unbound (the pool's own fields): after each change and a reset, a step equals a
    fresh pool's that was only ever given that source"""
    base = RS.traffic(13)
    C = dict(base, idm=None, pid=None, pursuit=None)
    n = C["n_env"] * C["A"]
    rng = np.random.default_rng(2)
    acts = [rng.uniform(-2, 2, (n, 2)).astype(np.float32) for _ in range(3)]     # columns (accel, steering)
    T1 = [torch.as_tensor(np.ascontiguousarray(acts[0][:, c]), device="cuda") for c in range(2)]
    T2 = torch.as_tensor(acts[1], device="cuda")

    def source(pool, k):
        if k == 0:
            pool.bind_actions(T1[0].data_ptr(), T1[1].data_ptr())
        elif k == 1:
            pool.bind_actions(T2.data_ptr(), T2.data_ptr() + 4, stride=2, extent=2 * n)
        else:
            pool.bind_actions(None, None)
            pool.set_actions(acts[2][:, 0], acts[2][:, 1])

    pool = fresh(C)
    outs = []
    for k in range(3):
        source(pool, k)
        reset(pool, C)
        got = _plain_step(pool, C)
        pool.step(100)              # (history under this source)
        twin = fresh(C)
        source(twin, k)
        want = _plain_step(twin, C)
        twin.close()
        for key in got:
            assert got[key].tobytes() == want[key].tobytes(), (k, key)
        outs.append(want)
    pool.close()
    assert (outs[0]["applied0"] != outs[1]["applied0"]).mean() > 0.5 and (outs[1]["applied0"] != outs[2]["applied0"]).mean() > 0.5


def test_step_n_with_an_action_ring_on_a_grid_tier_pool(torch):
    """a pool that went LDS record -> HBM grid tier: step_n(3) over a ring of three action sets (launch by launch: "unfused")
    against three single steps of a fresh pool"""
    ladder = dict((s, C) for s, C in RS.geometry_ladder(RS.WIDE, "full")[:3])
    small, C = ladder["small"], ladder["big"]
    n = C["n_env"] * C["A"]
    rng = np.random.default_rng(4)
    ring0 = torch.as_tensor(rng.uniform(-2, 2, (3, n)).astype(np.float32), device="cuda")
    ring1 = torch.as_tensor(rng.normal(0, 0.05, (3, n)).astype(np.float32), device="cuda")
    pool = fresh(small)
    history(torch, pool, small, 2)
    configure(pool, C)
    assert pool.step_form(3) == "unfused"
    pool.bind_actions(ring0.data_ptr(), ring1.data_ptr(), extent=3 * n)
    pool.step_n(3, 100, n)
    twin = fresh(C)
    for k in range(3):
        twin.bind_actions(ring0[k].data_ptr(), ring1[k].data_ptr())
        want = _plain_step(twin, C)
    from tactics2d_amd import layout as L
    pool.sync()
    got = {k: pool.download(f) for k, f in dict(x=L.F_X, y=L.F_Y, heading=L.F_HEADING, speed=L.F_SPEED, vx=L.F_VX, vy=L.F_VY, applied0=L.F_APPLIED0,
                                               applied1=L.F_APPLIED1, flags=L.F_FLAGS, env_flags=L.F_ENV_FLAGS, status=L.F_STATUS,
                                               reward=L.F_REWARD, cnt_step=L.F_CNT_STEP).items()}
    for p in (pool, twin):
        p.bind_actions(None, None)
        p.close()
    for key in got:
        assert got[key].tobytes() == want[key].tobytes(), key
    assert (got["x"] != C["x"]).mean() > 0.5 and (got["cnt_step"] == 3).all()


# ---------------------------------------------------------------------------------------------------- 10. the status configuration
def test_status_config_replaced_on_a_live_episode(torch, oracle):
    """three steps in, the ego moves and the checks are toggled, then max_step drops below cnt_step: the statuses, rewards and
    counters of the steps that follow equal the oracle's status chain started from the downloaded counters, and a fresh pool's
    that was given the downloaded state and the new configuration"""
    from tactics2d_amd import layout as L
    C = RS.status_scene()
    n_env, A = C["n_env"], C["A"]
    pool = fresh(C)
    history(torch, pool, C, 3)
    for cfg in RS.STATUS_STAGES:
        pool.set_status_config(**cfg)
        now = {k: pool.download(f) for k, f in dict(x=L.F_X, y=L.F_Y, heading=L.F_HEADING, speed=L.F_SPEED, vx=L.F_VX, vy=L.F_VY).items()}
        cnt, frame = pool.download(L.F_CNT_STEP).copy(), pool.download(L.F_FRAME_MS).copy()
        C1 = dict(C, status=cfg, **now)
        twin = fresh(C1)
        twin.upload(L.F_CNT_STEP, cnt)
        twin.upload(L.F_FRAME_MS, frame)
        cfg_o = oracle.make_config(**cfg)
        for k in range(3):
            got, want = observe(torch, pool, C1), observe(torch, twin, C1)
            same(got, want, C1, f"status {cfg}: step {k}")
            flags = anchor_flags(oracle, C1, got)
            st, rw = oracle.status(cfg_o, n_env, A, flags, 100, cnt, frame)
            assert np.array_equal(got["status"], st), (cfg, k, got["status"].tolist(), st.tolist())
            assert np.abs(got["reward"].astype(np.float64) - rw).max() <= 2e-6      # (one fp32 ulp of the time-penalty table)
            assert np.array_equal(got["cnt_step"], cnt) and np.array_equal(got["frame_ms"], frame)
        twin.close()
    pool.close()


# ---------------------------------------------------------------------------------------------------- 7. the camera
def test_camera_reconfigured_on_a_live_pool():
    """one pool through every rung of reuse_scenes.camera_ladder: a new size, the first size again, another scene's geometry and
    participants (loaded into the live pool), another palette and style.  Each render equals a fresh pool's bit for bit, and
    camera_ref's under test_gpu_camera.check_image's margin rule"""
    import test_gpu_camera as TC
    from tactics2d_amd import sensor
    from tactics2d_amd.pool import ParticipantPool
    ladder = RS.camera_ladder()
    pool = ParticipantPool(5, 8)
    loaded = None
    for stage, sc, size, cls_of, pal in ladder:
        if sc is not loaded:
            sc.load(pool)
            loaded = sc
        twin = TC.scene_pool(sc)
        imgs = []
        for p in (pool, twin):
            cam = sensor.BEVCamera(p, RS.CAMERA_RANGE, size, 0, True, RS.camera_layers(sc))
            cam.set_palette(pal)
            cam.set_style(cls_of)
            img, _ = TC.check_scene(sc, p, cam, range(sc.n_env), stage, class_of_type=cls_of)
            imgs.append(img)
        twin.close()
        for key in ("image_class", "image"):
            assert imgs[0][key].shape == imgs[1][key].shape and imgs[0][key].tobytes() == imgs[1][key].tobytes(), (stage, key)
        assert imgs[0]["image_class"].shape == (5, size[1], size[0])
        want_cls, want_rgb = RS.camera_want(sc, size, cls_of, pal)       # (what the CPU floors were computed on)
        assert (imgs[1]["image_class"] != want_cls).mean() <= TC.MAX_EXCLUDED
    pool.close()


# ---------------------------------------------------------------------------------------------------- 9. the tracks
def _drive(oracle, pool, sc, prog, n_steps=RS.TRACK_STEPS):
    """n steps of the scripted driver with one track_progress each, held to track_ref's Progress where one is given; returns
    everything the last step left"""
    import track_ref as R
    import track_scenes as TS
    from tactics2d_amd import layout as L
    drv, tid = TS.Driver(sc), np.zeros(sc.n_env, np.uint8)
    get = lambda *fs: tuple(pool.download(f) for f in fs)
    for _ in range(n_steps):
        pool.set_actions(*drv.actions(*get(L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED)))
        pool.step(100)
        x, y, h, pst, flags, cnt = get(L.F_X, L.F_Y, L.F_HEADING, L.F_STATUS, L.F_FLAGS, L.F_CNT_STEP)
        pool.track_progress()
        ts = pool.track_state()
        if prog is not None:
            prog.step(*R.boxes(oracle, sc.rows, tid, x, y, h), pst, flags, cnt)
            _track_equals(ts, prog, "progress")
    out = dict(ts)
    out.update(zip(("x", "y", "heading", "speed", "status_field", "flags", "cnt_step", "reward_field"),
                   get(L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_STATUS, L.F_FLAGS, L.F_CNT_STEP, L.F_REWARD)))
    return out


def _track_equals(ts, prog, what):
    for name, got, want in (("tile_visiting", ts["tile_visiting"], prog.visiting.astype(np.int32)), ("num_visited", ts["num_visited"], prog.num_visited),
                            ("mask", ts["mask"], prog.mask()), ("status", ts["status"], prog.status),
                            ("reward bits", ts["reward"].view(np.uint32), prog.reward.view(np.uint32))):
        assert np.array_equal(got, want), (what, name, got, want)


def _same_dicts(got, want, what):
    assert set(got) == set(want)
    for k in got:
        assert np.ascontiguousarray(got[k]).tobytes() == np.ascontiguousarray(want[k]).tobytes(), (what, k, got[k], want[k])


def test_tracks_replaced_on_a_live_pool(oracle):
    """set_tracks -> set_tracks (other rings) -> set_tracks_generated -> set_tracks, a masked and an unmasked track_reset in
    between, on one pool: after every rung the driven progress equals a fresh pool's bit for bit and track_ref's"""
    import dataclasses
    import test_gpu_camera as TC
    import track_ref as R
    from tactics2d_amd import sensor
    from tactics2d_amd.pool import ParticipantPool
    (_, first), (_, other), (_, again) = RS.track_ladder()
    pool = ParticipantPool(5, 1)

    def rung(sc, what):
        sc.load(pool)
        twin = ParticipantPool(5, 1)
        sc.load(twin)
        got = _drive(oracle, pool, sc, None)
        want = _drive(oracle, twin, sc, sc.progress(R.RULE_FORWARD, 8))
        imgs = []
        for p in (pool, twin):       # the camera's track layer draws the tiles installed now, not the ones before
            cam = sensor.BEVCamera(p, (30, 30, 50, 10), (64, 48), 0, True, ("tracks", "participants", "arrows"))
            imgs.append(TC.check_scene(TC._RaceAsScene(sc), p, cam, range(5), what, tracks=sc.tracks, set_of_env=sc.set_of_env)[0])
        twin.close()
        _same_dicts(got, want, what)
        _same_dicts(imgs[0], imgs[1], what + ": camera")
        return want

    a = rung(first, "two rings")
    sel = np.arange(5) % 2 == 0
    prog = first.progress(R.RULE_FORWARD, 8)
    prog.upload(a["tile_visiting"], _unpack(a["mask"], first))
    pool.track_reset(sel); prog.reset(sel)
    ts = pool.track_state()
    assert (ts["tile_visiting"][sel] == 0).all() and (ts["num_visited"][sel] == 1).all()
    assert np.array_equal(ts["tile_visiting"][~sel], a["tile_visiting"][~sel]) and np.array_equal(ts["mask"], prog.mask())
    b = rung(other, "three other rings")
    assert (b["num_tile"] != a["num_tile"]).all()
    pool.track_reset()
    assert (pool.track_state()["tile_visiting"] == 0).all() and (pool.track_state()["num_visited"] == 1).all()
    # device-generated tracks, every env its own: start poses, boundaries and snapshot come from the call
    twin = ParticipantPool(5, 1)
    other.load(twin)
    tiles = []
    for p in (pool, twin):
        p.set_tracks_generated(5, 7)
        p.restore()                      # a new episode from the generated start poses: state and counters
        tiles.append(p.generated_tracks()["tiles"])
    assert len(tiles[0]) == 5 and all(np.array_equal(u, w) for u, w in zip(*tiles))
    gen = dataclasses.replace(other, tracks=tiles[0], set_of_env=np.arange(5, dtype=np.int32))
    got = _drive(oracle, pool, gen, None)
    want = _drive(oracle, twin, gen, R.Progress(gen.tracks, gen.set_of_env, R.RULE_FORWARD, 8))
    twin.close()
    _same_dicts(got, want, "generated tracks")
    c = rung(again, "two rings again")
    _same_dicts(c, a, "the first rung again")
    pool.close()


def _unpack(mask, sc):
    from tactics2d_amd.pool import unpack_track_mask
    return unpack_track_mask(mask, max(len(t) for t in sc.tracks))


# ---------------------------------------------------------------------------------------------------- 10b. the target areas
def test_target_areas_replaced_and_removed_on_a_live_episode(torch, oracle):
    """three steps in, target areas are installed, replaced and removed: the IoU and shaping state starts again from the poses
    of that moment.  The next three steps equal the oracle's status chain (status_ex on a new EpisodeState) and a fresh pool's that
    was given the downloaded state, the counters and the same targets"""
    from tactics2d_amd import layout as L
    C = RS.status_scene()
    n_env, A = C["n_env"], C["A"]
    pool = fresh(C)
    history(torch, pool, C, 3)
    pool.set_status_config(**RS.TARGET_STATUS)
    cfg_o = oracle.make_config(**RS.TARGET_STATUS)
    for stage, target in RS.target_stages(C):
        pool.set_target_areas(target)
        now = {k: pool.download(f) for k, f in dict(x=L.F_X, y=L.F_Y, heading=L.F_HEADING, speed=L.F_SPEED, vx=L.F_VX, vy=L.F_VY).items()}
        cnt, frame = pool.download(L.F_CNT_STEP).copy(), pool.download(L.F_FRAME_MS).copy()
        C1 = dict(C, status=RS.TARGET_STATUS, target=target, **now)
        twin = fresh(C1)
        twin.upload(L.F_CNT_STEP, cnt)
        twin.upload(L.F_FRAME_MS, frame)
        start = np.stack([now["x"][3::A], now["y"][3::A]], 1)
        ep = oracle.EpisodeState(n_env, target, None, start) if target is not None else oracle.EpisodeState(n_env)
        for k in range(3):
            got, want = observe(torch, pool, C1), observe(torch, twin, C1)
            same(got, want, C1, f"targets, {stage}: step {k}")
            flags = anchor_flags(oracle, C1, got)
            st, rw, _ = oracle.status_ex(cfg_o, A, flags, 100, cnt, frame, C["rows"], got["x"], got["y"], got["heading"], C["type_id"], ep)
            assert np.array_equal(got["status"], st), (stage, k, got["status"].tolist(), st.tolist())
            assert np.abs(got["reward"].astype(np.float64) - rw).max() <= 2e-6, (stage, k, got["reward"], rw)
            assert np.array_equal(got["cnt_step"], cnt) and np.array_equal(got["frame_ms"], frame)
        twin.close()
    pool.close()


# ---------------------------------------------------------------------------------------------------- 6b. the planner's lidar gate
def test_rs_plan_is_refused_after_a_changed_range_and_plans_again_after_rs_config(torch):
    from tactics2d_amd import _ffi
    from tactics2d_amd.planner import RSPlanner, rs_params
    ladder = RS.lidar_ladder()
    C = ladder[3][1]                                   # 360 beams / 20 m, participants as obstacles, the ring statics
    target, heading = RS.rs_targets(C)
    pool = fresh(ladder[0][1])
    history(torch, pool, ladder[0][1], 2)
    configure(pool, C)

    def plan(p, lidar_range):
        p.set_target_areas(target)
        p.set_target_headings(heading)
        p.rs_config(**rs_params("medium_car", lidar_range=lidar_range, steer_hi=0.524))
        p.lidar_scan()
        p.rs_plan()
        p.sync()
        return {k: v.cpu().numpy().copy() for k, v in p.rs_plan_views().items()}

    first = plan(pool, 20.0)
    pool.lidar_config(360, 12.0, True)                 # the range changed behind the planner's back
    with pytest.raises(_ffi.T2DError) as ei:
        pool.rs_plan()
    assert ei.value.code == _ffi.ERR_STATE
    C12 = dict(C, lidar=dict(C["lidar"], max_range=12.0))
    got = plan(pool, 12.0)
    twin = fresh(C12)
    want = plan(twin, 12.0)
    twin.close(); pool.close()
    assert set(got) == set(want)
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), k
    assert (first["status"] != 0).any() and any(first[k].tobytes() != got[k].tobytes() for k in got)    # (0: no target)


# ---------------------------------------------------------------------------------------------------- 8b. the kinds of routes
# one step past the last recorded state: 3 - 9 m/s for 0.1 s leaves the cars 0.3 - 0.9 m beyond the end of their own trace
TRACE_THRESHOLD = 0.6


def test_route_kinds_switched_on_a_live_pool(torch, oracle):
    """CSR sets -> trace routes of a device trajectory (PID and pursuit are refused against them) -> CSR sets again; then route
    sets that a curve_routes launch has written into on the device -> set_routes: the written buffer is replaced by the host's"""
    import curve_ref as CR
    from route_writers import placeholder
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.history import DeviceTrajectory
    from tactics2d_amd.interpolator import Dubins, pack_words
    C = RS.route_ladder()[0][1]
    n_env, A, n = C["n_env"], C["A"], C["n_env"] * C["A"]
    pool = fresh(C)
    history(torch, pool, C, 2)
    reset(pool, C)
    twin = fresh(C)

    def traced(p):
        """four recorded states, a step between them; the pool's routes become the traces -> (trajectory, recorded xy, off_route)"""
        traj, xy = DeviceTrajectory(p, 0, capacity=8), []
        for k in range(4):
            traj.record(p, 100 * k)
            xy.append(np.stack([p.download(L.F_X), p.download(L.F_Y)], 1))
            observe(torch, p, C)
        p.set_routes_from(traj, threshold=TRACE_THRESHOLD)
        d, o = p.off_route_host()
        return traj, np.stack(xy), (np.asarray(d).reshape(-1).copy(), np.asarray(o).reshape(-1).astype(np.uint8))

    tr_pool, xy, got = traced(pool)
    tr_twin, xy_twin, want = traced(twin)
    assert np.array_equal(xy, xy_twin) and got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1])
    x, y = pool.download(L.F_X), pool.download(L.F_Y)
    slot = np.zeros(n, np.int32)
    d, off, _ = RR.evaluate_traces(xy, slot, slot + 3, np.arange(n_env), np.arange(n) % A, A, x, y, np.full(n, TRACE_THRESHOLD, np.float32), C["active"])
    assert (want[0].view(np.uint32) == d.view(np.uint32)).all() and np.array_equal(want[1], off) and off.any() and not off[C["active"] != 0].all()
    act = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    for call in (pool.pid_actions, pool.pursuit_actions):         # route sets are what the controllers follow
        with pytest.raises(_ffi.T2DError) as ei:
            call(None, act.data_ptr())
        assert ei.value.code == _ffi.ERR_STATE
    r = C["routes"]
    pool.set_routes(r["sets"], r["set_of_env"], r["route_of"], r["thr"])
    reset(pool, C)
    for p, t in ((twin, tr_twin),):
        p.clear_routes(); t.close(); p.close()
    tr_pool.close()
    twin = fresh(C)
    got, want = observe(torch, pool, C), observe(torch, twin, C)
    twin.close()
    same(got, want, C, "route sets after trace routes")
    anchor_off_route(C, want)
    anchor_controllers(oracle, C, want)

    # every env its own set of one 96-vertex route, written into by a launch
    own = dict(C, routes=dict(sets=[[placeholder(96, e, 0.0)] for e in range(n_env)], set_of_env=np.arange(n_env), route_of=np.zeros(n, np.int32), thr=0.5))
    configure(pool, own)
    before = pool.route_vertices().cpu().numpy().copy()
    rng = np.random.default_rng(6)
    start = np.concatenate([rng.uniform(-10, 10, (n_env, 2)), rng.uniform(-3, 3, (n_env, 1))], 1)
    goal = np.concatenate([start[:, :2] + rng.uniform(8, 20, (n_env, 2)), rng.uniform(-3, 3, (n_env, 1))], 1)
    path = Dubins(4.0, "standard").get_path(start[:, :2], start[:, 2], goal[:, :2], goal[:, 2])
    pad = torch.zeros((n_env, 2), dtype=torch.float64, device="cuda")
    words = pack_words(torch.cat([path.segments, pad], 1), torch.cat([path.steer, pad.to(torch.int8)], 1), path.n_seg)
    count = pool.curve_routes(words, torch.as_tensor(start, device="cuda"), 4.0, 0.5, "dubins", 0)
    pool.sync()
    written = pool.route_vertices().cpu().numpy()
    assert (count.cpu().numpy() > 0).all() and (written != before).reshape(n_env, -1).any(1).all()
    for name, Cn in (("the same sets uploaded again", own), ("other sets", C)):
        rr = Cn["routes"]
        pool.set_routes(rr["sets"], rr["set_of_env"], rr["route_of"], rr["thr"])
        reset(pool, Cn)
        if Cn is own:
            assert np.array_equal(pool.route_vertices().cpu().numpy(), before)
        twin = fresh(Cn)
        got, want = observe(torch, pool, Cn), observe(torch, twin, Cn)
        twin.close()
        same(got, want, Cn, f"set_routes after curve_routes: {name}")
        anchor_off_route(Cn, want)
    pool.close()
