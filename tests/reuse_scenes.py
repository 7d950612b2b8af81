"""Configurations for the pool-reuse tests (tests/test_reuse_scenes.py on the CPU, tests/test_gpu_reuse.py on the device): what a
pool is brought to after some history, as plain dicts, and the references' answers for them.  No GPU call is made here.

A configuration C is a dict:
    n_env, A, rows (parameter table), x / y / heading / speed / type_id / active (the reset), static / lanes / boundary /
    boundary_valid (geometry; None = none), status (t2d_set_status_config keywords), routes (None or dict(sets, set_of_env, route_of,
    thr)), idm / pid / pursuit (None or (rows, ctrl_id[, target_speed])), lidar (None or dict(n_beams, max_range,
    include_participants, all)), act float32 [N, 2] = the seeded (steering, accel) rows of observe().

Shapes: 5 envs x 8 participants (N = 40: less than one wave) by default; 37 x 3 (N = 111: a 64-participant segment spans ~21 envs)
where geometry is concerned.
"""
import numpy as np

import helpers as H
import pid_ref as PR
import pursuit_ref as UR
import route_ref as RR

F32 = np.float32
STRAIGHT = np.float32([[-1024, 0], [1024, 0]])
SHAPE = (5, 8)
WIDE = (37, 3)
HISTORY_STEPS = 6
MASKED = (0, 3)          # the envs a masked reset selects
# observe() outputs that are documented to differ between a pool with a history and a fresh one, and are left out of the
# fresh-twin comparison: the step counter (t2d_step_count counts launches since t2d_create), the slot of the record ring the
# step wrote (step_count % T2D_RECORD_RING: the slot's CONTENT is compared), and the profile counters.
NOT_COMPARED = ("step_count", "record_slot", "profile")


def kin_types():
    """(rows, the ids of two kinematic vehicle types, lf + lr per row)"""
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import full_type_table
    rows, names = full_type_table()
    kin = [k for k, nm in enumerate(names) if nm.endswith(":kin")]
    return rows, kin[:2], rows[:, L.P_LF] + rows[:, L.P_LR]


def controllers():
    """(idm row, pid row, cruise row, acc row) at the step's 0.1 s"""
    from tactics2d_amd.controller import IDMController, PIDController, PurePursuitController
    c = PurePursuitController(min_pre_aiming_distance=5.0)
    c._longitudinal_control.configure(delta_t=0.1)
    return IDMController().row(), PIDController(dt=0.1).row(), c.row("cruise"), c.row("acc")


def _seeded_actions(rng, n, accel=(-3.0, 2.0)):
    return np.stack([rng.normal(0, 0.02, n), rng.uniform(*accel, n)], 1).astype(F32)


def drift_row():
    from tactics2d_amd.physics import SingleTrackDrift
    return SingleTrackDrift(lf=1.262, lr=1.375, mass=1620.0, mass_height=0.7245, steer_range=(-0.524, 0.524),
                            speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)).param_row()


ROAD = np.float32([[-1100, -30], [1100, -30], [1100, 30], [-1100, 30]])   # one lane polygon under every platoon


def traffic(seed=0, shape=SHAPE, type_pick=0, inactive=1, max_step=100000, table="full", stuck_env=None, road=False, idm_on=True):
    """Platoons on a straight route east through y = 0: per env the participants 12 m apart in shuffled order, 3 - 9 m/s, a target
    speed 3 - 5 m/s off their own.  Slot a of every env: 0, 1, 2 cruise + pure pursuit; 3, 4 ACC + pure pursuit; 5 PID; 6 IDM; 7
    and up the seeded row.  `inactive` participants per env are off (never slot 0: the ego).  table: "full" (the 25 rows of
    full_type_table), "boxes" (its two kinematic rows in use alone: what the single-ego kernel asks for) or "drift" (full + a
    SingleTrackDrift row nobody has: the step goes launch by launch).  stuck_env: the ego of that env stands inside a static
    square (a collision in every step).  road: ROAD as every env's lane geometry."""
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    rng = np.random.default_rng([seed, n_env, A])
    rows, kin, wb_all = kin_types()
    if table == "boxes":
        rows, wb_all, kin = rows[kin], wb_all[kin], [0, 1]
    elif table == "drift":
        rows = np.concatenate([rows, drift_row()[None, :rows.shape[1]]])
        wb_all = np.concatenate([wb_all, [0.0]])
    order = np.stack([rng.permutation(A) for _ in range(n_env)])
    x = (order * 12.0 + rng.uniform(-1, 1, (n_env, A))).reshape(n)
    v = rng.uniform(3, 9, n)
    ts = np.where(rng.random(n) < 0.5, v + rng.uniform(3, 5, n), np.maximum(v - rng.uniform(3, 5, n), 0.0))
    active = np.ones((n_env, A), np.uint8)
    for e in range(n_env if inactive else 0):
        active[e, 1 + rng.choice(A - 1, inactive, replace=False)] = 0
    slot = np.arange(n) % A
    idm, pid, cruise, acc = controllers()
    none = np.full(n, 255, np.uint8)
    x, y = F32(x), F32(rng.normal(0, 0.3, n))
    type_id = np.where(rng.random(n) < 0.5, kin[type_pick], kin[1 - type_pick]).astype(np.uint8)
    static = None
    if stuck_env is not None:
        i = stuck_env * A
        sq = np.float32([[-3, -3], [3, -3], [3, 3], [-3, 3]]) + np.float32([x[i], y[i]])
        static = H.to_csr([[sq] if e == stuck_env else [] for e in range(n_env)])
    C = dict(n_env=n_env, A=A, rows=rows, x=x, y=y, heading=F32(rng.normal(0, 0.03, n)), speed=F32(v),
             type_id=type_id, active=active.reshape(n), wb=wb_all[type_id],
             static=static, lanes=H.to_csr([[ROAD]] * n_env) if road else None, boundary=None, boundary_valid=None,
             status=dict(max_step=max_step),
             routes=dict(sets=[[STRAIGHT]], set_of_env=None, route_of=np.zeros(n, np.int32), thr=0.5),
             idm=(idm[None], np.where(slot == 6, 0, none).astype(np.uint8)) if idm_on and A > 6 else None,
             pid=(pid[None], np.where(slot == 5, 0, none).astype(np.uint8), F32(ts)) if A > 5 else None,
             pursuit=(np.stack([cruise, acc]), np.where(slot <= 2, 0, np.where(slot <= 4, 1, none)).astype(np.uint8), F32(ts)),
             lidar=None, act=_seeded_actions(rng, n))
    return C


# the traffic() keywords that bring a pool to each one-step form of the step kernel (t2d_step_form(1)): A = 1 and boxes only for the
# single-ego kernel, A = 64 with statics and lanes (and t2d_set_split_step) for step_split, a drift row for launch by launch
RESTORE_FORMS = {"step": dict(shape=SHAPE), "unfused": dict(shape=SHAPE, table="drift"), "ego": dict(shape=(5, 1), table="boxes", inactive=0),
                 "step_split": dict(shape=(5, 64), road=True, idm_on=False)}


def state_of(C):
    """float32 [N, 6] x, y, heading, speed, vx, vy of the reset (t2d_reset: v cos / v sin of the fp64 heading)"""
    h, v = C["heading"].astype(np.float64), C["speed"].astype(np.float64)
    return np.stack([C["x"], C["y"], C["heading"], C["speed"], v * np.cos(h), v * np.sin(h)], 1).astype(F32)


def leaders(O, C, st, half_width=1.875, horizon=np.inf):
    from tactics2d_amd.controller import IDMController
    n = C["n_env"] * C["A"]
    z = np.zeros(n, F32)
    row = IDMController(lane_half_width=half_width, horizon=horizon).row()
    return O.idm(row[None], np.zeros(n, np.uint8), C["n_env"], C["A"], st[:, 0], st[:, 1], st[:, 2], st[:, 3], C["active"], z, z)[2]


def _flat_routes(C):
    """(list of polylines, index of each participant's polyline in it) of C's route sets"""
    r = C["routes"]
    n_env, A = C["n_env"], C["A"]
    soe = np.zeros(n_env, int) if r["set_of_env"] is None else np.asarray(r["set_of_env"])   # (None: set 0 serves every env)
    first = np.concatenate([[0], np.cumsum([len(s) for s in r["sets"]])])
    flat = [np.ascontiguousarray(p, F32) for s in r["sets"] for p in s]
    ro = np.asarray(r["route_of"])
    index = np.where(ro >= 0, first[np.repeat(soe, A)] + ro, -1)
    return flat, index


def pursuit_want(O, C, st, accel_last, act_in=None):
    """pursuit_ref.evaluate for one t2d_pursuit_actions of C at state st (float32 [N, >= 4]) with the given accel_last"""
    R, cid, ts = C["pursuit"]
    n = len(cid)
    ctrl = cid != 255
    flat, index = _flat_routes(C)
    lead = leaders(O, C, st)
    return UR.evaluate(R[np.where(ctrl, cid, 0)], ctrl, st[:, 0], st[:, 1], st[:, 2], st[:, 3], accel_last, C["active"], ts, flat, index,
                       C["wb"], act_in, lead, C["A"])


def pid_want(C, st, state=None, act_in=None, ended=None):
    R, cid, ts = C["pid"]
    n = len(cid)
    ctrl = cid != 255
    flat, index = _flat_routes(C)
    return PR.evaluate(R[np.where(ctrl, cid, 0)], ctrl, np.zeros((n, 6)) if state is None else state, st[:, 0], st[:, 1], st[:, 2], st[:, 3],
                       C["active"], ts, *RR.pad_routes(flat, index), C["wb"], act_in, ended)


def episode(O, C, n_steps=HISTORY_STEPS):
    """The oracle chain of observe()'s control sequence from C's reset, on the CPU: the seeded rows -> pid_ref -> pursuit_ref -> the
    IDM oracle -> the C oracle's integrator (deterministic trig).  Returns (states float32 [n_steps + 1][N, 6], applied accel float32
    [n_steps + 1][N] (0.0 at the reset: T2D_F_APPLIED0), rows float32 [n_steps][N, 2])."""
    from tactics2d_amd import layout as L
    n = C["n_env"] * C["A"]
    st, applied, pid_state = state_of(C), np.zeros(n, F32), np.zeros((n, 6))
    states, applieds, rows = [st], [applied], []
    for _ in range(n_steps):
        a = C["act"].copy()
        if C["pid"] is not None:
            e = pid_want(C, st, pid_state, a)
            a, pid_state = e["rows"], e["state"]
        if C["pursuit"] is not None:
            a = pursuit_want(O, C, st, applied, a)["rows"]
        a0, a1 = a[:, 1].copy(), a[:, 0].copy()
        if C["idm"] is not None:
            a0, a1, _ = O.idm(C["idm"][0], C["idm"][1], C["n_env"], C["A"], st[:, 0], st[:, 1], st[:, 2], st[:, 3], C["active"], a0, a1)
        O.set_trig(1)
        try:
            o = O.integrate(C["rows"], st[:, 0], st[:, 1], st[:, 2], st[:, 3], st[:, 4], st[:, 5], a0, a1, C["type_id"], C["active"], 100)
        finally:
            O.set_trig(0)
        st, applied = o[:, :6].astype(F32), np.where(C["active"] != 0, o[:, 6], applied).astype(F32)
        states.append(st); applieds.append(applied); rows.append(np.stack([a1, a0], 1))
    return states, applieds, rows


def second_reset(seed=1, shape=SHAPE):
    """what the second t2d_reset brings: other poses, another `active` pattern (two off per env), the type ids swapped"""
    return traffic(seed, shape, type_pick=1, inactive=2)


RESET_KEYS = ("x", "y", "heading", "speed", "type_id", "active", "wb")


def masked(C_old, C_new, envs=MASKED):
    """(env mask uint8 [n_env], C_old with C_new's reset arrays in the selected envs): what a masked t2d_reset leaves in those envs"""
    mask = np.zeros(C_old["n_env"], np.uint8)
    mask[list(envs)] = 1
    sel = np.repeat(mask, C_old["A"]).astype(bool)
    C = dict(C_old)
    for k in RESET_KEYS:
        C[k] = np.where(sel, C_new[k], C_old[k]).astype(C_old[k].dtype)
    return mask, C


def fraction_differing(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(((a != b) & ~(np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else (a != b)).mean())


# ---------------------------------------------------------------------------------------------------- 4. the geometry ladder
GEO_KINDS = ("full", "static", "lanes")
GEO_STAGES = (("small", 0), ("mid", 1), ("big", 2), ("small", 3), ("none", 4))    # (stage, selection shift)
GEO_SHAPES = (SHAPE, WIDE)
NO_POLYGON_ENV, NO_LANE_ENV = 2, 4
MAP_QUEUE = 2048                  # kMapQueue of t2d_mapgrid.hip (tests/test_reuse_scenes.py holds it to the source): (participant, part) pairs of a 64-participant segment
PILE = {SHAPE: 100, WIDE: 60}     # boxes piled on every participant in G_big
FAR_AWAY = 5000.0
_TRIANGLE = np.float32([[-0.5, -0.5], [0.7, 0.0], [-0.5, 0.5]])
_SQUARE = np.float32([[-4, -4], [4, -4], [4, 4], [-4, 4]])


def geometry_base(shape, seed=0, pitch=15.0):
    """Parked traffic on a grid of `pitch` metres (nobody moves: speed 0, acceleration 0), random headings, the nine kinematic vehicles and some
    pedestrians (discs), a tenth inactive; no controllers, no routes.  check_dynamic and check_off_lane are on."""
    from tactics2d_amd import layout as L
    n_env, A = shape
    n = n_env * A
    rng = np.random.default_rng([seed, n_env, A, 4])
    rows, _, wb_all = kin_types()
    a = np.arange(n) % A
    x = pitch * (a % 4) + rng.uniform(-2, 2, n)
    y = pitch * (a // 4) + rng.uniform(-2, 2, n)
    ped = rng.random(n) < 0.15
    type_id = np.where(ped, rng.integers(21, 25, n), rng.integers(0, 9, n)).astype(np.uint8)
    active = (rng.random(n) >= 0.1).astype(np.uint8)
    active[0::A] = 1
    active[1], type_id[1] = 1, 3      # (the participant G_big sends 5 km away: an active car)
    act = np.stack([np.where(ped, 0.0, rng.normal(0, 0.02, n)), np.zeros(n)], 1).astype(F32)
    return dict(n_env=n_env, A=A, rows=rows, x=F32(x), y=F32(y), heading=F32(rng.uniform(0, 2 * np.pi, n)), speed=np.zeros(n, F32),
                type_id=type_id, active=active, wb=wb_all[type_id], static=None, lanes=None, boundary=None, boundary_valid=None,
                status=dict(max_step=100000, check_dynamic=1, check_off_lane=1), routes=None, idm=None, pid=None, pursuit=None,
                lidar=None, act=act)


def _padding(K, y0):
    """K small squares in rows of 32, 100 m and more from every participant: they change no verdict"""
    return [np.float32([[q % 32, y0 + q // 32], [q % 32 + 0.5, y0 + q // 32], [q % 32 + 0.5, y0 + q // 32 + 0.5], [q % 32, y0 + q // 32 + 0.5]])
            for q in range(K)]


def _budget(C, statics, lanes):
    from tactics2d_amd import mapgeom
    return mapgeom.geometry_budget(C["n_env"], C["A"], statics, lanes)


def geometry_stage(base, kind, stage, shift, fill=0.5):
    """base with the geometry of one rung.  Every env's map is its own: a triangle on every third participant (a collision), an
    8 m square under every other one (on-lane; the rest are off-lane), which ones moving with `shift`; env NO_POLYGON_ENV has no
    polygon at all, env NO_LANE_ENV statics but no lanes.  mid: far-away padding until the record of the fullest workgroup is
    more than half the 32 KiB budget; big: the HBM grid tier -- PILE boxes on every participant (more (participant, part) pairs
    in a 64-participant segment than MAP_QUEUE) or, lanes only, far-away lane squares -- and participant 1 FAR_AWAY to the east."""
    n_env, A = base["n_env"], base["A"]
    C = dict(base)
    if stage == "none":
        return C
    rng = np.random.default_rng([n_env, A, shift, 11])
    with_static, with_lanes = kind != "lanes", kind != "static"
    statics, lanes = [], []
    for e in range(n_env):
        st, ln = [], []
        for a in range(A if e != NO_POLYGON_ENV else 0):
            c = np.float32([base["x"][e * A + a], base["y"][e * A + a]])
            if (a + shift) % 3 == 0:
                st.append(_TRIANGLE + c)
            if (a + e + shift) % 2 == 0 and e != NO_LANE_ENV:
                ln.append(_SQUARE + c)
            if stage == "big" and with_static:
                for _ in range(PILE[(n_env, A)]):
                    th, hl, hw = rng.uniform(0, np.pi), rng.uniform(0.3, 2.5), rng.uniform(0.3, 1.2)
                    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
                    box = np.array([[hl, -hw], [hl, hw], [-hl, hw], [-hl, -hw]]) @ R.T
                    st.append(np.float32(box + c + rng.uniform(-1.5, 1.5, 2)))
        statics.append(st); lanes.append(ln)
    if stage == "big" and not with_static:
        for e in range(n_env):
            if e not in (NO_POLYGON_ENV, NO_LANE_ENV):
                lanes[e] = lanes[e] + [q + np.float32([300.0, 0.0]) for q in _padding(64, 0.0)]
    if stage == "mid":
        K = 0
        while True:
            K += 2
            st = [s + _padding(K, 100.0) if e != NO_POLYGON_ENV else s for e, s in enumerate(statics)]
            ln = [l + _padding(K, 200.0) if e not in (NO_POLYGON_ENV, NO_LANE_ENV) else l for e, l in enumerate(lanes)]
            b = _budget(C, st if with_static else None, ln if with_lanes else None)
            if b["dwords_needed"] > fill * b["dwords_budget"]:
                break
        statics, lanes = st, ln
    C["static"] = H.to_csr(statics) if with_static else None
    C["lanes"] = H.to_csr(lanes) if with_lanes else None
    if stage == "big":
        C["x"] = base["x"].copy()
        C["x"][1] += FAR_AWAY
    return C


def geometry_ladder(shape, kind):
    base = geometry_base(shape)
    return [(stage, geometry_stage(base, kind, stage, shift)) for stage, shift in GEO_STAGES]


NARROW_SHAPE = (2100, 8)      # 132 workgroups of 16 envs, 263 of 8: on a 256-CU device envs_per_workgroup starts at 16


def narrowing_ladder():
    """[(stage, C)]: G_small -> G_mid -> G_small -> none at NARROW_SHAPE, statics and lanes.  G_mid's record is more than 0.6 of the
    budget at 8 envs per workgroup (what geometry_budget reports: the narrowest workgroup), so it cannot fit at 16."""
    base = geometry_base(NARROW_SHAPE)
    return [(stage, geometry_stage(base, "full", stage, shift, fill=0.6)) for stage, shift in (("small", 0), ("mid", 1), ("small", 3), ("none", 4))]


def collide_want(O, C, x=None, y=None, heading=None):
    sc = dict(rows=C["rows"], n_env=C["n_env"], A=C["A"], x=C["x"] if x is None else x, y=C["y"] if y is None else y,
              heading=C["heading"] if heading is None else heading, type_id=C["type_id"], active=C["active"], static=C["static"],
              boundary=C["boundary"], boundary_valid=C["boundary_valid"], lanes=C["lanes"])
    return H.oracle_collide(O, sc)


def segment_pairs(O, C, first=0, count=64):
    """lower bound of the (participant, static part) pairs the map walk of participants [first, first + count) queues: pairs of
    one env whose axis-aligned boxes overlap (the walk's box test rejects nothing closer than that)"""
    from tactics2d_amd import layout as L
    eo, vo, xy = C["static"]
    A, total = C["A"], 0
    for i in range(first, min(first + count, C["n_env"] * A)):
        r = C["rows"][C["type_id"][i]]
        if not C["active"][i] or r[L.P_SHAPE] != L.SHAPE_OBB:
            continue
        P = np.asarray(O.pose_obb(C["x"][i], C["y"][i], C["heading"][i], r[L.P_LENGTH], r[L.P_WIDTH])).reshape(4, 2)
        lo, hi = P.min(0), P.max(0)
        e = i // A
        for p in range(eo[e], eo[e + 1]):
            Q = xy[vo[p]:vo[p + 1]]
            total += bool((Q.min(0) <= hi).all() and (Q.max(0) >= lo).all())
    return total


# ---------------------------------------------------------------------------------------------------- 5. the parameter table
def table_ladders():
    """name -> [(stage, C, the one-step form)]: the parameter table replaced on a live pool, then a reset.
    circle_row: a single-ego pool (5 x 1, boxes only) whose table gains a disc row nobody has -- the single-ego kernel is off --
    and loses it again; drift_row: a SingleTrackDrift row appears and disappears (the step goes launch by launch while it is
    there); long_vehicles: 2 x 70 (the pair stage walks its hash grid, whose cell is the largest circum-diameter of the table):
    the length of one vehicle type triples -- its cars now reach their neighbours -- and shrinks back."""
    from tactics2d_amd import layout as L
    full = kin_types()[0]
    ego = traffic(7, (5, 1), table="boxes", inactive=0, stuck_env=1)
    disc = dict(ego, rows=np.concatenate([ego["rows"], full[21:22]]))
    plain = traffic(7, SHAPE, stuck_env=1)
    drift = traffic(7, SHAPE, stuck_env=1, table="drift")
    parked = geometry_stage(geometry_base((2, 70), seed=3, pitch=9.0), "static", "small", 0)
    rows = parked["rows"].copy()
    rows[3, L.P_LENGTH] *= 3.0
    long_ = dict(parked, rows=rows)
    return {"circle_row": [("boxes", ego, "ego"), ("disc", disc, "step"), ("boxes again", ego, "ego")],
            "drift_row": [("plain", plain, "step"), ("drift", drift, "unfused"), ("plain again", plain, "step")],
            "long_vehicles": [("table", parked, "step"), ("tripled", long_, "step"), ("table again", parked, "step")]}


# ---------------------------------------------------------------------------------------------------- 6. the lidar
def _ring_statics(rng, n_env, centre):
    """per env: ten quads 13 - 19 m from the ego (between the two lidar ranges) and three 5 - 9 m from it"""
    per = []
    for e in range(n_env):
        r = np.concatenate([rng.uniform(13, 19, 10), rng.uniform(5, 9, 3)])
        th = rng.uniform(0, 2 * np.pi, len(r))
        per.append([q + np.float32(centre[e]) for q, cx, cy in
                    ((H.random_quads(rng, 1, (0, 0), (0, 0), size=(3.0, 5.0))[0], a * np.cos(t), a * np.sin(t)) for a, t in zip(r, th))
                    for q in [q + np.float32([cx, cy])]])
    return H.to_csr(per)


def sensor_base(seed=0, shape=SHAPE):
    """helpers.random_scene's table, types and boundary as a configuration for the sensors: the ego (a box) near the middle, the
    other participants parked 6 - 11 m around it, quads in two rings around it (_ring_statics)"""
    n_env, A = shape
    rng = np.random.default_rng([seed, n_env, A, 6])
    sc = H.random_scene(rng, n_env, A, (60.0, 60.0), n_static=0)
    n = n_env * A
    ego = np.arange(n) % A == 0
    sc["active"][ego] = 1
    sc["type_id"][ego] = sc["type_id"][ego] % len(H.VEHICLE_DIMS)        # the sensor of lidar_scan is a box
    r, th = rng.uniform(6, 11, n), rng.uniform(0, 2 * np.pi, n)
    centre = rng.uniform(-1, 1, (n_env, 2))
    x = np.where(ego, 0.0, r * np.cos(th)) + np.repeat(centre[:, 0], A)
    y = np.where(ego, 0.0, r * np.sin(th)) + np.repeat(centre[:, 1], A)
    return dict(n_env=n_env, A=A, rows=sc["rows"], x=F32(x), y=F32(y), heading=sc["heading"], speed=np.zeros(n, F32),
                type_id=sc["type_id"], active=sc["active"], wb=np.full(n, 2.5), static=_ring_statics(rng, n_env, centre), lanes=None,
                boundary=sc["boundary"], boundary_valid=sc["boundary_valid"], status=dict(max_step=100000), routes=None, idm=None,
                pid=None, pursuit=None, lidar=None, act=np.zeros((n, 2), F32))


def lidar_ladder():
    """[(stage, C)]: 360 beams / 20 m -> 120 / 12 m -> 360 / 20 m (the all-participants scan into the pool's own buffer across
    both changes); participants become obstacles; the statics are replaced, then removed"""
    base = sensor_base(0)
    other = sensor_base(1)["static"]
    wide = dict(n_beams=360, max_range=20.0, include_participants=False, all=True)
    return [("360 / 20 m", dict(base, lidar=wide)),
            ("120 / 12 m", dict(base, lidar=dict(wide, n_beams=120, max_range=12.0))),
            ("360 / 20 m again", dict(base, lidar=wide)),
            ("participants", dict(base, lidar=dict(wide, include_participants=True))),
            ("statics replaced", dict(base, lidar=dict(wide, include_participants=True), static=other)),
            ("statics removed", dict(base, lidar=dict(wide, include_participants=True), static=None))]


def lidar_want(O, C, x=None, y=None, heading=None):
    """oracle.lidar(..., trig=0) of the ego scan: float32 [n_env, n_beams]"""
    l = C["lidar"]
    return O.lidar(C["rows"], C["n_env"], C["A"], C["status"].get("ego_index", 0), C["x"] if x is None else x, C["y"] if y is None else y,
                   C["heading"] if heading is None else heading, C["type_id"], C["active"], C["static"], int(l["include_participants"]),
                   l["n_beams"], l["max_range"], trig=0)


def beams_differing(a, b):
    """share of beams that differ between two scans at the angles both have (120 beams are every third of 360)"""
    if a.shape[-1] != b.shape[-1]:
        big, small = (a, b) if a.shape[-1] > b.shape[-1] else (b, a)
        a, b = big[..., ::big.shape[-1] // small.shape[-1]], small
    return float((a.view(np.uint32) != b.view(np.uint32)).mean())


# ---------------------------------------------------------------------------------------------------- 8. the routes
def _line(y0, n_vert, amplitude=0.0):
    xs = np.linspace(-1024.0, 1024.0, n_vert)
    return np.stack([xs, y0 + amplitude * np.where(np.arange(n_vert) % 2, 1.0, -1.0)], 1).astype(F32)


ROUTE_SETS = {"two lines": [[_line(0.45, 5), _line(-0.45, 5)]],          # 10 vertices, two routes
              "fewer": [[_line(-0.45, 2)]],                               # 2 vertices
              "more": [[_line(0.0, 65, 0.8), _line(0.3, 33)]]}            # 98 vertices: a zigzag of 32 m legs, +-0.8 m


def route_ladder():
    """[(stage, C)] on the platoons of traffic(): route sets with fewer and with more vertices than the ones before, the first
    set again, then its assignment replaced (every other participant takes the second line).  The threshold stays 0.5 m."""
    base = traffic(11)
    n = base["n_env"] * base["A"]
    zero, alt = np.zeros(n, np.int32), (np.arange(n) % 2).astype(np.int32)
    r = lambda name, ro: dict(base, routes=dict(sets=ROUTE_SETS[name], set_of_env=None, route_of=ro, thr=0.5))
    return [("two lines", r("two lines", zero)), ("fewer", r("fewer", zero)), ("more", r("more", zero)),
            ("two lines again", r("two lines", zero)), ("assignment", r("two lines", alt))]


def off_route_want(C, x=None, y=None):
    r = C["routes"]
    n = C["n_env"] * C["A"]
    soe = np.zeros(C["n_env"], int) if r["set_of_env"] is None else r["set_of_env"]
    return RR.evaluate_sets(r["sets"], soe, r["route_of"], C["A"], C["x"] if x is None else x, C["y"] if y is None else y,
                            np.broadcast_to(F32(r["thr"]), (n,)), C["active"])


# ---------------------------------------------------------------------------------------------------- 10. the status configuration
STATUS_STAGES = (dict(max_step=100000, ego_index=3, check_dynamic=1, check_off_lane=1),     # the ego moved, the checks toggled
                 dict(max_step=2, ego_index=3, check_dynamic=1, check_off_lane=1))          # max_step below cnt_step


def status_scene():
    """traffic() without controllers under the default configuration (ego 0, no time limit in reach): the ego of env 1 and slot 3
    of env 2 stand in static squares.  STATUS_STAGES, set one after the other on the live episode (three steps in), move the ego
    to slot 3 and turn the dynamic and off-lane checks on, then lower max_step below cnt_step."""
    C = traffic(17, stuck_env=1)
    C.update(idm=None, pid=None, pursuit=None)
    A, n_env = C["A"], C["n_env"]
    C["active"] = C["active"].copy()
    C["active"][3::A] = 1
    i = 2 * A + 3
    square = np.float32([[-3, -3], [3, -3], [3, 3], [-3, 3]])
    per_env = [[square + np.float32([C["x"][e * A + a], C["y"][e * A + a]])] if (e, a) in ((1, 0), (2, 3)) else [] for e in range(n_env)
               for a in [0 if e == 1 else 3]]
    C["static"] = H.to_csr(per_env)
    return C


# ---------------------------------------------------------------------------------------------------- 7. the camera
CAMERA_RANGE = (25, 25, 35, 15)
OTHER_PALETTE = (np.arange(24, dtype=np.uint8).reshape(8, 3) * 9 + 1)


class _Cam:
    """what test_gpu_camera.expected reads of a camera"""

    def __init__(self, size):
        self.window_size, self.perception_range, self.heading_up = size, tuple(float(v) for v in CAMERA_RANGE), True


def camera_ladder():
    """[(stage, Scene, (width, height), class_of_type, palette)]: 64 x 48 -> 32 x 32 -> 64 x 48 on an intersection pool, the
    geometry replaced (a highway pool's), then palette and style replaced (every vehicle type drawn as a cyclist: z-order 6, over
    the lanes)"""
    import test_gpu_camera as TC
    from tactics2d_amd import layout as L, scenarios as S, sensor
    a, b = S.intersection(5, A=8, seed=4), S.highway(5, A=8, seed=9)
    ca, cb = TC.class_table(a), TC.class_table(b)
    styled = np.where(cb == L.CAMERA_CLASS_VEHICLE, L.CAMERA_CLASS_CYCLIST, cb).astype(np.uint8)
    pal = sensor.PALETTE
    return [("64x48", a, (64, 48), ca, pal), ("32x32", a, (32, 32), ca, pal), ("64x48 again", a, (64, 48), ca, pal),
            ("geometry replaced", b, (64, 48), cb, pal), ("palette and style replaced", b, (64, 48), styled, OTHER_PALETTE)]


def camera_layers(sc):
    return ["participants", "arrows"] + (["static"] if sc.static is not None else []) + (["lanes"] if sc.lanes is not None else [])


def camera_want(sc, size, class_of_type, palette):
    """camera_ref's class images and their colours at the scene's reset poses: uint8 [n_env, H, W], uint8 [n_env, H, W, 3]"""
    import test_gpu_camera as TC
    cam, out = _Cam(size), []
    for e in range(sc.n_env):
        env = dict(target=None, static=TC.csr_env(sc.static, e), lanes=TC.csr_env(sc.lanes, e), tiles=[],
                   participants=TC.participants_of(sc, sc.x, sc.y, sc.heading, e, class_of_type))
        out.append(TC.expected(env, (sc.x[e * sc.A], sc.y[e * sc.A], sc.heading[e * sc.A]), cam, arrows=True)[0])
    cls = np.stack(out).astype(np.uint8)
    return cls, np.asarray(palette, np.uint8)[cls]


def pixels_differing(a, b):
    """share of pixels that differ between two stacks of images [n_env, H, W(, 3)]; images of another size are compared where the
    smaller one's pixels fall in the larger one's grid (row i of h rows -> row i * H // h)"""
    if a.shape[1:3] != b.shape[1:3]:
        big, small = (a, b) if a.shape[1] * a.shape[2] > b.shape[1] * b.shape[2] else (b, a)
        r = np.arange(small.shape[1]) * big.shape[1] // small.shape[1]
        c = np.arange(small.shape[2]) * big.shape[2] // small.shape[2]
        a, b = big[:, r][:, :, c], small
    d = a != b
    return float((d.any(-1) if d.ndim == 4 else d).mean())


# ---------------------------------------------------------------------------------------------------- 9. the tracks
TRACK_STEPS = 4


def track_ladder():
    """[(stage, RaceScene)]: five racing envs on two short rings, on three other rings, and on the first two again (a
    device-generated set stands between the last two in the GPU test)"""
    import track_scenes as TS
    ring = lambda *a: TS.centred_f32(TS.ellipse_ring(*a))
    first = [ring(16, 26.0, 26.0), ring(24, 50.0, 30.0, 0.3)]
    other = [ring(33, 52.0, 52.0, 2.0), ring(48, 90.0, 60.0, 1.1), ring(20, 30.0, 40.0, 0.7)]
    return [("two rings", TS.build(5, seed=3, tracks=first)), ("three other rings", TS.build(5, seed=8, tracks=other)),
            ("two rings again", TS.build(5, seed=3, tracks=first))]


def track_want(O, sc, n_steps=TRACK_STEPS):
    """track_ref's progress after n_steps of the scripted driver on the C oracle: (tile_visiting [n_env], num_visited [n_env])"""
    import track_ref as R
    import track_scenes as TS
    roll, prog = TS.cpu_rollout(O, sc, R.RULE_FORWARD, 8, n_steps)
    return prog.visiting.copy(), prog.num_visited.copy()


# ---------------------------------------------------------------------------------------------------- 10b. the target areas
TARGET_STATUS = dict(max_step=100000, ego_index=3, check_dynamic=1, check_arrival=1, shaped_reward=1)


def target_stages(C):
    """[(stage, target float32 [n_env, 4, 2] or None)] for status_scene(): a bay 4 m ahead of the ego (slot 3) of every env, a bay
    20 m ahead and 3 m to the side in its place, then none"""
    A = C["A"]
    ex, ey = C["x"][3::A].astype(np.float64), C["y"][3::A].astype(np.float64)
    bay = np.array([[-2.7, -1.3], [2.7, -1.3], [2.7, 1.3], [-2.7, 1.3]])
    quad = lambda dx, dy: np.float32(bay[None] + np.stack([ex + dx, ey + dy], 1)[:, None, :])
    return [("a bay ahead", quad(4.0, 0.0)), ("another bay", quad(20.0, 3.0)), ("no target", None)]


def rs_targets(C):
    """(target [n_env, 4, 2], heading [n_env]) for sensor_base(): a bay 9 m east of every ego, along x"""
    A = C["A"]
    ex, ey = C["x"][0::A].astype(np.float64), C["y"][0::A].astype(np.float64)
    bay = np.array([[-2.7, -1.3], [2.7, -1.3], [2.7, 1.3], [-2.7, 1.3]])
    return np.float32(bay[None] + np.stack([ex + 9.0, ey], 1)[:, None, :]), np.zeros(C["n_env"])
