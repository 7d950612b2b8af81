"""Shared test helpers: golden loading, scene synthesis, GPU drivers (through the C ABI)."""
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
TWO_PI = 2 * np.pi


def load_npz(name):
    return dict(np.load(os.path.join(GOLD, name)))


def load_json(name):
    with open(os.path.join(GOLD, name)) as f:
        return json.load(f)


def ang_err(a, b):
    d = np.abs(np.asarray(a, np.float64) - np.asarray(b, np.float64))
    return np.minimum(d, np.abs(TWO_PI - d))


def state_err(got, want, cols=4):
    """max abs error per column (x, y, heading (wrapped), speed[, vx, vy])."""
    got = np.asarray(got, np.float64); want = np.asarray(want, np.float64)
    e = np.abs(got[:, :cols] - want[:, :cols])
    e[:, 2] = ang_err(got[:, 2], want[:, 2])
    return e


# Conditioning of a SingleTrackDynamics step.  Column `sens` of dyn_random.npz (oracle/gen_golden.py) is the largest
# change of the REFERENCE's own output when one of its inputs (heading, speed, acceleration, steering angle) moves by one
# fp64 ulp.  The deterministic trig differs from numpy's by <= 1 ulp per call, ~80 calls per step, so:
#   * 100 x sens < 1e-6  -> the north-star tolerance (1e-5 abs after the fp32 store) is asserted as is;
#   * sens < 1e-3        -> a conditioning-scaled bound is asserted: 1e-5 + 1000 x sens;
#   * sens >= 1e-3       -> one ulp moves the reference's own result by a millimetre or more (its explicit Euler is
#                           unstable in the tyre-force branch at crawling speed, DESIGN.md "Dynamics conditioning"):
#                           reported, and covered by the bit-exact comparison with the deterministic oracle.
SENS_STRICT = 1e-8
SENS_CHAOTIC = 1e-3


SENS_SCALE = 600.0   # the worst observed |error| / (1e-5 + SENS_SCALE x sens) over the 221 scaled cases of dyn_random.npz is 0.9


def dyn_chaotic_bound(sens, tol=1e-5):
    """the bound held even where the reference is chaotic (sens >= SENS_CHAOTIC): the same K x sens as the scaled cases"""
    return tol + SENS_SCALE * np.asarray(sens, np.float64)


def dyn_max_trig_argument(d, k):
    """The largest |phi + beta| SingleTrackDynamics._step (single_track_dynamics.py:140-229) feeds to cos / sin while it
    integrates case k of dyn_random.npz: where the reference's own slip angle explodes (crawling speed, tyre-force branch)
    it reaches 1e14 .. 1e18 rad -- outside the domain the deterministic sincos is specified for (|x| < 1e9)."""
    from tactics2d_amd import layout as L
    row = d["rows"][d["type_id"][k]]
    iv, dt_ms = (int(v) for v in d["timing"][k])
    lf, lr, wb = row[L.P_LF], row[L.P_LR], row[L.P_WB]
    mass, hcg, mu, Iz, cf, cr = (row[c] for c in (L.P_MASS, L.P_MASS_HEIGHT, L.P_MU, L.P_IZ, L.P_CF, L.P_CR))
    _, _, phi, v = (float(np.float32(q)) for q in d["state"][k])
    accel = float(np.clip(np.float32(d["action"][k][0]), row[L.P_ACCEL_LO], row[L.P_ACCEL_HI]))
    delta = float(np.clip(np.float32(d["action"][k][1]), row[L.P_STEER_LO], row[L.P_STEER_HI]))
    dt, g = dt_ms / 1000, 9.81
    ff, fr = (g * lr - accel * hcg) / wb, (g * lf + accel * hcg) / wb
    d_phi, beta, worst = v / wb * np.tan(delta), np.arctan(lr / lf * np.tan(delta)), 0.0
    for _ in range(iv // dt_ms):
        worst = max(worst, abs(phi + beta))
        vs = v if abs(v) > 1e-6 else (1e-6 if v >= 0 else -1e-6)
        if abs(v) >= 0.1:
            dd_phi = mu * mass / Iz * (lf * cf * ff * delta + (lr * cr * fr - lf * cf * ff) * beta - (lf * lf * cf * ff + lr * lr * cr * fr) * d_phi / vs)
            d_beta = mu / vs * (cf * ff * delta - (cr * fr + cf * ff) * beta + (lr * cr * fr - lf * cf * ff) * d_phi / vs) - d_phi
            d_phi += dd_phi * dt
        else:
            d_beta = lr / (1 + np.tan(delta) * lr / wb) ** 2 / wb / np.cos(delta) ** 2 * delta
            d_phi += v * np.cos(beta) / wb * np.tan(delta) * dt
        v = float(np.clip(v + accel * dt, row[L.P_SPEED_LO], row[L.P_SPEED_HI]))
        phi += d_phi * dt
        beta += d_beta * dt
    return worst


def dyn_tolerance(sens, tol=1e-5):
    """per-case tolerance (np.inf where the reference is chaotic) and the mask of the strictly asserted cases"""
    sens = np.asarray(sens, np.float64)
    t = np.where(sens < SENS_STRICT, tol, np.where(sens < SENS_CHAOTIC, tol + SENS_SCALE * sens, np.inf))
    return t, sens < SENS_STRICT


def rollout_sensitivity(oracle, sc, acts, idx):
    """Conditioning of a whole roll-out, per participant of `idx`: the largest change of the ORACLE's final state (x, y,
    wrapped heading, speed; fp32 store after every step, as the pool does) when the start heading or speed, or the first
    step's action, moves by ONE fp32 ulp -- the yardstick for comparing two correct integrators (fast vs exact kernel
    variant: they differ by ~1e-15 relative per operation, i.e. ~1e-7 of an fp32 ulp of an input)."""
    idx = np.asarray(idx)
    f = np.float32
    tid, act = sc.type_id[idx], sc.active[idx]

    def run(h0, v0, a00, a10):
        x, y, h, v = sc.x[idx].copy(), sc.y[idx].copy(), h0.copy(), v0.copy()
        for k, (a0, a1) in enumerate(acts):
            o = oracle.integrate(sc.rows, x, y, h, v, None, None, a00 if k == 0 else a0[idx], a10 if k == 0 else a1[idx], tid, act, sc.interval_ms)
            x, y, h, v = (f(o[:, c]) for c in range(4))
        return np.stack([x, y, h, v], 1).astype(np.float64)

    h0, v0, a00, a10 = sc.heading[idx], sc.speed[idx], acts[0][0][idx], acts[0][1][idx]
    up = lambda z: np.nextafter(f(z), f(np.inf))
    dn = lambda z: np.nextafter(f(z), f(-np.inf))
    oracle.set_trig(1)
    try:
        base = run(h0, v0, a00, a10)
        worst = np.zeros(len(idx))
        for probe in ((up(h0), v0, a00, a10), (dn(h0), v0, a00, a10), (h0, up(v0), a00, a10), (h0, dn(v0), a00, a10),
                      (h0, v0, up(a00), a10), (h0, v0, a00, up(a10)), (h0, v0, a00, dn(a10))):
            o2 = run(*probe)
            d = np.abs(o2 - base)
            d[:, 2] = np.minimum(d[:, 2], np.abs(TWO_PI - d[:, 2]))
            worst = np.maximum(worst, d.max(1))
    finally:
        oracle.set_trig(0)
    return worst


# --------------------------------------------------------------------------- GPU drivers
def gpu_physics(rows, type_id, state, action, interval, variant="exact", model="kin"):
    """Run every case as its own 1-agent env through t2d_integrate; chunk by <= 32 types.
    state: (n,4) fp32 = x,y,heading,speed (kin/dyn) or x,y,vx,vy (pm).
    Returns fp32 (n, 8): x, y, heading, speed, vx, vy, applied0, applied1."""
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    rows = np.asarray(rows, np.float64)
    type_id = np.asarray(type_id)
    n = len(type_id)
    out = np.full((n, 8), np.nan, np.float32)
    utypes = np.unique(type_id)
    for c0 in range(0, len(utypes), 32):
        chunk = utypes[c0:c0 + 32]
        sel = np.nonzero(np.isin(type_id, chunk))[0]
        remap = {int(t): i for i, t in enumerate(chunk)}
        tid = np.array([remap[int(t)] for t in type_id[sel]], np.uint8)
        m = len(sel)
        pool = ParticipantPool(m, 1)
        try:
            pool.set_param_table(rows[chunk])
            pool.set_integrator_variant(variant)
            st = np.asarray(state[sel], np.float32)
            if model == "pm":
                z = np.zeros(m, np.float32)
                pool.reset(st[:, 0], st[:, 1], z, z, tid, vx=st[:, 2], vy=st[:, 3])
            else:
                pool.reset(st[:, 0], st[:, 1], st[:, 2], st[:, 3], tid)
            pool.set_actions(action[sel, 0], action[sel, 1])
            pool.integrate(int(interval))
            cols = [pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY,
                                               L.F_APPLIED0, L.F_APPLIED1)]
            out[sel] = np.stack(cols, 1)
        finally:
            pool.close()
    return out


def oracle_physics(O, rows, type_id, state, action, interval, model="kin", trig=0):
    O.set_trig(trig)
    try:
        st = np.asarray(state, np.float32)
        if model == "pm":
            r = O.integrate(rows, st[:, 0], st[:, 1], None, None, st[:, 2], st[:, 3],
                            action[:, 0], action[:, 1], type_id, None, interval)
        else:
            r = O.integrate(rows, st[:, 0], st[:, 1], st[:, 2], st[:, 3], None, None,
                            action[:, 0], action[:, 1], type_id, None, interval)
    finally:
        O.set_trig(0)
    return r


# --------------------------------------------------------------------------- scenes
VEHICLE_DIMS = [(3.540, 1.641), (4.053, 1.751), (4.284, 1.799), (4.866, 1.832), (5.050, 1.886),
                (5.302, 1.945), (4.788, 1.916), (5.155, 1.995), (4.828, 1.943)]
PED_DIMS = [(0.24, 0.40), (0.22, 0.37), (0.18, 0.25), (0.20, 0.35)]


def shape_rows(with_peds=True):
    """Parameter rows that only matter for their shape columns (collision tests)."""
    rows = []
    for (Ln, W) in VEHICLE_DIMS:
        r = np.zeros(24); r[0] = 0; r[1] = 1.2; r[2] = 1.3; r[3] = 2.5; r[17] = 5
        r[18] = 0; r[19] = Ln; r[20] = W
        rows.append(r)
    if with_peds:
        for (Ln, W) in PED_DIMS:
            r = np.zeros(24); r[0] = 2; r[17] = 5; r[18] = 1; r[19] = Ln; r[20] = W
            rows.append(r)
    return np.array(rows)


def random_quads(rng, n, cx_range, cy_range, size=(2.0, 6.0)):
    """n random convex quads (perturbed rotated boxes), random winding."""
    polys = []
    for _ in range(n):
        cx = rng.uniform(*cx_range); cy = rng.uniform(*cy_range)
        L_, W_ = rng.uniform(*size), rng.uniform(size[0] / 2, size[1] / 2)
        h = rng.uniform(0, TWO_PI)
        base = np.array([[L_ / 2, -W_ / 2], [L_ / 2, W_ / 2], [-L_ / 2, W_ / 2], [-L_ / 2, -W_ / 2]])
        base += rng.uniform(0, 0.2, base.shape) * min(L_, W_)
        R = np.array([[np.cos(h), -np.sin(h)], [np.sin(h), np.cos(h)]])
        q = base @ R.T + [cx, cy]
        if rng.uniform() < 0.5:
            q = q[::-1]
        polys.append(q.astype(np.float32))
    return polys


def random_convex_polys(rng, n, cx_range, cy_range, size=(2.0, 6.0)):
    """n random convex polygons with 3..8 vertices (points of an ellipse at sorted random angles), random winding."""
    polys = []
    for _ in range(n):
        k = int(rng.integers(3, 9))
        ang = np.sort(rng.uniform(0, TWO_PI, k))
        if np.min(np.diff(np.concatenate([ang, [ang[0] + TWO_PI]]))) < 0.15:     # keep the vertices apart
            ang = TWO_PI * (np.arange(k) + rng.uniform(0, 0.3, k)) / k
        a, b = rng.uniform(*size) / 2, rng.uniform(size[0] / 2, size[1] / 2) / 2
        h = rng.uniform(0, TWO_PI)
        q = np.stack([a * np.cos(ang), b * np.sin(ang)], 1)
        R = np.array([[np.cos(h), -np.sin(h)], [np.sin(h), np.cos(h)]])
        q = q @ R.T + [rng.uniform(*cx_range), rng.uniform(*cy_range)]
        if rng.uniform() < 0.5:
            q = q[::-1]
        polys.append(q.astype(np.float32))
    return polys


def polygon_scene(rng, n_env, A, extent=(40.0, 24.0), n_static=5, n_lanes=3, with_peds=True):
    """Static obstacles and lanes with 3..8 vertices (the library evaluates 5..8-gons as fans of quads)."""
    sc = random_scene(rng, n_env, A, extent, n_static=0, n_lanes=0, with_peds=with_peds)
    sc["static"] = to_csr([random_convex_polys(rng, int(rng.integers(0, n_static + 1)), (-extent[0] / 2, extent[0] / 2),
                                               (-extent[1] / 2, extent[1] / 2)) for _ in range(n_env)])
    sc["lanes"] = to_csr([random_convex_polys(rng, int(rng.integers(0, n_lanes + 1)), (-extent[0] / 3, extent[0] / 3),
                                              (-extent[1] / 3, extent[1] / 3), size=(10.0, 36.0)) for _ in range(n_env)])
    return sc


def to_csr(per_env_polys):
    eo = [0]; vo = [0]; xy = []
    for polys in per_env_polys:
        for q in polys:
            xy.append(np.asarray(q, np.float32)); vo.append(vo[-1] + len(q))
        eo.append(eo[-1] + len(polys))
    xy = np.concatenate(xy) if xy else np.zeros((0, 2), np.float32)
    return np.array(eo, np.int32), np.array(vo, np.int32), xy


def random_scene(rng, n_env, A, extent=(60.0, 20.0), n_static=6, n_lanes=0, with_peds=True,
                 inactive_frac=0.1, bounded=True):
    rows = shape_rows(with_peds)
    N = n_env * A
    x = rng.uniform(-extent[0] / 2, extent[0] / 2, N).astype(np.float32)
    y = rng.uniform(-extent[1] / 2, extent[1] / 2, N).astype(np.float32)
    h = rng.uniform(-0.5, TWO_PI + 0.5, N).astype(np.float32)
    tid = rng.integers(0, len(rows), N).astype(np.uint8)
    active = (rng.uniform(size=N) >= inactive_frac).astype(np.uint8)
    static = to_csr([random_quads(rng, int(rng.integers(0, n_static + 1)),
                                  (-extent[0] / 2, extent[0] / 2), (-extent[1] / 2, extent[1] / 2))
                     for _ in range(n_env)]) if n_static else None
    lanes = None
    if n_lanes:
        per = []
        for _ in range(n_env):
            k = int(rng.integers(0, n_lanes + 1))
            per.append(random_quads(rng, k, (-extent[0] / 3, extent[0] / 3), (-extent[1] / 3, extent[1] / 3),
                                    size=(10.0, 40.0)))
        lanes = to_csr(per)
    boundary = bvalid = None
    if bounded:
        bx = rng.uniform(0.35, 0.6, n_env) * extent[0]; by = rng.uniform(0.35, 0.6, n_env) * extent[1]
        boundary = np.stack([-bx, bx, -by, by], 1).astype(np.float32)
        bvalid = (rng.uniform(size=n_env) > 0.1).astype(np.uint8)
    return dict(rows=rows, n_env=n_env, A=A, x=x, y=y, heading=h, type_id=tid, active=active,
                static=static, lanes=lanes, boundary=boundary, boundary_valid=bvalid)


def structured_lanes(rng, kind):
    """Lane sets whose polygons ABUT exactly (shared fp32 vertices) or overlap: a straight multi-lane road in an
    arbitrary direction, a polygonal ring of trapezoids with an arm, crossing roads with corner fillets, a frame of
    four strips around a hole.  The union's boundary pieces (off-lane = not union.contains(pose)) matter here."""
    if kind == 0:
        th = rng.uniform(0, np.pi); n_l = int(rng.integers(2, 5)); w = 3.75
        c, s = np.cos(th), np.sin(th)
        rails = [np.float32([[-40 * c - o * s, -40 * s + o * c], [40 * c - o * s, 40 * s + o * c]])
                 for o in (np.arange(n_l + 1) - n_l / 2) * w]
        return [np.float32([rails[k][0], rails[k][1], rails[k + 1][1], rails[k + 1][0]]) for k in range(n_l)]
    if kind == 1:
        nseg = int(rng.integers(6, 13)); r_in, r_out = 12.0, 20.0
        ang = TWO_PI * (np.arange(nseg + 1) % nseg) / nseg
        ri = np.float32(np.stack([r_in * np.cos(ang), r_in * np.sin(ang)], 1))
        ro = np.float32(np.stack([r_out * np.cos(ang), r_out * np.sin(ang)], 1))
        lanes = [np.float32([ri[k], ro[k], ro[k + 1], ri[k + 1]]) for k in range(nseg)]
        lanes.append(np.float32([[19, -3.75], [45, -3.75], [45, 3.75], [19, 3.75]]))
        return lanes
    if kind == 2:
        half = 30.0
        lanes = [np.float32([[-half, -3.75], [half, -3.75], [half, 3.75], [-half, 3.75]]),
                 np.float32([[-3.75, -half], [3.75, -half], [3.75, half], [-3.75, half]])]
        for sx in (-1, 1):
            for sy in (-1, 1):
                lanes.append(np.float32([[sx * 3.75, sy * 3.75], [sx * 7.75, sy * 3.75], [sx * 3.75, sy * 7.75]]))
        return lanes
    g = rng.uniform(0.3, 3.0); t = rng.uniform(0.5, 3.0); o = g + t
    return [np.float32([[-o, -o], [o, -o], [o, -g], [-o, -g]]), np.float32([[-o, g], [o, g], [o, o], [-o, o]]),
            np.float32([[-o, -g], [-g, -g], [-g, g], [-o, g]]), np.float32([[g, -g], [o, -g], [o, g], [g, g]])]


def structured_lane_scene(rng, n_env, A, with_peds=True):
    """Participants scattered over structured lane unions (one family per env), random headings."""
    rows = shape_rows(with_peds)
    per, X, Y = [], [], []
    for e in range(n_env):
        kind = e % 4
        per.append(structured_lanes(rng, kind))
        ext = (9.0, 21.0, 9.0, 4.0)[kind]
        X.append(rng.uniform(-ext, ext, A)); Y.append(rng.uniform(-ext, ext, A))
    N = n_env * A
    return dict(rows=rows, n_env=n_env, A=A, x=np.concatenate(X).astype(np.float32), y=np.concatenate(Y).astype(np.float32),
                heading=rng.uniform(0, TWO_PI, N).astype(np.float32), type_id=rng.integers(0, len(rows), N).astype(np.uint8),
                active=np.ones(N, np.uint8), static=None, lanes=to_csr(per), boundary=None, boundary_valid=None)


def count_vertices_in_but_not_contained(O, sc, flags, envs=None):
    """Box participants flagged off-lane although each of their four vertices lies in some lane polygon -- the
    case a vertex-only rule misses (body cutting a corner of the union, a hole or gap under the body)."""
    eo, vo, xy = sc["lanes"]
    A = sc["A"]
    n = 0
    for e in (range(sc["n_env"]) if envs is None else envs):
        polys = []
        for p in range(eo[e], eo[e + 1]):
            P = np.float64(xy[vo[p]:vo[p + 1]])
            a2 = sum(P[i, 0] * P[(i + 1) % len(P), 1] - P[(i + 1) % len(P), 0] * P[i, 1] for i in range(len(P)))
            polys.append(np.ascontiguousarray(P if a2 > 0 else P[::-1]))
        for i in range(e * A, (e + 1) * A):
            r = sc["rows"][sc["type_id"][i]]
            if r[18] != 0 or not sc["active"][i] or not (flags[i] & 8):
                continue
            pose = O.pose_obb(sc["x"][i], sc["y"][i], sc["heading"][i], r[19], r[20])
            n += all(any(O.point_in_convex(P, v) for P in polys) for v in pose)
    return n


def lane_safe_rects(lanes):
    """t2d_lane_safe_rects for every env of a lane CSR triple: [n_env, SAFE_RECTS, 4] fp32 (xmin, xmax, ymin, ymax; an unused slot is
    not finite) -- the rectangles inside which the step kernel certifies a pose as on-lane without the lane sweep.  Host-only entry
    point of libt2d_hip.so: no device is touched."""
    import ctypes as C
    from tactics2d_amd import _ffi, layout as L
    eo, vo, xy = (np.ascontiguousarray(a, dt) for a, dt in zip(lanes, (np.int32, np.int32, np.float32)))
    n_env = len(eo) - 1
    out = np.zeros((n_env, L.SAFE_RECTS, 4), np.float32)
    rc = _ffi.lib().t2d_lane_safe_rects(n_env, eo.ctypes.data_as(C.c_void_p), vo.ctypes.data_as(C.c_void_p), xy.ctypes.data_as(C.c_void_p),
                                        out.ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    return out


def gpu_collide(sc):
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc["n_env"], sc["A"])
    try:
        pool.set_param_table(sc["rows"])
        pool.set_static_geometry(sc["static"], sc["boundary"], sc["boundary_valid"])
        pool.set_lane_geometry(sc["lanes"])
        z = np.zeros(sc["n_env"] * sc["A"], np.float32)
        pool.reset(sc["x"], sc["y"], sc["heading"], z, sc["type_id"], sc["active"])
        pool.collide()
        return pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS)
    finally:
        pool.close()


def oracle_collide(O, sc, trig=0):
    return O.collide(sc["rows"], sc["n_env"], sc["A"], sc["x"], sc["y"], sc["heading"], sc["type_id"],
                     sc["active"], sc["static"], sc["boundary"], sc["boundary_valid"], sc["lanes"], trig)
