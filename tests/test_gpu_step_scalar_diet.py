"""The step kernel after its scalar diet: in `process_lane` the verdict "a boundary piece meets the open pose" is a word in a
vector register OR-ed behind a plain divergent `if` (it was a loop-carried lane mask behind a ballot, and still is in the launches with
integrator waves only: `loop_pipe` on the diamond and structured scenes below, fewer than five lane polygons per env), and the record's staging
rounds come from a shift (workgroups of 64, 128 and 256 threads: the narrow pools below).  Results must be the oracle's, bit for bit, in every
form of the step -- one launch, chain, chain_split, loop, loop_pipe -- on small pools aimed at what was rewritten:

  (a) a wide pool (A = 64) and a narrow one (A = 5 of 8 slots: three invalid lanes per env, 37 envs: a last workgroup of 5 envs);
  (b) one env = one wave = one pass of the lane stage's queue, in which exactly ONE entry has a boundary piece through its pose
      and 63 are clear of every piece -- and the reverse -- for boxes and for discs (a diamond lane: no axis-parallel edge, so
      no safe rectangle takes a pose out of the lane stage);
  (c) a NaN position, an infinite heading and a NaN action in single lanes of the wide pool;
  (d) three steps of a mixed pool of 6 envs in every form against the oracle's own chain: state, flags, records, status, rewards,
      counters (exact integrator), and the flags of the fast integrator against the oracle on the poses it stored;
  (e) lane unions that overlap, nest and meet at reflex corners: the lane scenes of tests/golden/geometry_kats.json side by side
      in one pool, and 64 participants scattered over structured unions.
Each scene has a test without a GPU that confirms that the oracle itself flags what the scene is meant to flag.
"""
import numpy as np
import pytest

import geom_scenes as GS
import helpers as H

gpu = pytest.mark.gpu

OFF_LANE, DYNAMIC, STATIC, OUT_BOUND = 8, 1, 2, 4
# form -> (t2d_set_step_chaining, split); "step" is one t2d_step
# (chain_split: one workgroup per env -- envs of 33 .. 64 with static polygons AND lanes, and it is preferred to the loop where allowed)
WIDE_FORMS = {"step": None, "chain": (2, False), "chain_split": (2, True), "loop": (3, False), "loop_pipe": (1, True)}
NARROW_FORMS = {"step": None, "chain": (2, False), "loop": (3, False), "loop_pipe": (1, True)}
N_STEPS = 3
_cache = {}


def _cached(key, make):
    if key not in _cache:
        _cache[key] = make()
    return _cache[key]


# ---- (b) the diamond lane ---------------------------------------------------------------------------------------------------------
R = 10.0
DIAMOND = np.float32([[R, 0], [0, R], [-R, 0], [0, -R]])
T_BOX, T_DISC = 4, GS.T_DISC4          # a 0.125 x 0.0625 box, a disc of radius 1/16
IN = 0.02                              # a straddler's centre lies this far inside the edge: less than either shape's reach


def _reach(kind):
    """the shape's support along a diamond edge's normal (heading 0)"""
    L_, W_ = GS.BOXES[T_BOX]
    return (L_ / 2 + W_ / 2) / np.sqrt(2.0) if kind == "box" else GS.DISCS[1] / 2


def _not_clear(kind, x, y):
    """restatement of process_lane's filter: does the lane have a piece of the diamond's outline it must hand to the exact test?"""
    L_, W_ = GS.BOXES[T_BOX]
    P = np.float64(DIAMOND)
    hit = False
    for k in range(4):
        a, b = P[k], P[(k + 1) % 4]
        nx, ny = a[1] - b[1], b[0] - a[0]
        s1 = nx * (x - a[0]) + ny * (y - a[1])
        if kind == "box":    # (the edge vectors of a heading-0 box: P = vertex 0 - vertex 3 = (L, 0), Q = vertex 1 - vertex 0 = (0, W))
            e2 = abs(nx * L_) + abs(ny * W_)
            clear = abs(2 * s1) > e2 + 2e-9 * (abs(nx) + abs(ny))
        else:
            r = GS.DISCS[1] / 2
            clear = s1 * s1 > r * r * (nx * nx + ny * ny) * (1.0 + 1e-9)
        hit |= not clear
    return hit


def _interior(n):
    """n points of a 1-m grid well inside the diamond (nobody near anybody, every outline piece's line far away)"""
    g = [(gx, gy) for gx in np.arange(-R, R + 0.5, 1.0) for gy in np.arange(-R, R + 0.5, 1.0) if abs(gx) + abs(gy) <= R - 2.0]
    assert len(g) >= n
    return g[:n]


def _straddlers(n):
    """n points IN metres inside the outline, 0.5 m apart in x along the four edges, clear of the corners"""
    pts = []
    for sx, sy in ((1, 1), (-1, 1), (-1, -1), (1, -1)):
        for t in np.arange(1.0, R - 0.99, 0.5):
            ex, ey = sx * t, sy * (R - t)                               # on the edge |x| + |y| = R
            pts.append((ex - sx * IN / np.sqrt(2.0), ey - sy * IN / np.sqrt(2.0)))
    assert len(pts) >= n
    return pts[:n]


def diamond_scene(kind, which):
    """one env of 64: `one_cut` = 63 interior poses and one straddler (slot 37); `one_clear` = 63 straddlers and one interior pose"""
    pts = (_interior(63) + _straddlers(1)) if which == "one_cut" else (_straddlers(63) + _interior(1))
    pts = pts[:37] + pts[63:] + pts[37:63]      # the odd one out sits in slot 37, not at an end of the wave
    xy = np.float32(pts)
    n = 64
    return dict(rows=GS.rows(), n_env=1, A=n, x=xy[:, 0].copy(), y=xy[:, 1].copy(), heading=np.zeros(n, np.float32),
                type_id=np.full(n, T_BOX if kind == "box" else T_DISC, np.uint8), active=np.ones(n, np.uint8), static=None,
                lanes=H.to_csr([[DIAMOND]]), boundary=None, boundary_valid=None, odd=37)


@pytest.mark.parametrize("kind", ["box", "disc"])
@pytest.mark.parametrize("which", ["one_cut", "one_clear"])
def test_diamond_scenes_put_one_lane_on_the_other_side_of_the_branch(oracle, kind, which):
    sc = diamond_scene(kind, which)
    assert IN < _reach(kind)
    assert not np.isfinite(H.lane_safe_rects(sc["lanes"])).all(-1).any(), "a safe rectangle would keep poses out of the lane stage"
    need = np.array([_not_clear(kind, float(x), float(y)) for x, y in zip(sc["x"], sc["y"])])
    odd = np.zeros(64, bool); odd[sc["odd"]] = True
    assert np.array_equal(need, odd if which == "one_cut" else ~odd)
    f, _ = H.oracle_collide(oracle, sc)
    assert np.array_equal(f, np.where(need, OFF_LANE, 0)), f.tolist()   # every centre is inside: the piece alone decides; nobody collides


# ---- (a) wide and narrow, (c) non-finite lanes, (e) overlapping unions ---------------------------------------------------------------
def wide_scene():
    return _cached("wide", lambda: GS.map_scene(6, 64, seed=1))


def narrow_scene():
    return _cached("narrow", lambda: GS.map_scene(37, 5, seed=2))


def _nonfinite_lanes():
    """a participant off its lane (motif `lane_outside`: flagged whatever the ulps) in envs 1, 2 and 5 -- the last env sits in the partly
    filled workgroup"""
    m = wide_scene()["motif"].reshape(6, 64)
    pick = lambda e: e * 64 + int(np.flatnonzero(m[e] == "lane_outside")[0])
    return {"nan_x": pick(1), "inf_heading": pick(2), "nan_action": pick(5)}


def nonfinite_scene():
    NONFINITE = _nonfinite_lanes()
    sc = dict(wide_scene())
    sc["x"] = sc["x"].copy(); sc["heading"] = sc["heading"].copy()
    sc["x"][NONFINITE["nan_x"]] = np.nan
    sc["heading"][NONFINITE["inf_heading"]] = np.inf
    a0 = np.zeros(sc["n_env"] * sc["A"], np.float32)
    a0[NONFINITE["nan_action"]] = np.nan
    return sc, a0, NONFINITE


def kat_scene():
    """the lane scenes of geometry_kats.json, one env each (they share one type table), A = 3 with unused slots inactive"""
    def make():
        ks = [k for k in H.load_json("geometry_kats.json")["scenes"] if k["lanes"] and not k["static"] and not k["boundary"]]
        assert all(k["rows"] == ks[0]["rows"] for k in ks)
        A = 3
        n = len(ks)
        z = lambda dt: np.zeros((n, A), dt)
        x, y, h, tid, act, want = z(np.float32), z(np.float32), z(np.float32), z(np.uint8), z(np.uint8), z(np.uint32)
        for e, k in enumerate(ks):
            m = len(k["x"])
            x[e, :m], y[e, :m], h[e, :m], tid[e, :m], act[e, :m], want[e, :m] = k["x"], k["y"], k["heading"], k["type_id"], 1, k["flags"]
        sc = dict(rows=np.array(ks[0]["rows"]), n_env=n, A=A, x=x.reshape(-1), y=y.reshape(-1), heading=h.reshape(-1),
                  type_id=tid.reshape(-1), active=act.reshape(-1), static=None, boundary=None, boundary_valid=None,
                  lanes=H.to_csr([[np.float32(q) for q in k["lanes"]] for k in ks]), want=want.reshape(-1),
                  names=[k["name"] for k in ks])
        return sc
    return _cached("kats", make)


def structured_scene():
    return _cached("structured", lambda: H.structured_lane_scene(np.random.default_rng(41), 8, 64))


def test_wide_and_narrow_scenes_bite_and_leave_lanes_and_envs_unfilled(oracle):
    for sc in (wide_scene(), narrow_scene()):
        f, _ = H.oracle_collide(oracle, sc)
        for bit in (STATIC, OUT_BOUND, OFF_LANE):
            assert 0.0 < ((f & bit) != 0).mean() < 1.0, (sc["A"], bit)
    n = narrow_scene()
    assert n["A"] == 5 and n["n_env"] % 32 == 5      # 8 slots per env: 32 envs per workgroup, the last one holds 5


def test_nonfinite_lanes_would_have_been_flagged(oracle):
    """the three lanes sit at contact in the finite scene (flags set); not finite, the oracle gives them no flag and nobody one on
    their account; and a NaN acceleration makes the oracle's own next position a NaN"""
    sc, a0, NONFINITE = nonfinite_scene()
    base, _ = H.oracle_collide(oracle, wide_scene())
    idx = np.array(sorted(NONFINITE.values()))
    assert (base[idx] != 0).all(), base[idx]
    parked = dict(sc); parked["x"] = sc["x"].copy(); parked["x"][NONFINITE["nan_action"]] = np.nan
    f, _ = H.oracle_collide(oracle, parked)
    assert (f[idx] == 0).all()
    rest = np.ones(len(f), bool); rest[idx] = False
    assert np.array_equal(f[rest], base[rest])      # (a cell holds one motif: nobody else's verdict hung on these three)
    i = NONFINITE["nan_action"]
    z = np.zeros(1, np.float32)
    o = oracle.integrate(sc["rows"], sc["x"][i:i + 1], sc["y"][i:i + 1], sc["heading"][i:i + 1], z, z, z, a0[i:i + 1], z,
                         sc["type_id"][i:i + 1], np.ones(1, np.uint8), 100)
    assert np.isnan(o[0, 0]) or np.isnan(o[0, 3]), o


def test_kat_and_structured_scenes_cover_overlap_nesting_and_reflex_corners(oracle):
    sc = kat_scene()
    f, _ = H.oracle_collide(oracle, sc)
    assert np.array_equal(f, sc["want"]), [n for n, a, b in zip(np.repeat(sc["names"], 3), f, sc["want"]) if a != b]
    for needle in ("overlapping lanes", "nested lanes", "reflex corner", "cuts the corner of two crossing roads"):
        assert any(needle in n for n in sc["names"]), needle
    st = structured_scene()
    g, _ = H.oracle_collide(oracle, st)
    assert 0.05 < ((g & OFF_LANE) != 0).mean() < 0.95
    assert H.count_vertices_in_but_not_contained(oracle, st, g) > 0     # bodies over a corner or a gap of the union


# ---- the scenes through every form of the step ---------------------------------------------------------------------------------------
def _run(sc, form, forms, variant, a0=None):
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc["n_env"], sc["A"])
    try:
        pool.set_param_table(sc["rows"])
        pool.set_static_geometry(sc["static"], sc["boundary"], sc["boundary_valid"])
        pool.set_lane_geometry(sc["lanes"])
        pool.set_status_config(check_dynamic=1, check_off_lane=1)
        z = np.zeros(sc["n_env"] * sc["A"], np.float32)
        pool.reset(sc["x"], sc["y"], sc["heading"], z, sc["type_id"], sc["active"])
        pool.set_integrator_variant(variant)
        pool.set_actions(z if a0 is None else a0, z)
        if forms[form] is None:
            assert pool.step_form(1) in ("step", "step_split"), pool.step_form(1)
            pool.step(100)
        else:
            pool.set_step_chaining(forms[form][0])
            pool.set_split_step(forms[form][1])
            assert pool.step_form(N_STEPS) == form, (pool.step_form(N_STEPS), form)
            pool.step_n(N_STEPS, 100, 0)
        pose = {name: pool.download(f) for f, name in ((L.F_X, "x"), (L.F_Y, "y"), (L.F_HEADING, "heading"))}
        return pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS), pose
    finally:
        pool.close()


def _check(oracle, name, sc, form, forms, variant, a0=None, frozen=True):
    gf, ge, pose = _run(sc, form, forms, variant, a0)
    if frozen and variant == "exact":   # zero speed, zero actions: the exact integrator stores the pose it was given
        for k in ("x", "y", "heading"):
            assert np.array_equal(pose[k].view(np.uint32), sc[k].view(np.uint32)), (name, form, k)
    wf, we = H.oracle_collide(oracle, dict(sc, **pose))
    bad = np.flatnonzero(gf != wf)
    assert bad.size == 0, (f"{name} {form} {variant}: {bad.size} participants differ, first {bad[:8].tolist()}: "
                           f"got {gf[bad[:8]].tolist()} want {wf[bad[:8]].tolist()}")
    assert np.array_equal(ge, we), (name, form)
    return gf, pose


@gpu
@pytest.mark.parametrize("variant", ["fast", "exact"])
@pytest.mark.parametrize("form", list(WIDE_FORMS))
def test_wide_pool_in_every_form_equals_the_oracle(oracle, form, variant):
    """(a), (b), (e) at A = 64: the contact scene with its last workgroup half empty, the four diamond scenes and the structured unions"""
    _check(oracle, "wide", wide_scene(), form, WIDE_FORMS, variant)
    if form == "chain_split":   # (the scenes below have lanes only: no such form for them)
        return
    for kind in ("box", "disc"):
        for which in ("one_cut", "one_clear"):
            _check(oracle, f"diamond {kind} {which}", diamond_scene(kind, which), form, WIDE_FORMS, variant)
    # (not `frozen`: a point mass at rest stores the heading of its zero velocity)
    _check(oracle, "structured", structured_scene(), form, WIDE_FORMS, variant, frozen=False)


@gpu
@pytest.mark.parametrize("variant", ["fast", "exact"])
@pytest.mark.parametrize("form", list(NARROW_FORMS))
def test_narrow_pools_in_every_form_equal_the_oracle(oracle, form, variant):
    """(a), (e) at A = 5 and A = 3: invalid lanes in every env, a last workgroup of 5 envs, the hand-built lane unions"""
    _check(oracle, "narrow", narrow_scene(), form, NARROW_FORMS, variant)
    gf, _ = _check(oracle, "kats", kat_scene(), form, NARROW_FORMS, variant)
    assert np.array_equal(gf, kat_scene()["want"])


@gpu
@pytest.mark.parametrize("variant", ["fast", "exact"])
@pytest.mark.parametrize("form", list(WIDE_FORMS))
def test_a_lane_that_is_not_finite_leaks_into_nobodys_flags(oracle, form, variant):
    """(c): flags of every participant equal the oracle's on the stored poses (a pose that is not finite takes no part: no flag of its
    own, nobody's partner); the three lanes end without a flag, and the lane with the NaN action has lost its position by then"""
    sc, a0, NONFINITE = nonfinite_scene()
    gf, pose = _check(oracle, "nonfinite", sc, form, WIDE_FORMS, variant, a0, frozen=False)
    idx = np.array(sorted(NONFINITE.values()))
    assert (gf[idx] == 0).all(), gf[idx]
    assert not np.isfinite(pose["x"][NONFINITE["nan_action"]]) or not np.isfinite(pose["y"][NONFINITE["nan_action"]])
    base, _ = H.oracle_collide(oracle, wide_scene())
    rest = np.ones(len(gf), bool); rest[idx] = False
    assert np.array_equal(gf[rest], base[rest])


# ---- (d) three steps of a mixed pool against the oracle's chain --------------------------------------------------------------------
def _mixed():
    def make():
        from tactics2d_amd import scenarios as S
        sc = S.mixed(6, 64, seed=5)
        rng = np.random.default_rng(17)
        odd = np.repeat(np.arange(sc.n_env) % 2 == 1, sc.A)    # every other env scattered: collisions, off-lane, out-of-bound at once
        sc.x = np.where(odd, sc.x + rng.normal(0, 1.5, sc.n), sc.x).astype(np.float32)
        sc.y = np.where(odd, sc.y + rng.normal(0, 1.0, sc.n), sc.y).astype(np.float32)
        sc.status.update(max_step=5)
        return sc
    return _cached("mixed", make)


def test_the_mixed_pool_ends_episodes_and_keeps_others_alive(oracle):
    """the oracle's own chain over the three steps: some envs end an episode (the auto-reset runs inside the fragment), some live
    through all of them (their last flags can be held against the stored poses)"""
    from test_gpu_chain_oracle import _oracle_env_chain, _ring
    sc = _mixed()
    r0, r1 = _ring(sc, N_STEPS, seed=3)
    vx = (sc.speed.astype(np.float64) * np.cos(sc.heading.astype(np.float64))).astype(np.float32)
    vy = (sc.speed.astype(np.float64) * np.sin(sc.heading.astype(np.float64))).astype(np.float32)
    ended = [any(st[2] or st[3] for st, _ in _oracle_env_chain(oracle, sc, e, r0, r1, vx, vy)[0]) for e in range(sc.n_env)]
    assert any(ended) and not all(ended), ended


MIXED_FORMS = [("step", 0, False), ("chain", 2, False), ("chain_split", 2, True), ("loop", 3, False), ("loop_pipe", 1, True)]


@gpu
@pytest.mark.parametrize("form,chaining,split", MIXED_FORMS, ids=[f[0] for f in MIXED_FORMS])
def test_three_steps_of_every_form_equal_the_oracle_chain(oracle, form, chaining, split):
    """exact integrator: per-step records (status bytes, reward), final state, flags, env flags, counters and status of EVERY env equal
    the oracle's own chain (integrate -> fp32 store -> collide -> status -> auto-reset); fast integrator: flags and env flags equal
    the oracle's verdict on the stored poses in every env the last step did not end"""
    from tactics2d_amd import layout as L
    from test_gpu_chain_oracle import _gpu_fragment, _oracle_env_chain, _ring
    sc = _mixed()
    r0, r1 = _ring(sc, N_STEPS, seed=3)
    start, got = _gpu_fragment(sc, r0, r1, chaining, split, form)
    ends = 0
    for e in range(sc.n_env):
        steps, fin = _oracle_env_chain(oracle, sc, e, r0, r1, start["vx"], start["vy"])
        sl = slice(e * sc.A, (e + 1) * sc.A)
        for k, (st, rw) in enumerate(steps):
            word = int(st[0]) | int(st[1]) << 8 | int(st[2]) << 16 | int(st[3]) << 24
            assert int(got["record"][k, e, 1]) == word, (form, e, k, hex(int(got["record"][k, e, 1])), hex(word))
            assert abs(float(got["record"][k, e, 0:1].view(np.float32)[0]) - float(rw)) <= 2e-6, (form, e, k)
            ends += int(st[2] or st[3])
        for f, key in ((L.F_X, "x"), (L.F_Y, "y"), (L.F_HEADING, "h"), (L.F_SPEED, "v")):
            assert np.array_equal(got[f][sl], fin[key]), (form, e, key)
        assert np.array_equal(got[L.F_FLAGS][sl], fin["flags"]), (form, e)
        assert got[L.F_ENV_FLAGS][e] == fin["env_flags"]
        assert got[L.F_CNT_STEP][e] == fin["cnt"] and got[L.F_FRAME_MS][e] == fin["frame"]
        assert np.array_equal(got[L.F_STATUS][e], steps[-1][0])
    assert ends > 0, "no episode ended: the auto-reset inside the fragment was not exercised"
    _, fast = _gpu_fragment(sc, r0, r1, chaining, split, form, variant="fast")
    st = np.ascontiguousarray(fast["record"][N_STEPS - 1, :, 1]).view(np.uint8).reshape(sc.n_env, 4)
    live = (st[:, 2] | st[:, 3]) == 0
    wf, we = oracle.collide(sc.rows, sc.n_env, sc.A, fast[L.F_X], fast[L.F_Y], fast[L.F_HEADING], sc.type_id, sc.active,
                            sc.static, sc.boundary, sc.boundary_valid, sc.lanes, 1)
    bad = (wf != fast[L.F_FLAGS]) & np.repeat(live, sc.A)
    assert not bad.any(), (form, int(bad.sum()), np.nonzero(bad)[0][:8])
    assert np.array_equal(we[live], fast[L.F_ENV_FLAGS][live]), form
    assert live.any() and (fast[L.F_FLAGS][np.repeat(live, sc.A)] != 0).any(), form
