"""The step kernel after its instruction diet: sweep verdicts read off a sign bit, ring-queue entries ordered by the
narrow phase, filters fed from three vertices and the stored centre, the point mass reusing its speed.  Flags must stay the oracle's on
the kernel's own stored poses, bit for bit, where poses sit in contact and an fp32 ulp (~1e-7 m at these coordinates) either side of
it.  Two invariance tests ride along for code this change left as it was: lanes of a dynamics wave do not depend on whether another
lane of the wave reaches its speed bound, and poses at a safe rectangle's edge get the oracle's flags.

Scenes come from tests/geom_scenes.py (the constructions of tests/test_gpu_geom_scenes.py) at the shapes that pick the sweep's paths:
8 x 64 the unrolled ring (log2A = 6), 8 x 16 batches of four offset pairs, 8 x 4 batches of one, 8 x 2 the single partner.
"""
import numpy as np
import pytest

import geom_scenes as GS
import helpers as H
from test_oracle_geometry import _kernel_pose_box, _safe_rects

gpu = pytest.mark.gpu

SHAPES = [(8, 64), (8, 16), (8, 4), (8, 2)]
TOL = 1e-5   # the north-star tolerance of tests/test_gpu_physics.py (fp32 pose state, abs)


# ---- a lane rectangle and poses on, inside, outside and across the edge of its safe rectangle -------------------------------------
LANE = np.float32([[-1.0, -9.0], [1.0, -9.0], [1.0, 9.0], [-1.0, 9.0]])
BOX_L, BOX_W = GS.BOXES[0]           # 0.25 x 0.125, heading 0: the pose's extent in x is x -+ 0.125 exactly


def _edge_poses():
    """fp32 x of a heading-0 box whose kernel pose box (outward rounded) ends ON the safe rectangle's xmax (the certificate's
    m = 0), the neighbouring fp32 values either side (m < 0: certified; m > 0: not), and one across the lane's own edge (off-lane).
    The rectangle is the library's own (t2d_lane_safe_rects: the host routine t2d_set_lane_geometry runs, through the C ABI); the
    pose box is the restatement of tests/test_oracle_geometry.py.  What this cannot show: the first three poses lie 0.1 mm inside
    the lane, so they are not off-lane whichever path decides -- a certificate that wrongly covered the `outside` pose would give
    the same flags.  The scene checks that poses at the edge get the oracle's flags, not which path gave them."""
    xmax = _safe_rects([LANE])[0, 1]
    x = np.float32(xmax - np.float32(BOX_L / 2))
    hi = lambda v: _kernel_pose_box(np.float64(v) - BOX_L / 2, np.float64(v) + BOX_L / 2, 0.0, 0.0)[1]
    for _ in range(64):      # walk down until the rounded box no longer sticks out ...
        if hi(x) <= xmax:
            break
        x = np.nextafter(x, np.float32(-np.inf))
    on = x
    assert hi(on) == xmax, (hi(on), xmax)
    inside, outside = np.nextafter(on, np.float32(-np.inf)), np.nextafter(on, np.float32(np.inf))
    assert hi(inside) < xmax < hi(outside)
    return np.float32([on, inside, outside, 1.0 - BOX_L / 4]), xmax


def safe_scene(n_env, A):
    xs, _ = _edge_poses()
    k = np.arange(n_env * A)
    y = np.float32(-8.0 + 0.25 * (k % A))              # 0.125 wide, 0.25 apart: nobody touches anybody
    sc = dict(rows=GS.rows(), n_env=n_env, A=A, x=xs[(k + k // A) % 4], y=y, heading=np.zeros(n_env * A, np.float32),
              type_id=np.zeros(n_env * A, np.uint8), active=np.ones(n_env * A, np.uint8), static=None,
              lanes=H.to_csr([[LANE]] * n_env), boundary=None, boundary_valid=None,
              motif=np.array(["safe_on_edge", "safe_inside", "safe_outside", "across_lane_edge"], dtype=object)[(k + k // A) % 4])
    return sc


def test_safe_rectangle_poses_sit_on_and_either_side_of_the_edge(oracle):
    xs, xmax = _edge_poses()
    assert np.float32(xmax) < 1.0 and xs[0] < xs[2] and xs[1] < xs[0]
    sc = safe_scene(2, 4)
    f, _ = H.oracle_collide(oracle, sc)
    off = (f & 8) != 0
    assert np.array_equal(off, sc["motif"] == "across_lane_edge")


@pytest.mark.parametrize("n_env,A", SHAPES)
def test_scenes_bite_at_every_shape(oracle, n_env, A):
    """every scene of the GPU test sets its bit for some participants and not for others (contact decides)"""
    for sc, bit in ((GS.pair_scene(oracle, n_env, A, "saturated"), 1), (GS.map_scene(n_env, A), 2), (GS.map_scene(n_env, A), 8),
                    (safe_scene(n_env, A), 8)):
        f, _ = H.oracle_collide(oracle, sc)
        share = ((f & bit) != 0).mean()
        assert 0.0 < share < 1.0, (bit, share)


# ---- sweeps and filters through t2d_step ---------------------------------------------------------------------------------------------
def _step_flags_and_poses(sc, variant):
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
        pool.set_actions(z, z)
        assert pool.step_form(1) in ("step", "step_split"), pool.step_form(1)
        pool.step(100)
        pose = {name: pool.download(f) for f, name in ((L.F_X, "x"), (L.F_Y, "y"), (L.F_HEADING, "heading"))}
        return pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS), pose
    finally:
        pool.close()


@gpu
@pytest.mark.parametrize("variant", ["fast", "exact"])
@pytest.mark.parametrize("n_env,A", SHAPES)
def test_flags_equal_the_oracle_on_the_stored_poses_at_contact(oracle, n_env, A, variant):
    """pairs (boxes and discs mixed) in contact and ulps either side of it; boxes and discs on static polygons, on the lane
    outline and on the boundary rectangle; boxes on, inside and outside a safe rectangle's edge: oracle.collide on the poses the
    kernel stored equals the kernel's flags and env words exactly.  At zero speed and zero actions the exact integrator stores
    the uploaded pose (checked: the constructions are what the kernel sees)."""
    scenes = [("pairs", GS.pair_scene(oracle, n_env, A, "saturated")), ("pairs_mixed", GS.pair_scene(oracle, n_env, A, "mixed")),
              ("map", GS.map_scene(n_env, A)), ("safe_rectangle", safe_scene(n_env, A))]
    for name, sc in scenes:
        gf, ge, pose = _step_flags_and_poses(sc, variant)
        if variant == "exact":
            for k in ("x", "y", "heading"):
                assert np.array_equal(pose[k].view(np.uint32), sc[k].view(np.uint32)), (name, k)
        wf, we = H.oracle_collide(oracle, dict(sc, **pose))
        bad = np.flatnonzero(gf != wf)
        assert bad.size == 0, (f"{name} {n_env} x {A} {variant}: {bad.size} participants differ, motifs {sorted(set(sc['motif'][bad]))}; "
                               f"first {bad[:8].tolist()}: got {gf[bad[:8]].tolist()} want {wf[bad[:8]].tolist()}")
        assert np.array_equal(ge, we), name


# ---- dynamics: a lane on its bound changes nothing for the others -------------------------------------------------------------------
def _highway_wave():
    """one highway env of 64 SingleTrackDynamics lanes (speeds 20 .. 35 m/s), lane 0 moved to 0.05 m/s below its type's speed bound"""
    from tactics2d_amd import layout as L, scenarios as S
    sc = S.highway(1, 64, seed=1)
    rows = sc.rows[sc.type_id]
    assert (rows[:, L.P_MODEL] == L.MODEL_DYNAMICS).all() and sc.active.all()
    assert (rows[:, L.P_RANGE_FLAGS].astype(int) & L.RANGE_SPEED).all()
    hi, lo = rows[:, L.P_SPEED_HI], rows[:, L.P_SPEED_LO]
    speed = sc.speed.copy()
    speed[0] = np.float32(hi[0] - 0.05)
    a0 = np.zeros(64, np.float32)
    a1 = np.float32(np.random.default_rng(3).normal(0.0, 0.02, 64))
    a0[1:] = np.float32(np.random.default_rng(4).uniform(-3.0, 2.0, 63))
    # lanes 1 .. 63 stay a metre per second and more inside their bounds over three steps of 0.1 s at |a| <= 3
    assert ((speed[1:] + 1.0 < hi[1:]) & (speed[1:] - 1.0 > lo[1:])).all()
    acc_hi = rows[0, L.P_ACCEL_HI] if int(rows[0, L.P_RANGE_FLAGS]) & L.RANGE_ACCEL else 2.0
    assert min(acc_hi, 2.0) * 0.1 > 0.05 + 1e-3      # run A: lane 0 reaches the bound inside the first step
    return sc, speed, a0, a1


def _run_dynamics(sc, speed, a0, a1, n_steps):
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(1, 64)
    try:
        sc.load(pool)
        pool.reset(sc.x, sc.y, sc.heading, speed, sc.type_id, sc.active)
        pool.set_integrator_variant("fast")
        pool.set_actions(a0, a1)
        if n_steps == 1:
            pool.step(sc.interval_ms)
        else:
            pool.step_n(n_steps, sc.interval_ms, 0)
        return np.stack([pool.download(f).view(np.uint32) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_FLAGS)], 1)
    finally:
        pool.close()


@gpu
@pytest.mark.parametrize("n_steps", [1, 3])
def test_dynamics_lanes_do_not_depend_on_the_clamp_path_of_their_wave(n_steps):
    """An invariance test (the dynamics loop is the parent's): run A, lane 0 accelerates into its speed bound; run B, lane 0 holds
    its speed and nobody reaches a bound.  Lanes 1 .. 63 have the same inputs in both runs: the same bits come out, after one step
    and after a chained fragment of three -- what any wave-uniform short cut round the clamp would have to keep."""
    from tactics2d_amd import layout as L
    sc, speed, a0, a1 = _highway_wave()
    a0_a = a0.copy(); a0_a[0] = 2.0
    A = _run_dynamics(sc, speed, a0_a, a1, n_steps)
    B = _run_dynamics(sc, speed, a0, a1, n_steps)
    hi0 = np.float32(sc.rows[sc.type_id[0], L.P_SPEED_HI])
    assert A[0, 3].view(np.float32) == hi0, "run A: lane 0 ends on its bound"
    assert B[0, 3].view(np.float32) < hi0, "run B: lane 0 stays below it"
    assert np.array_equal(A[1:], B[1:]), np.flatnonzero((A[1:] != B[1:]).any(1))[:8] + 1


# ---- point mass: the unclipped branch reuses the speed it already has ------------------------------------------------------------
@gpu
def test_pointmass_step_clipped_and_unclipped_equals_the_oracle_bit_for_bit(oracle):
    """64 point masses of the committed fixture (tests/golden/pm_random.npz) in one env, 32 whose new speed leaves the type's range
    (the clipped branch) and 32 whose does not, through t2d_step, fast variant: within 1e-5 of the reference's result, and the
    bits of the oracle (sqrt of the same sum of the same squares: what the kernel stored before it reused the value)."""
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    d = H.load_npz("pm_random.npz")
    iv = int(np.bincount(d["timing"][:, 0].astype(int)).argmax())
    m = np.flatnonzero(d["timing"][:, 0] == iv)
    rows = np.asarray(d["rows"], np.float64)
    r = rows[d["type_id"][m]]
    st, ac = np.float64(np.float32(d["state"][m])), np.float64(np.float32(d["action"][m]))
    ns = np.hypot(st[:, 2] + ac[:, 0] * iv / 1000.0, st[:, 3] + ac[:, 1] * iv / 1000.0)
    ranged = (r[:, L.P_RANGE_FLAGS].astype(int) & L.RANGE_SPEED) != 0
    margin = 1e-6
    clipped = ranged & ((ns < r[:, L.P_SPEED_LO] - margin) | (ns > r[:, L.P_SPEED_HI] + margin))
    free = ~ranged | ((ns > r[:, L.P_SPEED_LO] + margin) & (ns < r[:, L.P_SPEED_HI] - margin))
    sel = np.concatenate([m[clipped][:32], m[free][:32]])
    assert len(sel) == 64, (clipped.sum(), free.sum())
    types = np.unique(d["type_id"][sel])
    assert len(types) <= 32
    tid = np.searchsorted(types, d["type_id"][sel]).astype(np.uint8)
    s, a = np.float32(d["state"][sel]), np.float32(d["action"][sel])
    pool = ParticipantPool(1, 64)
    try:
        pool.set_param_table(rows[types])
        pool.set_integrator_variant("fast")
        z = np.zeros(64, np.float32)
        pool.reset(s[:, 0], s[:, 1], z, z, tid, vx=s[:, 2], vy=s[:, 3])
        pool.set_actions(a[:, 0], a[:, 1])
        pool.step(iv)
        got = np.stack([pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY)], 1)
    finally:
        pool.close()
    err = H.state_err(got, d["out"][sel], cols=6)
    print("pointmass through t2d_step, fast: max abs err", err.max(0))
    assert err.max() <= TOL, err.max(0)
    want = np.float32(H.oracle_physics(oracle, rows[types], tid, s, a, iv, "pm", trig=1))[:, :6]
    bad = (got.view(np.uint32) != want.view(np.uint32)) & ~((got == 0) & (want == 0))
    assert not bad.any(), (np.argwhere(bad)[:8].tolist(), got[bad][:4], want[bad][:4])
