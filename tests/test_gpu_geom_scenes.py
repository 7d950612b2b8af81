"""Contact-dense scenes (tests/geom_scenes.py) through the real event kernels: flags and env words bit-exact against the oracle where
the certifying filters answer `undecided` and sat_quads has the last word -- every pair-stage path, the fused step and the event-only
call, the LDS record and the HBM grid tier, the general kernel and the wave-per-env ego kernel -- and the IoU of the status epilogue at
contact, bit for bit.  The tests not marked gpu check, with the oracle and exact rational arithmetic, that the scenes are what they
claim to be; tests/test_geom_cases.py does the same for the predicate arrays.
"""
import numpy as np
import pytest

import geom_scenes as GS
import helpers as H
import test_geom_cases as TC

gpu = pytest.mark.gpu

# the pair-stage paths of tests/test_gpu_collide.py::test_flags_bit_exact at their smallest: wave = env; two envs per wave; grid,
# geometry from global; brute-force pairs; A_pad = 256
SHAPES = [(64, 64), (96, 32), (40, 8), (60, 4), (3, 200)]
MAP_SHAPES = SHAPES + [(64, 1)]          # (64, 1): the wave-per-env ego kernel (tests/test_gpu_ego.py)
FAR_LANES = 200                          # extra lane polygons 300 m away that push every MAP_SHAPES scene into the HBM grid tier


def _undecided_share(oracle, sc):
    PA, PB = GS.pair_vertices(oracle, sc)
    v = TC.rect_pair_filter_np(PA, PB)
    return float((v == 2).mean()), PA, PB, v


# ---- the scenes are what they say (CPU) ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_env,A", SHAPES)
def test_pair_scenes_are_saturated_or_mixed_and_bite(oracle, n_env, A):
    """saturated: >= 50 % of the neighbouring box pairs undecided for the restated rect_pair_filter on the oracle's vertices; mixed:
    between 5 % and 50 %.  Either way the filter never contradicts the oracle, the dynamic bit is set for 10 .. 90 % of the
    participants, and >= 20 % of the contact pairs are hits BECAUSE closed sets that touch intersect: their exact-rational gap is 0"""
    for kind in ("saturated", "mixed"):
        sc = GS.pair_scene(oracle, n_env, A, kind)
        share, PA, PB, v = _undecided_share(oracle, sc)
        truth = oracle.geom("sat_quads", PA, PB) != 0
        assert not ((v != 2) & ((v == 1) != truth)).any()
        assert share >= 0.5 if kind == "saturated" else 0.05 <= share <= 0.5, (kind, share)
        f, _ = H.oracle_collide(oracle, sc)
        assert 0.1 <= ((f & 1) != 0).mean() <= 0.9
        # the pair's own verdict is the participants' flag: nothing of another cell reaches them
        assert np.array_equal((f[sc["pairs"][:, 0]] & 1) != 0, truth) and np.array_equal((f[sc["pairs"][:, 1]] & 1) != 0, truth)
        c = np.flatnonzero(sc["contact"])
        step = max(1, len(c) // 150)
        touch = [TC.exact_gap_is_zero(PA[i], PB[i]) for i in c[::step]]
        assert np.mean(touch) >= 0.2, np.mean(touch)
        assert all(truth[i] for i, t in zip(c[::step], touch) if t)
        # discs: tangent ones are there, and they hit
        m = sc["motif"]
        assert all((m == k).any() for k in ("disc_disc", "disc_side", "disc_corner")) or A < 32
        # zero speed and zero actions leave every pose bit-identical: the fused step sees the uploaded scene
        z = np.zeros(n_env * A, np.float32)
        oracle.set_trig(1)
        o = oracle.integrate(sc["rows"], sc["x"], sc["y"], sc["heading"], z, None, None, z, z, sc["type_id"], sc["active"], 100)
        oracle.set_trig(0)
        for k, name in enumerate(("x", "y", "heading")):
            assert np.array_equal(np.float32(o[:, k]).view(np.uint32), sc[name].view(np.uint32)), name


@pytest.mark.parametrize("n_env,A", MAP_SHAPES)
def test_map_scenes_bite_and_reach_both_tiers(oracle, n_env, A):
    """static, out-of-bound and off-lane bits each set for 10 .. 90 % of the participants; every motif present (all of them over the
    shapes with A >= 32); the far lanes change no flag and push the scene out of the LDS record"""
    from tactics2d_amd import mapgeom as MG
    sc = GS.map_scene(n_env, A)
    f, _ = H.oracle_collide(oracle, sc)
    for bit in (2, 4, 8):
        assert 0.1 <= ((f & bit) != 0).mean() <= 0.9, (bit, ((f & bit) != 0).mean())
    if A >= 32:
        assert {"boundary", "static_vertex", "static_edge", "static_centre_on_edge", "lane_inside", "lane_outside",
                "lane_across_shared_side", "lane_centre_on_outline"} <= set(sc["motif"])
    # contact decides: the same motif gives both verdicts
    for m, bit in (("static_vertex", 2), ("static_edge", 2), ("boundary", 4), ("lane_inside", 8)):
        r = ((f[sc["motif"] == m] & bit) != 0).mean() if (sc["motif"] == m).sum() > 20 else 0.5
        assert 0.05 < r < 0.95, (m, r)
    far = GS.map_scene(n_env, A, far_lanes=FAR_LANES)
    assert np.array_equal(H.oracle_collide(oracle, far)[0], f)
    assert MG.geometry_budget(n_env, A, static=sc["static"], lanes=sc["lanes"])["fits"]
    assert not MG.geometry_budget(n_env, A, static=far["static"], lanes=far["lanes"])["fits"]
    vo = sc["static"][1]
    assert set(np.diff(vo)) == set(range(3, 9)) or A < 32
    if A == 1:       # the variant the wave-per-env ego kernel takes: boxes only, no lanes
        ego = GS.map_scene(n_env, A, ego=True)
        fe, _ = H.oracle_collide(oracle, ego)
        assert ego["lanes"] is None and (ego["rows"][:, 18] == 0).all()
        for bit in (2, 4):
            assert 0.1 <= ((fe & bit) != 0).mean() <= 0.9, (bit, ((fe & bit) != 0).mean())


# ---- through the kernels -----------------------------------------------------------------------------------------------------
def _gpu_flags(sc, how, ego_kernel=None):
    """how = "collide": the event-only call; "step": the fused step at zero speed and zero actions (the stored pose is the uploaded
    one: checked above with the oracle's integrator, and below on the downloaded state)"""
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
        if ego_kernel is not None:
            pool.set_ego_kernel(ego_kernel)
        form = pool.step_form(1)
        if how == "collide":
            pool.collide()
        else:
            pool.set_integrator_variant("exact")
            pool.set_actions(z, z)
            pool.step(100)
            for fld, name in ((L.F_X, "x"), (L.F_Y, "y"), (L.F_HEADING, "heading")):
                assert np.array_equal(pool.download(fld).view(np.uint32), sc[name].view(np.uint32)), name
        return pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS), form
    finally:
        pool.close()


def _assert_flags(got, want, sc, what):
    (gf, ge, form), (wf, we) = got, want
    bad = np.flatnonzero(gf != wf)
    assert bad.size == 0, (f"{what} ({form}): {bad.size} participants differ, motifs {sorted(set(sc['motif'][bad]))}; first {bad[:8].tolist()}: "
                           f"got {gf[bad[:8]].tolist()} want {wf[bad[:8]].tolist()}")
    assert np.array_equal(ge, we), what


@gpu
@pytest.mark.parametrize("kind", ["saturated", "mixed"])
@pytest.mark.parametrize("n_env,A", SHAPES)
def test_pair_scenes_flags_are_bit_exact_in_the_event_call_and_the_fused_step(oracle, n_env, A, kind):
    sc = GS.pair_scene(oracle, n_env, A, kind)
    want = H.oracle_collide(oracle, sc)
    _assert_flags(_gpu_flags(sc, "collide"), want, sc, "t2d_collide")
    _assert_flags(_gpu_flags(sc, "step"), want, sc, "t2d_step")


@gpu
@pytest.mark.parametrize("tier", ["lds_record", "hbm_grid"])
@pytest.mark.parametrize("n_env,A", MAP_SHAPES)
def test_map_scenes_flags_are_bit_exact_in_both_tiers(oracle, n_env, A, tier):
    sc = GS.map_scene(n_env, A, far_lanes=FAR_LANES if tier == "hbm_grid" else 0)
    want = H.oracle_collide(oracle, sc)
    _assert_flags(_gpu_flags(sc, "collide"), want, sc, "t2d_collide")
    got = _gpu_flags(sc, "step")
    _assert_flags(got, want, sc, "t2d_step")
    if tier == "hbm_grid":
        assert got[2] == "unfused"
    if A == 1 and tier == "lds_record":
        # statics and the boundary through the wave-per-env ego kernel (boxes only, no lanes), and the same pool on the general one
        ego = GS.map_scene(n_env, A, ego=True)
        want = H.oracle_collide(oracle, ego)
        got = _gpu_flags(ego, "step", ego_kernel=True)
        assert got[2].startswith("ego"), got[2]
        _assert_flags(got, want, ego, "t2d_step, ego kernel")
        got = _gpu_flags(ego, "step", ego_kernel=False)
        assert got[2] == "step", got[2]
        _assert_flags(got, want, ego, "t2d_step, general kernel")


@gpu
@pytest.mark.parametrize("A,ego_kernel", [(1, True), (1, False), (4, None)])
def test_iou_of_the_status_epilogue_at_contact_equals_the_oracle_bit_for_bit(oracle, A, ego_kernel):
    """egos on, beside and identical to their targets (tests/geom_scenes.py iou_scene), two steps at zero speed: T2D_F_IOU is
    float32(t2do_quad_iou(pose, target)) -- the same arithmetic on both sides, so the same bits -- and the status words are the
    oracle's (the second step's NoAction IoU is the pose against itself)"""
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    n_env = 112
    ex, ey, eh, tgt, case = GS.iou_scene(n_env, A)
    N = n_env * A
    x = np.zeros(N, np.float32); y = np.zeros(N, np.float32); h = np.zeros(N, np.float32)
    ego = np.arange(n_env) * A
    x[ego], y[ego], h[ego] = ex, ey, eh
    active = np.zeros(N, np.uint8); active[ego] = 1
    tid = np.zeros(N, np.uint8); z = np.zeros(N, np.float32)
    rows = GS.iou_rows()
    status = dict(max_step=50, check_arrival=1, check_no_action=1, no_action_max_step=100, shaped_reward=1)
    pool = ParticipantPool(n_env, A)
    try:
        pool.set_param_table(rows)
        pool.set_target_areas(tgt)
        pool.set_status_config(**status)
        pool.reset(x, y, h, z, tid, active)
        pool.snapshot()
        pool.set_integrator_variant("exact")
        if ego_kernel is not None:
            pool.set_ego_kernel(ego_kernel)
        cfg = oracle.make_config(**status)
        ep = oracle.EpisodeState(n_env, tgt, None, np.stack([ex, ey], 1))
        cnt = np.zeros(n_env, np.int32); frame = np.zeros(n_env, np.int32)
        for t in range(2):
            form = pool.step_form(1)
            pool.set_actions(z, z)
            pool.step(100)
            wf, _ = oracle.collide(rows, n_env, A, x, y, h, tid, active, None, None, None, None, 0)
            wst, wrw, wiou = oracle.status_ex(cfg, A, wf, 100, cnt, frame, rows, x, y, h, tid, ep)
            giou, gst = pool.download(L.F_IOU), pool.download(L.F_STATUS)
            assert np.array_equal(pool.download(L.F_X), x) and np.array_equal(pool.download(L.F_HEADING), h)
            bad = np.flatnonzero(giou.view(np.uint32) != wiou.view(np.uint32))
            assert bad.size == 0, (form, t, sorted(set(case[bad])), giou[bad[:6]].tolist(), wiou[bad[:6]].tolist())
            assert np.array_equal(gst, wst), (form, t, sorted(set(case[np.flatnonzero((gst != wst).any(1))])))
            assert np.array_equal(pool.download(L.F_CNT_NO_ACTION), ep.cnt_na)
            if t == 0:
                # the cases are what they say, for the oracle whose exact-arithmetic check is tests/test_geom_cases.py
                for name, val in (("identical", 1.0), ("shared_side_front", 0.0), ("shared_side_left", 0.0), ("shared_side_rear", 0.0),
                                  ("shared_side_right", 0.0), ("shared_corner", 0.0), ("apart", 0.0), ("nested", np.float32(2 / 4.5)),
                                  ("shifted_along_side", np.float32(7 / 9)), ("cross", np.float32(1 / 3))):
                    assert (wiou[case == name] == np.float32(val)).all(), (name, wiou[case == name][:4])
                assert (wst[case == "identical", 0] == 2).all()          # arrived
        if ego_kernel is True:
            assert form.startswith("ego"), form
    finally:
        pool.close()
