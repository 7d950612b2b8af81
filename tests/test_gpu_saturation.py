"""The step kernel with its per-wave candidate queues SATURATED (tests/saturation_scenes.py; tests/test_saturation_scenes.py holds the
scenes' preconditions): waves with several times kQueueCap candidates, so that compact_and_process goes round two to seven times
and lanes emit part of their entries (n_emit < cnt) and keep the rest -- in the ring caller of the pair stage and both callers of
sweep_stage, across the half-words and 64-box chunks of box_sweep and its remainder loop -- and hash-grid buckets with chains of
tens of participants.  Flags and env words must equal the oracle's brute-force fp64 evaluation on the fp32 poses the kernel stored,
bit for bit: every contact of these scenes is the only one of its participants, a lost queue entry is a wrong flag.

Events only (t2d_collide) on every scene, shape and seed; t2d_step with both integrators at zero speed and zero actions; t2d_step_n
of three steps through loop_pipe, loop, chain_split and chain.  Auto-reset stays off: a finished env keeps its flags.

Slat counts K run over {1, 3, 4, 5, 31, 32, 33, 63, 64, 65, 130} at A in {1, 4, 16, 64, 100}, less those whose geometry does not fit
the 32 KiB LDS record (they would run on the HBM grid tier, other kernels): static K >= 31 at A = 1 and K >= 63 at A = 4; lanes
K >= 5 at A = 1, K >= 31 at A = 4, K >= 63 at A = 16 (saturation_scenes.SLAT_FITS; test_saturation_scenes.py asserts `fits` for
every case and `not fits` for one dropped case per stage).  An env of one agent takes two lanes, so a wave holds 32 of them and no
A = 1 case that fits saturates: those are there for the sweep's remainder loops.  In the combined scene 64 lanes cannot carry three
capacities in all three stages at once (44 needles for 946 pairs leave 20 boxes): 64 x 64 has 3.3 / 2.4 / 3.9 capacities in pairs /
statics / lanes, 64 x 16 has 1.1 / 2.0 / 2.7.  These counts are per call of compact_and_process: sweep_stage makes one per 64-box
chunk of an env's polygon list, so at K = 130 the ~24 slats in reach of a box spread over three calls (450 to 1100 entries a wave in
each of the first two, 721 at the least in the fuller, about 20 in the third: the chunk loop with two to four rounds inside), at K = 65 over two (1435 and more, and a few), and the
split form gives each half of the lane list a wave and a queue of its own (about 770 entries each).
"""
import numpy as np
import pytest

import helpers as H
import saturation_scenes as S

pytestmark = pytest.mark.gpu
_oracle_cache = {}


def _want(oracle, key, sc):
    """the oracle's flags and env words on the scene's uploaded poses, once per (case, seed)"""
    if key not in _oracle_cache:
        _oracle_cache[key] = H.oracle_collide(oracle, sc)
    return _oracle_cache[key]


def _pool(sc, variant="exact"):
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc["n_env"], sc["A"])
    try:
        pool.set_param_table(sc["rows"])
        pool.set_static_geometry(sc["static"], None, None)
        pool.set_lane_geometry(sc["lanes"])
        pool.set_status_config(check_dynamic=1, check_off_lane=1)
        pool.set_auto_reset(False)
        z = np.zeros(sc["n_env"] * sc["A"], np.float32)
        pool.reset(sc["x"], sc["y"], sc["heading"], z, sc["type_id"], sc["active"])
        pool.set_integrator_variant(variant)
        pool.set_actions(z, z)
    except Exception:
        pool.close()
        raise
    return pool


def _download(pool):
    from tactics2d_amd import layout as L
    pose = {name: pool.download(f) for f, name in ((L.F_X, "x"), (L.F_Y, "y"), (L.F_HEADING, "heading"))}
    return pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS), pose


def _same_poses(pose, sc):
    return all(np.array_equal(pose[k].view(np.uint32), sc[k].view(np.uint32)) for k in ("x", "y", "heading"))


def _check(oracle, label, key, sc, got, must_keep_poses, tile=1):
    """flags and env words against the oracle on the stored poses (`tile`: the pool is that many copies of the scene)"""
    gf, ge, pose = got
    big = S.tiled(sc, tile) if tile > 1 else sc
    kept = _same_poses(pose, big)
    if must_keep_poses:
        assert kept, f"{label}: the stored poses differ from the uploaded ones"
    if kept:
        wf, we = _want(oracle, key, sc)
        wf, we = np.tile(wf, tile), np.tile(we, tile)
    else:
        wf, we = H.oracle_collide(oracle, dict(big, **pose))
    bad = np.flatnonzero(gf != wf)
    A = sc["A"]
    assert bad.size == 0, (f"{label}: {bad.size} participants differ; first (env, agent) {[(int(b) // A, int(b) % A) for b in bad[:8]]}: "
                           f"got {gf[bad[:8]].tolist()} want {wf[bad[:8]].tolist()}")
    assert np.array_equal(ge, we), f"{label}: env words differ in envs {np.flatnonzero(ge != we)[:8].tolist()}"
    return kept


# ---------------------------------------------------------------------------------------------------------------- events only
@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_events_only(oracle, case):
    """t2d_collide on the uploaded poses (stored poses == uploaded, bitwise): every scene, shape and seed"""
    for seed in case.seeds:
        sc = case.scene(seed)
        pool = _pool(sc)
        try:
            pool.collide()
            got = _download(pool)
        finally:
            pool.close()
        _check(oracle, f"{case} seed {seed} events only", (case.name, seed), sc, got, True)


# ------------------------------------------------------------------------------------------------------------------- t2d_step
@pytest.mark.parametrize("variant", ["exact", "fast"])
@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_step(oracle, case, variant):
    """one fused step at zero speed and zero actions: `step`, or `step_split` (pair stage and lane halves on waves of their own,
    each with its queue) where a pool of 64-agent envs has lanes.  exact stores the uploaded poses; fast is held against the oracle
    on what it stored."""
    for seed in case.seeds[:3]:
        sc = case.scene(seed)
        pool = _pool(sc, variant)
        try:
            form = pool.step_form(1)
            assert form == ("step_split" if case.has_lanes and sc["A"] == 64 else "step"), (case, form)
            pool.step(100)
            got = _download(pool)
        finally:
            pool.close()
        _check(oracle, f"{case} seed {seed} t2d_step {variant} ({form})", (case.name, seed), sc, got, variant == "exact")


# ----------------------------------------------------------------------------------------------------------------- t2d_step_n
def _step_n(oracle, label, key, sc, variant, form, chaining=None, split=None, tile=1):
    """collide, then three chained steps on one pool: both must give the oracle's flags, and the same flags.  At zero speed and zero
    actions either integrator stores the pose it read (x + 0 * cos, heading + 0): asserted for fast as for exact, so the comparison
    of the two launches is never passed over."""
    big = S.tiled(sc, tile) if tile > 1 else sc
    pool = _pool(big, variant)
    try:
        if split is not None:
            pool.set_split_step(split)
        if chaining is not None:
            pool.set_step_chaining(chaining)
        got_form = pool.step_form(3)
        if got_form != form:
            return got_form
        pool.collide()
        events = _download(pool)
        pool.step_n(3, 100, 0)
        got = _download(pool)
    finally:
        pool.close()
    _check(oracle, f"{label} events only", key, sc, events, True, tile)
    _check(oracle, f"{label} t2d_step_n {variant} ({form})", key, sc, got, True, tile)
    assert np.array_equal(got[0], events[0]) and np.array_equal(got[1], events[1]), f"{label}: flags after the last step differ from the events-only launch"
    return form


STEP_N_CASES = [c for c in S.CASES if "step_n" in c.runs]


@pytest.mark.parametrize("variant", ["exact", "fast"])
@pytest.mark.parametrize("form", ["loop_pipe", "loop", "chain_forced"])
@pytest.mark.parametrize("case", STEP_N_CASES, ids=repr)
def test_step_n_small_pool_forms(oracle, case, form, variant):
    """the combined scene through the multi-step forms of a small pool.  loop_pipe: integrator waves a step ahead, and (the scene
    has five and more lane polygons per env) lane waves with queues of their own -- PIPE 2.  loop: set_step_chaining(3), with the
    one-workgroup-per-env form switched off (a 64-agent pool with statics and lanes would chain per env instead).  chain_forced:
    set_step_chaining(2) -- chain_split for 64-agent envs, the plain chain for 16-agent envs, which have no split form."""
    name = {"loop_pipe": "loop_pipe", "loop": "loop", "chain_forced": "chain_split" if "x64" in case.name else "chain"}[form]
    kw = {"loop_pipe": {}, "loop": dict(chaining=3, split=False), "chain_forced": dict(chaining=2)}[form]
    for seed in case.seeds[:3]:
        sc = case.scene(seed)
        got = _step_n(oracle, f"{case} seed {seed}", (case.name, seed), sc, variant, name, **kw)
        assert got == name, (case, form, got)


@pytest.mark.parametrize("case", [c for c in S.CASES if c.name in ("needles_64x64", "needles_64x16")], ids=repr)
def test_step_n_loop_pipe_without_lanes(oracle, case):
    """no lanes: loop_pipe is PIPE 1 (integrator waves only); the pair stage's queue goes round seven times (64 x 64), twice (64 x 16)"""
    sc = case.scene(0)
    assert _step_n(oracle, f"{case} seed 0", (case.name, 0), sc, "fast", "loop_pipe") == "loop_pipe"


@pytest.mark.parametrize("A", [64, 16])
def test_step_n_chained_large_pool(oracle, A):
    """`chain` as large pools take it by themselves: 8 distinct envs of the combined scene tiled to the smallest pool (of 520, 1032,
    2056, ... envs: past twice the 256 compute units in workgroups) whose three steps chain; the oracle's answer for the 8, tiled"""
    sc = S.combined_scene(8, A, seed=0)
    tried = {}
    for n_env in (520, 1032, 2056, 4104, 8200):
        tried[n_env] = _step_n(oracle, f"combined 8 x {A} tiled to {n_env}", ("combined_tile", A), sc, "exact", "chain", tile=n_env // 8)
        if tried[n_env] == "chain":
            return
    pytest.fail(f"no pool size took the chained form: {tried}")
