"""Every wave-uniform path of the fast integrators, reached on purpose (tests/fast_paths.py builds the scenes wave by wave and
names each wave's path; tests/test_fast_paths.py checks on the CPU that every path is reached) and held against the oracle
in fp64 -- run on the MI355X with -m gpu.

Every scene goes through t2d_integrate on an (n, 1) pool with the variants fast, fast_iterated and fast_resummed, through
t2d_step on that pool with the single-ego kernel on and off, and through t2d_step on an (n / 64, 64) pool without geometry.
Alongside, the exact variant on the same pool is bit-equal to the oracle's fp32 rounding.

Bounds (against oracle.integrate(..., trig=1) in fp64):
  kinematics  x, y: 0.5 ulp32 + 2e-9;  heading, speed, vx, vy: 0.5 ulp32 + 1e-7  (those of test_resummed_kinematics...: the
              piecewise form equals the iterated sum in exact arithmetic, so no larger term is due); a lane that ends pinned
              on a speed bound stores the bound's bits.
  dynamics    the same two floors + 1e-4 x sens, sens = the oracle's one-step helpers.rollout_sensitivity (yardstick and factor
              of test_gpu_configs.py).  rotate_tiny's truncation gives a few 1e-10 m over a step at the scenes' displacements.
              Lanes with sens > 10 are left out and reported, at most 1 % per scene: on the CPU the oracle alone has none
              (largest sens of any scene: 4e-6, test_fast_paths.py asserts the cap), so a lane lost here is the kernel's doing.
"""
from collections import defaultdict
from types import SimpleNamespace

import numpy as np
import pytest

import fast_paths as FP
import helpers as H
from tactics2d_amd import layout as L

pytestmark = pytest.mark.gpu

ENTRIES = ["integrate:fast", "integrate:fast_iterated", "integrate:fast_resummed", "step_ego:fast", "step_lanes:fast", "step_64:fast"]
_CACHE = {}


def _prepared(oracle, model, interval, delta_t=None):
    """scene, oracle result (fp64), sensitivity: computed once per scene and shared by the entry points; never modified"""
    key = (model, interval, delta_t)
    if key not in _CACHE:
        sc = FP.kin_scene(interval, delta_t) if model == "kin" else FP.dyn_scene(interval)
        ref = H.oracle_physics(oracle, sc.rows, sc.tid, sc.state, sc.action, interval, model, trig=1)
        sens = None
        if model == "dyn":
            ns = SimpleNamespace(rows=sc.rows, x=sc.state[:, 0], y=sc.state[:, 1], heading=sc.state[:, 2], speed=sc.state[:, 3],
                                 type_id=sc.tid, active=np.ones(sc.n, np.uint8), interval_ms=interval)
            sens = H.rollout_sensitivity(oracle, ns, [(sc.action[:, 0], sc.action[:, 1])], np.arange(sc.n))
            sens.setflags(write=False)
        ref.setflags(write=False)
        _CACHE[key] = (sc, ref, sens)
    return _CACHE[key]


def _run(sc, entry, variant):
    """fp32 (n, 8): x, y, heading, speed, vx, vy, applied0, applied1 after one step of the scene through `entry`"""
    from tactics2d_amd.pool import ParticipantPool
    if entry == "integrate":
        return H.gpu_physics(sc.rows, sc.tid, sc.state, sc.action, sc.interval, variant, sc.model)
    n_env, A = (sc.n // 64, 64) if entry == "step_64" else (sc.n, 1)
    pool = ParticipantPool(n_env, A)
    try:
        pool.set_param_table(sc.rows)
        pool.set_integrator_variant(variant)
        pool.reset(sc.state[:, 0], sc.state[:, 1], sc.state[:, 2], sc.state[:, 3], sc.tid)
        pool.set_actions(sc.action[:, 0], sc.action[:, 1])
        if A == 1:
            pool.set_ego_kernel(entry == "step_ego")
            assert pool.step_form(1) == ("ego" if entry == "step_ego" else "step")
        pool.step(sc.interval)
        return np.stack([pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY, L.F_APPLIED0, L.F_APPLIED1)], 1)
    finally:
        pool.close()


def _assert_exact_is_the_oracle(sc, entry, ref):
    got = _run(sc, entry, "exact")
    want = np.float32(ref)
    for c in [0, 1, 2, 3] + ([4, 5] if sc.model == "kin" else []):
        bad = (got[:, c].view(np.uint32) != want[:, c].view(np.uint32)) & ~((got[:, c] == 0) & (want[:, c] == 0))
        assert not bad.any(), (entry, c, int(bad.sum()), np.nonzero(bad)[0][:5], got[bad, c][:3], want[bad, c][:3])


def _errors_over_bounds(sc, got, ref, sens):
    """|got - ref| / bound per lane and column (x, y, heading, speed[, vx, vy])"""
    cols = 6 if sc.model == "kin" else 4
    e = np.abs(got[:, :cols].astype(np.float64) - ref[:, :cols])
    e[:, 2] = H.ang_err(got[:, 2], ref[:, 2])
    ulp = np.float64(np.spacing(np.abs(np.float32(ref[:, :cols]))))
    bound = 0.5 * ulp + np.where(np.arange(cols) < 2, 2e-9, 1e-7)[None, :]
    if sens is not None:
        bound = bound + 1e-4 * sens[:, None]
    return e, e / bound, np.maximum(e[:, :2] - 0.5 * ulp[:, :2], 0.0).max(1)


def _report(tag, sc, paths, ratio, err, keep, excess):
    worst = defaultdict(lambda: (0.0, 0.0, 0.0))
    for w, (label, path) in enumerate(zip(sc.labels, paths)):
        sl = slice(64 * w, 64 * w + 64)
        k = keep[sl]
        if not k.any():
            continue
        r, e, x = float(ratio[sl][k].max()), float(err[sl][k][:, :2].max()), float(excess[sl][k].max())
        key = path if sc.want[w] is not None and not label.startswith("spoiler") else f"{label.split('/')[0]} ({path})"
        worst[key] = (max(worst[key][0], r), max(worst[key][1], e), max(worst[key][2], x))
    print(f"{tag}: per path class the worst error / bound, the largest |dx|, |dy|, and the largest part of it beyond half an fp32 ulp")
    for key in sorted(worst):
        print(f"    {key:34s} {worst[key][0]:.3f}   {worst[key][1]:.2e} m   {worst[key][2]:.2e} m")


def _paths(sc, entry, variant):
    # the resummation table: fast_resummed only (pools of this size do not fill the GPU; the single-ego kernel has no series)
    kin_n = sc.interval // int(sc.rows[0, L.P_DELTA_T_MS]) if (entry, variant) == ("integrate", "fast_resummed") and sc.model == "kin" else 0
    return FP.wave_paths(sc.model, sc.rows, sc.tid, sc.state, sc.action, sc.interval, group=64, kin_n=kin_n)


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("interval,delta_t", FP.KIN_TIMINGS)
def test_kinematic_paths_against_the_oracle(oracle, interval, delta_t, entry):
    sc, ref, _ = _prepared(oracle, "kin", interval, delta_t)
    where, variant = entry.split(":")
    _assert_exact_is_the_oracle(sc, where, ref)
    got = _run(sc, where, variant)
    err, ratio, excess = _errors_over_bounds(sc, got, ref, None)
    paths = _paths(sc, where, variant)
    _report(f"kinematics ({interval}, {delta_t}) {entry}", sc, paths, ratio, err, np.ones(sc.n, bool), excess)
    worst = np.unravel_index(np.argmax(ratio), ratio.shape)
    assert ratio.max() <= 1.0, (entry, "lane", int(worst[0]), "wave", int(worst[0]) // 64, sc.labels[worst[0] // 64], paths[worst[0] // 64],
                                "column", int(worst[1]), "error", err[worst], "error / bound", ratio[worst])
    # a lane that ends pinned on a bound stores the bound's bits
    k = FP.kin_lanes(sc.rows, sc.tid, sc.state, sc.action, interval)
    named = np.repeat([w is not None for w in sc.want], 64)
    ends_on = named & (k["crossing"] | k["pinned"])
    bound = np.where(k["pinned"], np.float64(sc.state[:, 3]), k["vB"])
    assert ends_on.sum() >= 64 * 2 * (interval // delta_t)
    assert np.array_equal(got[ends_on, 3].view(np.uint32), np.float32(bound[ends_on]).view(np.uint32)), entry
    assert np.array_equal(got[:, 6:8], np.float32(ref[:, 6:8]))


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("interval", FP.DYN_INTERVALS)
def test_dynamics_paths_against_the_oracle(oracle, interval, entry):
    sc, ref, sens = _prepared(oracle, "dyn", interval)
    where, variant = entry.split(":")
    _assert_exact_is_the_oracle(sc, where, ref)
    got = _run(sc, where, variant)
    err, ratio, excess = _errors_over_bounds(sc, got, ref, sens)
    keep = sens <= 10
    paths = _paths(sc, where, variant)
    print(f"dynamics {interval} {entry}: {int((~keep).sum())} of {sc.n} lanes beyond sens 10 left out; largest sens {sens.max():.3g}")
    _report(f"dynamics {interval} {entry}", sc, paths, ratio, err, keep, excess)
    assert (~keep).mean() <= 0.01
    r = np.where(keep[:, None], ratio, 0.0)
    worst = np.unravel_index(np.argmax(r), r.shape)
    assert r.max() <= 1.0, (entry, "lane", int(worst[0]), "wave", int(worst[0]) // 64, sc.labels[worst[0] // 64], paths[worst[0] // 64],
                            "column", int(worst[1]), "error", err[worst], "error / bound", r[worst], "sens", sens[worst[0]])
