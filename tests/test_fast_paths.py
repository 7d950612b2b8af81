"""The path model of the fast integrators (tests/fast_paths.py) on the CPU: what the existing tests' inputs reach when taken
in the order drawn, what the wave-by-wave scenes and the sorted fixtures reach, and the model's dynamics replay against the
oracle.  The GPU side is tests/test_gpu_fast_paths.py."""
from collections import Counter
from types import SimpleNamespace

import numpy as np
import pytest

import fast_paths as FP
import helpers as H


def _fixture_groups(d):
    for iv in np.unique(d["timing"][:, 0]):
        yield int(iv), np.nonzero(d["timing"][:, 0] == iv)[0]


def test_in_drawn_order_the_older_tests_reach_the_plain_loop_and_the_general_loop_only():
    """The record of what made this module necessary.  test_fast_kinematics_speed_clipping_paths mixes its cases lane by lane:
    a fifth of them start outside their range, so every wave takes the plain loop -- the piecewise form is never run.
    test_dynamics_within_1e5...[fast] on dyn_random.npz as drawn: almost every LANE is always_fast and tiny, almost no WAVE."""
    for interval, delta_t in [(100, 5), (50, 3), (9, 5), (100, 7)]:
        rows, tid, st, act = FP.clipping_cases(interval, delta_t)
        k = FP.kin_lanes(rows, tid, st, act, interval)
        drawn = Counter(FP.wave_paths("kin", rows, tid, st, act, interval))
        o = FP.by_path_order("kin", rows, tid, st, act, interval)
        by_path = Counter(FP.wave_paths("kin", rows, tid[o], st[o], act[o], interval))
        print(f"clipping test ({interval}, {delta_t}): lanes linear {100 * k['lane_linear'].mean():.0f} %, crossing {100 * k['crossing'].mean():.0f} %;"
              f" waves as drawn {dict(drawn)}, by path {dict(by_path)}")
        assert drawn == {"plain": 94}
        assert by_path["piecewise"] >= 5 and by_path["linear/tiny"] + by_path["linear/small"] >= 55 and by_path["plain"] >= 15
    d = H.load_npz("dyn_random.npz")
    drawn, lanes_fast, lanes_tiny, sub_tiny, sub_all = Counter(), 0, 0, 0, 0
    for iv, m in _fixture_groups(d):
        r = FP.dyn_replay(d["rows"], d["type_id"][m], d["state"][m], d["action"][m], iv)
        drawn.update(FP.dyn_wave_path(r, slice(i, min(i + 64, len(m)))) for i in range(0, len(m), 64))
        lanes_fast += int(r["always_fast"].sum())
        with np.errstate(invalid="ignore"):
            lanes_tiny += int((np.nan_to_num(np.nanmax(r["eps"], 1), nan=np.inf) <= FP.K_EPS_TINY).sum())
        for i in range(0, len(m), 64):            # wave-sub-steps that take rotate_tiny: the whole wave below kEpsTiny
            e = r["eps"][i:i + 64]
            live = ~np.isnan(e).all(0)
            with np.errstate(invalid="ignore"):
                sub_tiny += int((np.nan_to_num(np.nanmax(e[:, live], 0), nan=np.inf) <= FP.K_EPS_TINY).sum())
            sub_all += int(live.sum())
    n_fast = sum(v for p, v in drawn.items() if p.startswith("always_fast"))
    print(f"dyn_random.npz as drawn: {lanes_fast} of 6000 lanes always_fast, {lanes_tiny} tiny in every sub-step; waves {dict(drawn)}; "
          f"{sub_tiny} of {sub_all} wave-sub-steps take rotate_tiny")
    assert lanes_fast >= 5400 and lanes_tiny >= 4400
    assert n_fast <= 2 and sub_tiny <= 5 and sum(drawn.values()) == 95


def test_sorted_by_path_the_dynamics_fixture_runs_what_the_benchmark_runs():
    d = H.load_npz("dyn_random.npz")
    got = Counter()
    strict_tiny = total_tiny = 0
    for iv, m in _fixture_groups(d):
        o = m[FP.by_path_order("dyn", d["rows"], d["type_id"][m], d["state"][m], d["action"][m], iv)]
        p = FP.wave_paths("dyn", d["rows"], d["type_id"][o], d["state"][o], d["action"][o], iv)
        got.update(p)
        for w, name in enumerate(p):
            if name == "always_fast/tiny":
                total_tiny += 1
                strict_tiny += bool((d["sens"][o[64 * w:64 * w + 64]] < H.SENS_STRICT).all())
    print("dyn_random.npz by path:", dict(got), f"-- {strict_tiny} of the {total_tiny} always_fast/tiny waves hold strict cases only")
    assert got["always_fast/tiny"] >= 60
    assert got["always_fast/small"] + got["always_fast/reseed"] >= 5
    assert got["general/tiny"] + got["general/small"] + got["general/reseed"] >= 5
    assert strict_tiny >= 60


@pytest.mark.parametrize("interval,delta_t", FP.KIN_TIMINGS)
def test_kinematic_scene_reaches_every_path_on_purpose(interval, delta_t):
    sc = FP.kin_scene(interval, delta_t)
    n_steps = interval // delta_t
    assert sc.n == 64 * len(sc.labels) and sc.n % 64 == 0 and len(sc.rows) <= 32
    k = FP.kin_lanes(sc.rows, sc.tid, sc.state, sc.action, interval)
    paths = FP.wave_paths("kin", sc.rows, sc.tid, sc.state, sc.action, interval)
    for w, (label, want, got) in enumerate(zip(sc.labels, sc.want, paths)):
        assert want is None or want == got, (w, label, want, got)
    count = Counter(paths)
    print(f"kin scene ({interval}, {delta_t}): {len(paths)} waves {dict(count)}")
    for p in ("linear/tiny", "linear/small", "piecewise", "plain"):
        assert count[p] >= 2, (p, count)
    # the series: on for fast_resummed (and for fast on pools that fill the GPU), off for the spoiler wave
    res = FP.wave_paths("kin", sc.rows, sc.tid, sc.state, sc.action, interval, kin_n=n_steps)
    assert Counter(res)["resummed"] >= 2
    assert res[sc.labels.index("spoiler/resum+n")].startswith("linear/")
    # the single-ego kernel's waves (four consecutive envs): the same classes
    ego = Counter(FP.wave_paths("kin", sc.rows, sc.tid, sc.state, sc.action, interval, group=4))
    for p in ("linear/tiny", "linear/small", "piecewise", "plain"):
        assert ego[p] >= 2, (p, ego)
    # margins: 20 % clear of the thresholds that define the class
    seen = {True: set(), False: set()}
    for w, label in enumerate(sc.labels):
        sl = slice(64 * w, 64 * w + 64)
        if label.startswith("cross/") and "kstar=" in label:
            ks = int(label.split("=")[1])
            up = "/hi/" in label
            assert k["crossing"][sl].all() and (k["kstar"][sl] == ks).all(), label
            frac = ks - k["t_cross"][sl]
            assert (frac >= 0.19).all() and (frac <= 0.81).all(), (label, frac.min(), frac.max())
            seen[up].add(ks)
        if label.endswith("/mixed"):
            ks = k["kstar"][sl]
            assert (ks == FP.INT_MAX).sum() >= 10 and len(np.unique(ks)) >= min(4, n_steps + 1), label
        if label == "cross/near-integer":
            from tactics2d_amd import layout as L
            tid = sc.tid[sl].astype(int)   # (rows T_EXACT .. +3: the upper bound was placed, +4 .. +7: the lower one)
            bound = np.where(tid < FP.T_EXACT + 4, sc.rows[tid, L.P_SPEED_HI], sc.rows[tid, L.P_SPEED_LO])
            t = (bound - np.float64(sc.state[sl, 3])) / (np.float64(sc.action[sl, 0]) * (delta_t / 1000.0))
            assert (np.round(t) >= 1).all() and (np.round(t) <= n_steps).all()
            assert (np.abs(t - np.round(t)) <= 1e-12).all(), np.abs(t - np.round(t)).max()
        if label == "linear/tiny":
            assert (k["amax"][sl] <= FP.EPS_TINY_IN).all()
        if label == "linear/small":
            assert (k["amax"][sl] >= 0.012).sum() >= 8 and (k["amax"][sl] <= FP.EPS_SMALL_HI).all()
        if label == "pinned":
            assert k["pinned"][sl].all()
    assert seen[True] == seen[False] == set(range(1, n_steps + 1))
    pinned = np.concatenate([np.arange(64 * w, 64 * w + 64) for w, l in enumerate(sc.labels) if l == "pinned"])
    a = np.float64(sc.action[pinned, 0])
    assert ((a == 0) & ~np.signbit(a)).any() and ((a == 0) & np.signbit(a)).any()            # ah == +0 and -0
    assert ((sc.state[pinned, 3] == 0) & (a < 0)).any()                                        # v == vlo == 0, ah < 0
    # coordinates the fp32 store resolves
    assert np.abs(sc.state[:, :2]).max() <= 0.01 and sc.state[:, 2].min() >= 0 and sc.state[:, 2].max() < 0.2
    assert np.abs(sc.state[:, 3]).max() * interval / 1000 <= 3.1


def _sens(oracle, sc):
    ns = SimpleNamespace(rows=sc.rows, x=sc.state[:, 0], y=sc.state[:, 1], heading=sc.state[:, 2], speed=sc.state[:, 3],
                         type_id=sc.tid, active=np.ones(sc.n, np.uint8), interval_ms=sc.interval)
    return H.rollout_sensitivity(oracle, ns, [(sc.action[:, 0], sc.action[:, 1])], np.arange(sc.n))


@pytest.mark.parametrize("interval", FP.DYN_INTERVALS)
def test_dynamics_scene_reaches_every_path_on_purpose_and_the_replay_is_the_oracle(oracle, interval):
    sc = FP.dyn_scene(interval)
    assert sc.n == 64 * len(sc.labels) and len(sc.rows) <= 32
    d = FP.dyn_replay(sc.rows, sc.tid, sc.state, sc.action, interval)
    paths = FP.wave_paths("dyn", sc.rows, sc.tid, sc.state, sc.action, interval)
    for w, (label, want, got) in enumerate(zip(sc.labels, sc.want, paths)):
        assert want is None or want == got, (w, label, want, got)
    named = Counter(p for p, want in zip(paths, sc.want) if want is not None)
    print(f"dyn scene {interval}: {len(paths)} waves {dict(Counter(paths))}")
    for p in ("always_fast/tiny", "always_fast/small", "always_fast/reseed", "general/tiny", "general/small"):
        assert named[p] >= 2, (p, named)
    # trip counts differ inside every wave (delta_t 5 and 3), and odd counts occur where the interval has them
    for w in range(len(paths)):
        assert len(np.unique(d["n"][64 * w:64 * w + 64])) == 2, sc.labels[w]
    if interval in (9, 35):
        assert (d["n"] % 2 == 1).all()
    # margins of the non-edge waves
    with np.errstate(invalid="ignore"):
        mx = np.nanmax(d["eps"], 1)
    for w, (label, want) in enumerate(zip(sc.labels, sc.want)):
        if want is None or label.startswith("spoiler"):
            continue
        sl = slice(64 * w, 64 * w + 64)
        band = (mx[sl] <= FP.EPS_TINY_IN) | ((mx[sl] >= FP.EPS_SMALL_LO) & (mx[sl] <= FP.EPS_SMALL_HI)) | (mx[sl] >= FP.EPS_RESEED)
        assert band.all(), (label, mx[sl][~band])
        fast = d["always_fast"][sl]
        v0 = np.abs(np.float64(sc.state[sl, 3]))
        assert ((v0[fast] >= FP.V_HIGH) & (np.abs(d["v_fin"][sl][fast]) >= FP.V_HIGH)).all(), label
        with np.errstate(invalid="ignore"):
            assert (np.nanmax(np.abs(d["v_sub"][sl][~fast]), 1) <= FP.V_LOW).all(), label
    # the model's replay IS the oracle's recurrence: final speed and heading to 1e-12
    o = H.oracle_physics(oracle, sc.rows, sc.tid, sc.state, sc.action, interval, "dyn", trig=1)
    assert np.abs(d["v"] - o[:, 3]).max() <= 1e-12
    assert H.ang_err(np.mod(d["phi"], 2 * np.pi), o[:, 2]).max() <= 1e-12
    # conditioning: the oracle alone keeps every lane far below the cut (sens > 10) of the GPU test
    sens = _sens(oracle, sc)
    print(f"   one-step sensitivity of the oracle: max {sens.max():.3g}, {int((sens > 10).sum())} lanes beyond 10")
    assert np.isfinite(sens).all() and (sens > 10).mean() <= 0.01
    assert np.abs(sc.state[:, :2]).max() <= 0.01 and sc.state[:, 2].max() < 0.2
