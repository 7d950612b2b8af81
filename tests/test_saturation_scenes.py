"""Preconditions of the saturation scenes (tests/saturation_scenes.py), on the CPU: what tests/test_gpu_saturation.py feeds the step
kernel really has several times the queue capacity in candidates per wave, the oracle's flags are the intended witnesses, and enough
queue entries decide a flag alone that a fault losing one entry per round cannot hide."""
import numpy as np
import pytest

import helpers as H
import saturation_scenes as S

CAP = S.queue_cap()


def test_queue_capacity_is_read_from_the_source():
    assert CAP >= 3 * 96, CAP      # (the kernel's own static_assert: the ring sweep's staging floats live in the queue)


@pytest.mark.parametrize("case", S.CASES, ids=repr)
def test_preconditions(oracle, case):
    """per case, over its seeds: oracle flags == witnesses; the share of set flags per stage in [0.2, 0.8]; in every full wave the
    lower bound on the entries of the busiest call of compact_and_process (a polygon stage makes one call per 64-box chunk of
    the env's list, and in the split form per lane half) against the expected multiple of kQueueCap; sole witnesses >= 1000 and
    >= 0.5 % of the bound on all entries.  Lane scenes: no env has a safe rectangle (a certified pose would skip the lane sweep
    and its candidates with it)."""
    bits = dict(pairs=S.F_DYNAMIC, static=S.F_STATIC, lanes=S.F_OFF_LANE)
    bound_min = {s: None for s in ("pairs", "static", "lanes")}
    bound_max = dict.fromkeys(bound_min, 0)
    bound_sum = dict.fromkeys(bound_min, 0)
    sole = dict.fromkeys(case.stages, 0)
    split_min = 1 << 30
    set_n = dict.fromkeys(case.stages, 0); pop_n = dict.fromkeys(case.stages, 0)
    for seed in case.seeds:
        sc = case.scene(seed)
        assert not sc["heading"].any()
        if "shifted" not in case.name:
            assert np.abs(sc["x"]).max() <= 16.0 and np.abs(sc["y"]).max() <= 16.0
        f, _ = H.oracle_collide(oracle, sc)
        want = case.flags_of(sc)
        bad = np.flatnonzero((f & sc["bit"]) != want)
        assert bad.size == 0, f"{case} seed {seed}: the oracle's flags differ from the witnesses at {bad[:8].tolist()}: {f[bad[:8]].tolist()} / {want[bad[:8]].tolist()}"
        fits = S.geometry_fits(sc)
        assert fits["fits"], (case, fits)
        if sc["lanes"] is not None:
            rects = H.lane_safe_rects(sc["lanes"])
            assert not np.isfinite(rects).all(2).any(), "a lane scene with a safe rectangle: certified poses skip the lane sweep"
        wb = S.wave_lower_bounds(sc, fits["envs_per_workgroup"])
        for s in bound_min:
            v = wb[s][wb["full"]]
            bound_min[s] = int(v.min()) if bound_min[s] is None else min(bound_min[s], int(v.min()))
            bound_max[s] = max(bound_max[s], int(v.max()))
            bound_sum[s] += int(wb[s + "_all"].sum())
        if case.split_expect is not None:
            ws = S.wave_lower_bounds(sc, fits["envs_per_workgroup"], split=True)
            split_min = min(split_min, int(ws["lanes"][ws["full"]].min()))
        for s, n in S.sole_witnesses(sc).items():
            sole[s] += n
        for s in case.stages:
            # the stage's own population: in the combined scene the needles for pairs (boxes touch boxes by chance), the boxes for the
            # polygon stages (every needle lies across the lanes)
            pop = sc["active"] != 0
            if sc["kind"] == "combined":
                pop = sc["type_id"] == (S.T_NEEDLE if s == "pairs" else S.T_BOX)
            set_n[s] += int(((f & bits[s]) != 0)[pop].sum()); pop_n[s] += int(pop.sum())
    share = {s: set_n[s] / pop_n[s] for s in case.stages}
    msg = (f"{case}: capacity {CAP}; lower bound on the busiest call per full wave min {bound_min} max {bound_max}"
           + (f", lane halves of the split form min {split_min}" if case.split_expect is not None else "")
           + f", entries of all calls, waves and seeds {bound_sum}; "
           f"flag share {({s: round(v, 3) for s, v in share.items()})}; sole witnesses {sole} over {len(case.seeds)} seeds")
    print(msg)
    for s in case.stages:
        assert 0.2 <= share[s] <= 0.8, msg
    for s, m in case.expect.items():
        if m == 0:
            assert bound_max[s] < CAP, msg
        else:
            assert bound_min[s] >= m * CAP, msg
    for s, m in case.below.items():
        assert bound_max[s] < m * CAP, msg
    if case.split_expect is not None:
        assert split_min >= case.split_expect * CAP, msg
    # (the hash-grid cases have no pair queue and no multiple to reach -- their chains are what is long, see
    # test_grid_scenes_... -- but a lost pair must show there as anywhere)
    for s in case.stages:
        assert sole[s] >= 1000 and sole[s] >= 0.005 * bound_sum[s], msg


@pytest.mark.parametrize("name", ["needles_64x16", "needles_half_inactive_64x64"])
def test_two_needle_scenes_reach_exactly_the_second_round(name):
    """4 x 120 pairs are all a wave of 16-agent envs holds, 496 all that 32 active needles make: past one capacity, short of two"""
    case = next(c for c in S.CASES if c.name == name)
    assert case.expect == dict(pairs=1) and case.below == dict(pairs=2)
    for seed in case.seeds:
        wb = S.wave_lower_bounds(case.scene(seed))
        assert CAP < wb["pairs"].min() and wb["pairs"].max() < 2 * CAP, wb["pairs"]


@pytest.mark.parametrize("stage,n_env,A,K", S.SLAT_DOES_NOT_FIT)
def test_the_boundary_between_the_tiers_is_known(stage, n_env, A, K):
    """one (shape, K) per stage that does NOT fit the LDS record -- it would run on the HBM grid tier, other kernels
    (tests/test_gpu_mapgrid.py) -- next to the largest K of that shape that does"""
    assert not S.geometry_fits(S.slat_scene(n_env, A, K, stage, 0))["fits"]
    below = max(S.SLAT_FITS[stage][A])
    assert below < K and S.geometry_fits(S.slat_scene(n_env, A, below, stage, 0))["fits"]


@pytest.mark.parametrize("name", ["needles_grid_16x100", "needles_grid_8x200", "needles_grid_shifted_16x100", "needles_grid_shifted_8x200"])
def test_grid_scenes_cross_cell_borders_and_fill_buckets(name):
    """hash-grid needle stacks: contacts cross cell borders in x, in y and diagonally where the stack straddles x = 0 (the unshifted
    scenes; moved by (-1000, 2000) the stack lies inside one cell column, x = -1000 being no cell border, and its contacts cross
    rows only or stay in a cell: the long-chain variant), the stack runs through several cell rows, and a cell holds tens of
    needles -- the chains the walk goes down"""
    case = next(c for c in S.CASES if c.name == name)
    cell = S.cell_edge()
    kinds = dict(x=0, y=0, diagonal=0, same=0)
    longest, rows = 0, 0
    for seed in case.seeds:
        sc = case.scene(seed)
        A = sc["A"]
        cx = np.floor(np.float64(sc["x"]) / cell).astype(int); cy = np.floor(np.float64(sc["y"]) / cell).astype(int)
        i = np.flatnonzero(sc["partner"] >= 0)
        j = (i // A) * A + sc["partner"][i]
        dx, dy = cx[i] != cx[j], cy[i] != cy[j]
        kinds["x"] += int((dx & ~dy).sum()) // 2; kinds["y"] += int((~dx & dy).sum()) // 2
        kinds["diagonal"] += int((dx & dy).sum()) // 2; kinds["same"] += int((~dx & ~dy).sum()) // 2
        for e in range(sc["n_env"]):
            cells, counts = np.unique(np.stack([cx, cy], 1)[e * A:(e + 1) * A], axis=0, return_counts=True)
            longest = max(longest, int(counts.max())); rows = max(rows, len(np.unique(cells[:, 1])))
    print(name, kinds, "longest bucket", longest, "cell rows", rows)
    assert longest >= 20 and kinds["y"] >= 1
    if "shifted" not in name:
        assert kinds["x"] >= 100 and kinds["diagonal"] >= 1
    else:
        assert kinds["same"] >= 100 and kinds["x"] == 0 and longest >= 40
    if name.endswith("8x200"):
        assert rows >= 4
