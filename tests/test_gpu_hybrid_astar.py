"""t2d_hybrid_astar on the device: EVERY case of the fixture made by running the reference's HybridAStar.plan
(tests/golden/hybrid_astar.npz) as ragged batches through the C interface into sentinel-filled buffers with guard regions, path,
path length, status, pops and nodes BIT-EQUAL to the specification (tests/hybrid_astar_ref.py); the same cases in reversed order
with identical rows; one query at both ends of a 130-row batch and alone; INVALID, TRUNCATED, MAX_ITER and OVERFLOW rows (by
max_nodes, by the open-set cap, by the cost grid's cap) beside good ones; device tensors in and out on a side stream;
HybridAStar.plan against the recorded reference lists, and its refusal to answer [] for a search it did not finish; and a fresh
random batch against the specification."""
import math

import numpy as np
import pytest

import hybrid_astar_ref as R
from test_hybrid_astar import MAX_NODES, MAX_PATH, case_deltas, fixture, fixture_case, n_cases, spec_case

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -12345.0, 7.0e30   # outputs start as SENTINEL; PAD fills the weights no kernel may read
GUARD = 64
FIVE = (-0.6, -0.3, 0.0, 0.3, 0.6)


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _raw(torch, rows, deltas, step_size, max_iter, max_nodes=MAX_NODES, max_path=MAX_PATH, cell_size=1.0, origin=(0.0, 0.0), hw=None,
         stride=None):
    """t2d_hybrid_astar through the C interface; rows: (grid, start, target, boundary) each.  Outputs are sentinel-filled with a guard
    region behind them (checked here), the workspace is filled with a pattern ->
    (path [n, max_path, 3], path_len, status, iterations, nodes [n])"""
    from tactics2d_amd import _ffi
    lib = _ffi.lib()
    n = len(rows)
    stride = max(r[0].size for r in rows) if stride is None else stride
    w = np.full((n, stride), PAD)
    for k, r in enumerate(rows):
        w[k, :r[0].size] = r[0].reshape(-1)
    hw = np.int32([r[0].shape for r in rows]) if hw is None else np.int32(hw)
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    w_d, hw_d = t(w, np.float64), t(hw, np.int32)
    s_d, t_d, b_d = (t(np.float64([r[i] for r in rows]), np.float64) for i in (1, 2, 3))
    d_d = t(np.float64(deltas), np.float64)
    need = lib.t2d_hybrid_astar_workspace_bytes(n, max_nodes)
    ws = torch.full((need + GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    path = torch.full((n * max_path * 3 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    small = [torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    rc = lib.t2d_hybrid_astar(0, n, w_d.data_ptr(), hw_d.data_ptr(), stride, s_d.data_ptr(), t_d.data_ptr(), b_d.data_ptr(), d_d.data_ptr(),
                              len(deltas), step_size, cell_size, origin[0], origin[1], max_iter, max_nodes, max_path, ws.data_ptr(), need,
                              path.data_ptr(), *(x.data_ptr() for x in small), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.t2d_last_error(None).decode()
    path = path.cpu().numpy()
    small = [x.cpu().numpy() for x in small]
    assert (path[n * max_path * 3:] == SENTINEL).all() and all((x[n:] == -7).all() for x in small)
    assert (ws[need:] == 0x5a).all().item()
    return (path[:n * max_path * 3].reshape(n, max_path, 3),) + tuple(x[:n] for x in small)


def _same(got, want, what):
    """one row of _raw against a specification dict"""
    path, path_len, status, iterations, nodes = got
    assert (status, path_len, iterations, nodes) == (want["status"], want["path_len"], want["iterations"], want["nodes"]), \
        (what, status, path_len, iterations, nodes, want["status"], want["path_len"], want["iterations"], want["nodes"])
    m = min(path_len, len(path))
    assert path[:m].tobytes() == want["path"][:m].tobytes(), what
    assert np.isnan(path[m:]).all() and np.isnan(want["path"][m:]).all(), what


def _groups():
    """fixture cases that can share a launch: the same step_size, steering angles, wheelbase and max_iter"""
    g = fixture()
    out = {}
    for k in range(n_cases()):
        c = fixture_case(k)
        out.setdefault((c["step_size"], tuple(c["steering"]), c["wheelbase"], c["max_iter"]), []).append(k)
    return out


def _launch(torch, ks):
    cases = [fixture_case(k) for k in ks]
    c = cases[0]
    return _raw(torch, [(x["grid"], x["start"], x["target"], x["boundary"]) for x in cases], case_deltas(c), c["step_size"], c["max_iter"])


@pytest.fixture(scope="module")
def forward(torch):
    """every fixture case, one launch per group -> {case: row of _raw}"""
    rows = {}
    for ks in _groups().values():
        out = _launch(torch, ks)
        for i, k in enumerate(ks):
            rows[k] = tuple(o[i] for o in out)
    return rows


def test_the_whole_fixture_is_bit_equal_to_the_specification(forward):
    g = fixture()
    found = 0
    for k in range(n_cases()):
        _same(forward[k], spec_case(k), g["name"][k])
        c = fixture_case(k)
        path, path_len, status = forward[k][:3]
        assert status == c["status"] and path_len == len(c["path"]), g["name"][k]
        if path_len:
            assert np.abs(path[:path_len] - c["path"]).max() <= 1e-9, g["name"][k]
            found += 1
    assert found >= 150


def test_reversed_order_changes_no_row(torch, forward):
    for ks in _groups().values():
        ks = ks[::-1]
        out = _launch(torch, ks)
        for i, k in enumerate(ks):
            for a, b in zip((o[i] for o in out), forward[k]):
                assert np.asarray(a).tobytes() == np.asarray(b).tobytes(), fixture()["name"][k]


def test_a_query_gives_the_same_row_at_both_ends_of_a_batch_and_alone(torch):
    g = fixture()
    k = int(np.flatnonzero((g["path_len"] >= 10) & (g["n_steer"] == 3) & (g["step_size"] == 1.0) & (g["max_iter"] == 20000))[0])
    c = fixture_case(k)
    others = [j for j in _groups()[(c["step_size"], tuple(c["steering"]), c["wheelbase"], c["max_iter"])] if j != k]
    others = (others * (128 // len(others) + 1))[:128]   # (the group has about a hundred cases: some come twice)
    row = lambda j: (fixture_case(j)["grid"], fixture_case(j)["start"], fixture_case(j)["target"], fixture_case(j)["boundary"])
    batch = [row(k)] + [row(j) for j in others] + [row(k)]
    out = _raw(torch, batch, case_deltas(c), c["step_size"], c["max_iter"])
    alone = _raw(torch, [row(k)], case_deltas(c), c["step_size"], c["max_iter"])
    for i in (0, 129):
        _same(tuple(o[i] for o in out), spec_case(k), i)
    _same(tuple(o[0] for o in alone), spec_case(k), "alone")
    for i, j in enumerate(others):
        _same(tuple(o[i + 1] for o in out), spec_case(j), g["name"][j])


def test_invalid_truncated_max_iter_and_overflow_rows_sit_beside_good_ones(torch):
    g = fixture()
    std = (-0.5, 0.0, 0.5)
    pick = lambda cond: [int(k) for k in np.flatnonzero(cond & (g["n_steer"] == 3) & (g["step_size"] == 1.0) & (g["max_iter"] == 20000)
                                                        & (g["generated"] == 1))]
    short = pick((g["path_len"] >= 3) & (g["path_len"] <= 4) & (g["nodes"] <= 10))[:3]
    long_ = pick((g["path_len"] >= 9) & (g["nodes"] > 15))[:3]
    none = pick((g["path_len"] == 0) & (g["nodes"] >= 2) & (g["nodes"] <= 10))[:1] + pick((g["path_len"] == 0) & (g["nodes"] > 400))[:1]
    assert len(short) == 3 and len(long_) == 3 and len(none) == 2
    deltas = R.steer_deltas(std, 2.5, 1.0)
    row = lambda j: [fixture_case(j)["grid"], fixture_case(j)["start"], fixture_case(j)["target"], fixture_case(j)["boundary"]]
    nan, inf = float("nan"), float("inf")
    rows = [row(short[0]), row(long_[0]), row(none[0]), row(short[1]), row(long_[1]), row(short[2]), row(long_[2]), row(none[1])]
    bad = []
    for change in (lambda r: r.__setitem__(1, [nan, 1.0, 0.0]), lambda r: r.__setitem__(2, [1.0, inf, 0.0]),
                   lambda r: r.__setitem__(3, [r[3][1], r[3][0], r[3][2], r[3][3]]), lambda r: r.__setitem__(3, [0.0, 5.0, 2.0, 2.0]),
                   lambda r: r.__setitem__(1, [r[3][0] - 2.0, r[3][2], 0.0]), lambda r: r.__setitem__(1, [r[3][0], r[3][3] + 1.5, 0.0]),
                   lambda r: r.__setitem__(1, [1.0, 1.0, 3e9]), lambda r: r.__setitem__(3, [0.0, 4e150, 0.0, 5.0])):
        r = row(long_[0])
        change(r)
        bad.append(r)
    rows = rows[:2] + bad[:4] + rows[2:5] + bad[4:] + rows[5:]
    for what, kw in (("as they are", {}), ("max_path 5", dict(max_path=5)), ("max_iter 9", dict(max_iter=9)),
                     ("max_nodes 20", dict(max_nodes=20))):
        params = {"max_iter": 20000, "max_nodes": MAX_NODES, "max_path": MAX_PATH, **kw}
        out = _raw(torch, rows, deltas, 1.0, **params)
        seen = set()
        for i, r in enumerate(rows):
            want = R.solve(r[0], r[1], r[2], r[3], deltas, 1.0, **params)
            _same(tuple(o[i] for o in out), want, (what, i))
            seen.add(want["status"])
        assert R.INVALID in seen and R.FOUND in seen and R.NO_PATH in seen, (what, seen)
        assert {"max_path 5": R.TRUNCATED, "max_iter 9": R.MAX_ITER, "max_nodes 20": R.OVERFLOW}.get(what, R.FOUND) in seen, (what, seen)
    # an hw that does not fit its row: INVALID, the neighbours as before
    good = _raw(torch, rows, deltas, 1.0, 20000)
    hw = [r[0].shape for r in rows]
    stride = max(r[0].size for r in rows)
    hw[0], hw[6], hw[len(rows) - 1] = (0, 5), (-3, 4), (stride, 2)
    out = _raw(torch, rows, deltas, 1.0, 20000, hw=hw)
    for i in range(len(rows)):
        if i in (0, 6, len(rows) - 1):
            assert (out[1][i], out[2][i], out[3][i], out[4][i]) == (0, R.INVALID, 0, 0) and np.isnan(out[0][i]).all()
        else:
            assert all(np.asarray(a[i]).tobytes() == np.asarray(b[i]).tobytes() for a, b in zip(out, good)), i


def _wide_open(side=60):
    """a free grid and a target heading that is never met: the open set grows past T2D_HYBRID_MAX_OPEN"""
    return np.ones((side, side)), [5.0, side / 2, 0.3], [50.0, side / 2, 2 * math.pi], [0.0, float(side), 0.0, float(side)]


def test_overflow_by_the_open_set_cap_and_by_the_cost_grid_cap_beside_good_rows(torch):
    g = fixture()
    ks = [int(k) for k in np.flatnonzero((g["n_steer"] == 5) & (g["step_size"] == 1.0) & (g["max_iter"] == 20000) & (g["generated"] == 1)
                                         & (g["path_len"] >= 3) & (g["nodes"] < 3000))[:3]]
    deltas = R.steer_deltas(FIVE, 2.5, 1.0)
    row = lambda j: (fixture_case(j)["grid"], fixture_case(j)["start"], fixture_case(j)["target"], fixture_case(j)["boundary"])
    big = (np.ones((4, 4)), [1.0, 1.0, 0.0], [3.0, 3.0, 0.0], [0.0, 100.0, 0.0, 100.0])   # 201 x 201 x-y cells
    rows = [row(ks[0]), _wide_open(), row(ks[1]), big, row(ks[2])]
    out = _raw(torch, rows, deltas, 1.0, 20000)
    wants = [R.solve(r[0], r[1], r[2], r[3], deltas, 1.0, max_iter=20000, max_nodes=MAX_NODES, max_path=MAX_PATH) for r in rows]
    assert [w["status"] for w in wants] == [R.FOUND, R.OVERFLOW, R.FOUND, R.OVERFLOW, R.FOUND]
    assert wants[1]["open_peak"] == R.MAX_OPEN and wants[1]["nodes"] < MAX_NODES and wants[3]["iterations"] == 0
    for i, want in enumerate(wants):
        _same(tuple(o[i] for o in out), want, i)


def test_tensors_in_and_out_on_a_side_stream(torch):
    from tactics2d_amd import search
    g = fixture()
    ks = [int(k) for k in np.flatnonzero((g["hw"][:, 0] == 16) & (g["n_steer"] == 3) & (g["step_size"] == 0.5) & (g["max_iter"] == 20000))]
    cases = [fixture_case(k) for k in ks]
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")
    weights, starts = dev(np.stack([c["grid"] for c in cases])), dev([c["start"] for c in cases])
    targets, bounds = dev([c["target"] for c in cases]), dev([c["boundary"] for c in cases])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    out = search.HybridAStar.plan_batch(starts, targets, bounds, weights, step_size=0.5, max_iter=20000, max_path=MAX_PATH,
                                        max_nodes=MAX_NODES, stream=side)
    side.synchronize()
    assert out._inputs[0].data_ptr() == weights.data_ptr() and out._inputs[2].data_ptr() == starts.data_ptr()
    assert out._inputs[3].data_ptr() == targets.data_ptr() and out._inputs[4].data_ptr() == bounds.data_ptr()
    for x, dt in ((out.path, torch.float64), (out.path_len, torch.int32), (out.status, torch.int32), (out.iterations, torch.int32),
                  (out.nodes, torch.int32)):
        assert x.is_cuda and x.dtype == dt
    assert out.path.shape == (len(ks), MAX_PATH, 3)
    got = [x.cpu().numpy() for x in (out.path, out.path_len, out.status, out.iterations, out.nodes)]
    for i, k in enumerate(ks):
        _same(tuple(x[i] for x in got), spec_case(k), g["name"][k])
    # numpy in, one boundary for all rows, the default stream
    again = search.hybrid_plan_batch(np.float64([c["start"] for c in cases]), np.float64([c["target"] for c in cases]), cases[0]["boundary"],
                                     np.stack([c["grid"] for c in cases]), step_size=0.5, max_iter=20000, max_path=MAX_PATH,
                                     max_nodes=MAX_NODES)
    assert again.path.cpu().numpy().tobytes() == got[0].tobytes() and (again.status.cpu().numpy() == got[2]).all()


def test_plan_returns_the_reference_lists(torch):
    from tactics2d_amd import search
    g = fixture()
    picks = [int(np.argmax(g["path_len"]))] + [int(k) for k in np.flatnonzero((g["path_len"] == 0) & (g["nodes"] < 500))[:2]] + \
            [int(k) for k in np.flatnonzero((g["path_len"] >= 5) & (g["n_steer"] == 5))[:2]] + \
            [int(k) for k in np.flatnonzero(g["generated"] == 0) if g["nodes"][k] < 3000]
    for k in picks:
        c = fixture_case(k)
        got = search.HybridAStar.plan(list(c["start"]), list(c["target"]), list(c["boundary"]), c["grid"],
                                      search.grid_collide if k % 2 else None, c["step_size"], c["max_iter"], c["steering"], 1.0, c["wheelbase"])
        assert isinstance(got, list) and len(got) == len(c["path"]), g["name"][k]
        if got:
            assert all(isinstance(s, list) and len(s) == 3 for s in got)
            assert np.abs(np.float64(got) - c["path"]).max() <= 1e-9, g["name"][k]


def test_plan_raises_for_a_search_it_did_not_finish_and_for_an_invalid_row(torch):
    from tactics2d_amd import search
    grid, start, target, boundary = _wide_open()
    with pytest.raises(RuntimeError) as ei:
        search.HybridAStar.plan(start, target, boundary, grid, None, 1.0, 50000, list(FIVE))
    assert "not finished" in str(ei.value) and str(R.MAX_OPEN) in str(ei.value)
    with pytest.raises(ValueError):
        search.HybridAStar.plan([-5.0, 1.0, 0.0], [3.0, 3.0, 0.0], [0.0, 5.0, 0.0, 5.0], np.ones((5, 5)))
    # a path longer than plan's first buffer comes back whole
    long_path = search.HybridAStar.plan([1.0, 2.0, 0.0], [299.0, 2.0, 0.0], [0.0, 300.0, 0.0, 4.0], np.ones((4, 300)), None, 1.0, 50000, [0.0])
    assert len(long_path) == 299 and long_path[0] == [1.0, 2.0, 0.0] and long_path[-1] == [299.0, 2.0, 0.0]


def test_a_fresh_random_batch_equals_the_specification(torch):
    """not in the fixture: other grids, a cell size and an origin that are not 1 and 0, four steering angles"""
    rng = np.random.RandomState(20261020)
    steering, step, cs, origin = (-0.45, -0.1, 0.2, 0.5), 0.75, 0.8, (-1.5, 2.25)
    deltas = R.steer_deltas(steering, 2.2, step)
    rows = []
    for _ in range(24):
        h, w = rng.randint(4, 15), rng.randint(4, 15)
        grid = rng.randint(1, 6, size=(h, w)).astype(float)
        grid[rng.rand(h, w) < rng.choice([0.0, 0.1, 0.25])] = np.inf
        if rng.rand() < 0.3:
            grid[rng.randint(h), rng.randint(w)] = np.nan
        free = np.argwhere(np.isfinite(grid))
        (r0, c0), (r1, c1) = free[rng.randint(len(free))], free[rng.randint(len(free))]
        sx, sy, tx, ty = origin[0] + c0 * cs, origin[1] + r0 * cs, origin[0] + c1 * cs, origin[1] + r1 * cs
        aim = math.atan2(ty - sy, tx - sx)
        boundary = [origin[0] - 0.4, origin[0] + (w - 0.5) * cs, origin[1] - 0.4, origin[1] + (h - 0.5) * cs]
        rows.append((grid, [sx, sy, aim + rng.uniform(-0.5, 0.5)], [tx, ty, aim], boundary))
    out = _raw(torch, rows, deltas, step, 3000, cell_size=cs, origin=origin)
    statuses = set()
    for i, r in enumerate(rows):
        want = R.solve(r[0], r[1], r[2], r[3], deltas, step, cs, origin, max_iter=3000, max_nodes=MAX_NODES, max_path=MAX_PATH)
        _same(tuple(o[i] for o in out), want, i)
        statuses.add(want["status"])
    assert {R.FOUND, R.NO_PATH} <= statuses
