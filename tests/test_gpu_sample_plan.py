"""t2d_sample_plan on the device: EVERY case of the fixture made by running the reference's RRT.plan, RRTStar.plan and
RRTConnect.plan (tests/golden/sample_plan.npz) as ragged batches through the C interface into sentinel-filled buffers with guard
regions and a patterned workspace; path, path length, status, iterations, node counts and the trees (x, y, parents, costs of the
nodes that exist) BIT-EQUAL to the specification (tests/sample_plan_ref.py); the same cases in reversed order with identical rows;
one query at both ends of a 130-row batch and alone; INVALID, TRUNCATED, MAX_ITER and OVERFLOW rows beside good ones; equal and
different seeds; device tensors in and out on a side stream; the three plan methods against the recorded reference lists; and a
fresh random batch of 256 queries per kind against the specification."""
import numpy as np
import pytest

import sample_plan_ref as R
from test_sample_plan import KINDS, MAX_NODES, MAX_PATH, fixture, fixture_case, n_cases, spec_case

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -12345.0, 7.0e30   # outputs start as SENTINEL; PAD fills the weights no kernel may read
GUARD = 64


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _raw(torch, kind, rows, step, max_iter, radius=3.0, max_nodes=MAX_NODES, max_path=MAX_PATH, cell_size=1.0, origin=(0.0, 0.0), hw=None):
    """t2d_sample_plan through the C interface; rows: (grid, start, target, boundary, seed) each.  Outputs are sentinel-filled with
    a guard region behind them (checked here), the workspace is filled with a pattern -> a list of dicts shaped like the
    specification's, one per row"""
    from tactics2d_amd import _ffi
    lib = _ffi.lib()
    n = len(rows)
    stride = max(r[0].size for r in rows)
    w = np.full((n, stride), PAD)
    for k, r in enumerate(rows):
        w[k, :r[0].size] = r[0].reshape(-1)
    hw = np.int32([r[0].shape for r in rows]) if hw is None else np.int32(hw)
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    w_d, hw_d = t(w, np.float64), t(hw, np.int32)
    s_d, t_d, b_d = (t(np.float64([r[i] for r in rows]), np.float64) for i in (1, 2, 3))
    seed_d = t(np.array([int(r[4]) for r in rows], np.uint64).view(np.int64), np.int64)
    need = lib.t2d_sample_plan_workspace_bytes(n, max_nodes)
    ws = torch.full((need + GUARD,), 0x5a, dtype=torch.uint8, device="cuda")
    path = torch.full((n * max_path * 2 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    small = [torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda") for _ in range(3)]
    nodes = torch.full((2 * n + GUARD,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rc = lib.t2d_sample_plan(0, n, kind, w_d.data_ptr(), hw_d.data_ptr(), stride, s_d.data_ptr(), t_d.data_ptr(), b_d.data_ptr(),
                             seed_d.data_ptr(), step, radius, cell_size, origin[0], origin[1], max_iter, max_nodes, max_path, ws.data_ptr(),
                             need, path.data_ptr(), *(x.data_ptr() for x in small), nodes.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.t2d_last_error(None).decode()
    path, nodes, ws = path.cpu().numpy(), nodes.cpu().numpy(), ws.cpu().numpy()
    path_len, status, iterations = (x.cpu().numpy() for x in small)
    assert (path[n * max_path * 2:] == SENTINEL).all() and all((x[n:] == -7).all() for x in (path_len, status, iterations))
    assert (nodes[2 * n:] == -7).all() and (ws[need:] == 0x5a).all()
    path = path[:n * max_path * 2].reshape(n, max_path, 2)
    out, row = [], need // n
    for i in range(n):
        na, nb = int(nodes[2 * i]), int(nodes[2 * i + 1])
        mem = ws[i * row:(i + 1) * row]
        xy = mem[:16 * max_nodes].view(np.float64).reshape(max_nodes, 2)
        cost = mem[16 * max_nodes:24 * max_nodes].view(np.float64)
        parent = mem[24 * max_nodes:28 * max_nodes].view(np.int32)
        assert na + nb <= max_nodes and (mem[28 * max_nodes:] == 0x5a).all()
        if kind != R.RRT_STAR:
            assert (cost.view(np.uint8) == 0x5a).all()
        assert (xy[na:max_nodes - nb].view(np.uint8) == 0x5a).all() and (parent[na:max_nodes - nb].view(np.uint8) == 0x5a).all()
        out.append(dict(status=int(status[i]), path=path[i], path_len=int(path_len[i]), iterations=int(iterations[i]), nodes=(na, nb),
                        xy=xy[:na].copy(), parent=parent[:na].copy(), cost=cost[:na].copy() if kind == R.RRT_STAR else None,
                        xy_b=xy[::-1][:nb].copy(), parent_b=parent[::-1][:nb].copy()))
    return out


def _same(got, want, what):
    """one row of _raw against a specification dict (or another row of _raw)"""
    key = lambda d: (d["status"], d["path_len"], d["iterations"], tuple(d["nodes"]))
    assert key(got) == key(want), (what, key(got), key(want))
    m = min(got["path_len"], len(got["path"]))
    assert got["path"][:m].tobytes() == want["path"][:m].tobytes(), what
    assert np.isnan(got["path"][m:]).all() and np.isnan(want["path"][m:]).all(), what
    for name in ("xy", "parent", "xy_b", "parent_b"):
        assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(want[name]).tobytes(), (what, name)
    assert (got["cost"] is None) == (want["cost"] is None) and (got["cost"] is None or got["cost"].tobytes() == want["cost"].tobytes()), what


def _row(k):
    c = fixture_case(k)
    return (c["grid"], c["start"], c["target"], c["boundary"], c["seed"])


def _groups():
    """fixture cases that can share a launch: the same kind, extension_step and max_iter"""
    out = {}
    for k in range(n_cases()):
        c = fixture_case(k)
        out.setdefault((c["kind"], c["extension_step"], c["max_iter"]), []).append(k)
    return out


def _launch(torch, ks, **kw):
    c = fixture_case(ks[0])
    return _raw(torch, c["kind"], [_row(k) for k in ks], c["extension_step"], c["max_iter"], c["radius"], **kw)


@pytest.fixture(scope="module")
def forward(torch):
    """every fixture case, one launch per group -> {case: row of _raw}"""
    rows = {}
    for ks in _groups().values():
        for k, got in zip(ks, _launch(torch, ks)):
            rows[k] = got
    return rows


def test_the_whole_fixture_is_bit_equal_to_the_specification(forward):
    g = fixture()
    seen = [0, 0, 0]
    for k in range(n_cases()):
        _same(forward[k], spec_case(k), g["name"][k])
        c = fixture_case(k)
        assert forward[k]["status"] == c["status"], g["name"][k]
        seen[c["kind"]] += forward[k]["status"] == R.FOUND
    assert min(seen) >= 100


def test_reversed_order_changes_no_row(torch, forward):
    for ks in _groups().values():
        ks = ks[::-1]
        for k, got in zip(ks, _launch(torch, ks)):
            _same(got, forward[k], fixture()["name"][k])


@pytest.mark.parametrize("kind", range(3), ids=KINDS)
def test_a_query_gives_the_same_row_at_both_ends_of_a_batch_and_alone(torch, kind):
    g = fixture()
    groups = _groups()
    key = max((key for key in groups if key[0] == kind and key[1] == 1.0), key=lambda key: len(groups[key]))
    ks = groups[key]
    k = max(ks, key=lambda j: g["nodes"][j].sum())
    others = [j for j in ks if j != k]
    others = (others * (128 // len(others) + 1))[:128]
    out = _launch(torch, [k] + others + [k])
    assert len(out) == 130
    for i in (0, 129):
        _same(out[i], spec_case(k), i)
    _same(_launch(torch, [k])[0], spec_case(k), "alone")
    for i, j in enumerate(others):
        _same(out[i + 1], spec_case(j), g["name"][j])


@pytest.mark.parametrize("kind", range(3), ids=KINDS)
def test_invalid_truncated_max_iter_and_overflow_rows_sit_beside_good_ones(torch, kind):
    g = fixture()
    pick = lambda cond: [int(k) for k in np.flatnonzero(cond & (g["kind"] == kind) & (g["extension_step"] == 1.0) & (g["generated"] == 1))]
    total = g["nodes"].sum(axis=1)
    short = pick((g["found"] == 1) & (g["path_len"] <= 4) & (total <= 8))[:3]
    long_ = pick((g["found"] == 1) & (g["path_len"] >= 7) & (total >= 12))[:3]
    stuck = pick(g["found"] == 0)[:2]
    assert len(short) == 3 and len(long_) == 3 and len(stuck) >= 1
    nan, inf = float("nan"), float("inf")
    rows = [list(_row(k)) for k in (short[0], long_[0], stuck[0], short[1], long_[1], short[2], long_[2], stuck[-1])]
    bad = []
    for change in (lambda r: r.__setitem__(1, [nan, 1.0]), lambda r: r.__setitem__(2, [1.0, inf]),
                   lambda r: r.__setitem__(3, [0.0, 4e150, 0.0, 5.0]), lambda r: r.__setitem__(3, [0.0, 5.0, -inf, 5.0])):
        r = list(_row(long_[0]))
        change(r)
        bad.append(r)
    swapped = list(_row(long_[1]))
    swapped[3] = [swapped[3][1], swapped[3][0], swapped[3][2], swapped[3][3]]   # (min > max: not invalid, never a node)
    rows = rows[:2] + bad[:2] + rows[2:5] + bad[2:] + [swapped] + rows[5:]
    for what, kw in (("as they are", {}), ("max_path 5", dict(max_path=5)), ("max_iter 9", dict(max_iter=9)), ("max_nodes 10", dict(max_nodes=10)),
                     ("max_nodes 1", dict(max_nodes=1)), ("max_nodes 2", dict(max_nodes=2))):
        params = {"max_iter": 600, "max_nodes": MAX_NODES, "max_path": MAX_PATH, **kw}
        out = _raw(torch, kind, rows, 1.0, params["max_iter"], 3.0, params["max_nodes"], params["max_path"])
        seen = set()
        for i, r in enumerate(rows):
            want = R.solve(kind, r[0], r[1], r[2], r[3], r[4], 1.0, 3.0, **params)
            _same(out[i], want, (what, i))
            seen.add(want["status"])
        expect = {"as they are": {R.FOUND, R.MAX_ITER}, "max_path 5": {R.TRUNCATED}, "max_iter 9": {R.MAX_ITER}}.get(what, {R.OVERFLOW})
        assert R.INVALID in seen and expect <= seen, (what, seen)
    # an hw that does not fit its row: INVALID, the neighbours as before
    good = _raw(torch, kind, rows, 1.0, 600)
    hw = [r[0].shape for r in rows]
    stride = max(r[0].size for r in rows)
    hw[0], hw[6], hw[len(rows) - 1] = (0, 5), (-3, 4), (stride, 2)
    out = _raw(torch, kind, rows, 1.0, 600, hw=hw)
    for i in range(len(rows)):
        if i in (0, 6, len(rows) - 1):
            assert (out[i]["status"], out[i]["path_len"], out[i]["iterations"], out[i]["nodes"]) == (R.INVALID, 0, 0, (0, 0))
            assert np.isnan(out[i]["path"]).all()
        else:
            _same(out[i], good[i], i)


def test_the_two_trees_of_rrt_connect_meet_in_the_shared_buffer(torch):
    """max_nodes is exactly what the search needs, and one less: the trees fill the buffer from both ends without a gap"""
    g = fixture()
    k = int(np.flatnonzero((g["kind"] == R.RRT_CONNECT) & (g["found"] == 1) & (g["nodes"].min(axis=1) >= 5))[0])
    c, full = fixture_case(k), spec_case(k)
    need = sum(full["nodes"])
    for max_nodes, status in ((need, R.FOUND), (need - 1, R.OVERFLOW)):
        got = _launch(torch, [k, k], max_nodes=max_nodes)
        want = R.solve(c["kind"], c["grid"], c["start"], c["target"], c["boundary"], c["seed"], c["extension_step"], c["radius"],
                       max_iter=c["max_iter"], max_nodes=max_nodes, max_path=MAX_PATH)
        assert want["status"] == status and sum(want["nodes"]) == max_nodes
        for row in got:
            _same(row, want, max_nodes)


@pytest.mark.parametrize("kind", range(3), ids=KINDS)
def test_equal_seeds_give_equal_rows_and_different_seeds_different_trees(torch, kind):
    k = int(np.flatnonzero((fixture()["kind"] == kind) & (fixture()["nodes"].sum(axis=1) > 40))[0])
    c = fixture_case(k)
    row = lambda seed: (c["grid"], c["start"], c["target"], c["boundary"], seed)
    seeds = [c["seed"], 12345, c["seed"], 2 ** 64 - 1, 12345, 0]
    out = _raw(torch, kind, [row(s) for s in seeds], c["extension_step"], c["max_iter"], c["radius"])
    _same(out[0], spec_case(k), "the fixture's seed")
    _same(out[2], out[0], "equal seeds")
    _same(out[4], out[1], "equal seeds")
    for i in (1, 3, 5):
        want = R.solve(kind, c["grid"], c["start"], c["target"], c["boundary"], seeds[i], c["extension_step"], c["radius"],
                       max_iter=c["max_iter"], max_nodes=MAX_NODES, max_path=MAX_PATH)
        _same(out[i], want, seeds[i])
    trees = {out[i]["xy"][1:3].tobytes() for i in (0, 1, 3, 5)}
    assert len(trees) == 4


def test_tensors_in_and_out_on_a_side_stream(torch):
    from tactics2d_amd import search
    g = fixture()
    for kind, cls in enumerate((search.RRT, search.RRTStar, search.RRTConnect)):
        ks = [int(k) for k in np.flatnonzero((g["hw"][:, 0] == 16) & (g["kind"] == kind) & (g["extension_step"] == 0.5) & (g["max_iter"] == 150)
                                             & (g["generated"] == 1))]
        assert len(ks) >= 3
        cases = [fixture_case(k) for k in ks]
        dev = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")
        weights, starts = dev(np.stack([c["grid"] for c in cases])), dev([c["start"] for c in cases])
        targets, bounds = dev([c["target"] for c in cases]), dev([c["boundary"] for c in cases])
        seeds = torch.as_tensor(np.array([c["seed"] for c in cases], np.uint64).view(np.int64), device="cuda")
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        out = cls.plan_batch(starts, targets, bounds, weights, seeds, extension_step=0.5, max_iter=150, max_path=MAX_PATH,
                             max_nodes=MAX_NODES, stream=side)
        side.synchronize()
        assert out._inputs[0].data_ptr() == weights.data_ptr() and out._inputs[2].data_ptr() == starts.data_ptr()
        assert out._inputs[3].data_ptr() == targets.data_ptr() and out._inputs[5].data_ptr() == seeds.data_ptr()
        for x, dt in ((out.path, torch.float64), (out.path_len, torch.int32), (out.status, torch.int32), (out.iterations, torch.int32),
                      (out.nodes, torch.int32), (out.xy, torch.float64), (out.parent, torch.int32)):
            assert x.is_cuda and x.dtype == dt
        assert out.path.shape == (len(ks), MAX_PATH, 2) and out.nodes.shape == (len(ks), 2) and out.xy.shape == (len(ks), MAX_NODES, 2)
        assert out.parent.shape == (len(ks), MAX_NODES) and (out.cost is None) == (kind != R.RRT_STAR)
        path, path_len, status, iterations, nodes = (x.cpu().numpy() for x in (out.path, out.path_len, out.status, out.iterations, out.nodes))
        for i, k in enumerate(ks):
            xy, parent, cost = out.tree(i)
            xy_b, parent_b, _ = out.tree(i, "b")
            _same(dict(status=int(status[i]), path=path[i], path_len=int(path_len[i]), iterations=int(iterations[i]),
                       nodes=tuple(int(v) for v in nodes[i]), xy=xy, parent=parent, cost=cost, xy_b=xy_b, parent_b=parent_b),
                  spec_case(k), g["name"][k])
        # numpy in, one boundary for all rows, ONE integer for the seeds (row_seeds), the default stream
        again = search.sample_plan_batch(KINDS[kind], np.float64([c["start"] for c in cases]), np.float64([c["target"] for c in cases]),
                                         cases[0]["boundary"], np.stack([c["grid"] for c in cases]), 77, extension_step=0.5, max_iter=150,
                                         max_path=MAX_PATH, max_nodes=MAX_NODES)
        derived = R.row_seeds(77, len(ks))
        for i, c in enumerate(cases):
            want = R.solve(kind, c["grid"], c["start"], c["target"], cases[0]["boundary"], int(derived[i]), 0.5, 3.0, max_iter=150,
                           max_nodes=MAX_NODES, max_path=MAX_PATH)
            assert (int(again.status[i]), int(again.path_len[i]), int(again.iterations[i])) == (want["status"], want["path_len"], want["iterations"])
            assert again.path[i].cpu().numpy()[:want["path_len"]].tobytes() == want["path"][:want["path_len"]].tobytes()


def test_plan_returns_the_reference_lists(torch):
    from tactics2d_amd import search
    g = fixture()
    total = g["nodes"].sum(axis=1)
    for kind, cls in enumerate((search.RRT, search.RRTStar, search.RRTConnect)):
        mine = g["kind"] == kind
        picks = [int(np.argmax(np.where(mine, g["path_len"], -1))), int(np.argmax(np.where(mine, total, -1)))] + \
                [int(k) for k in np.flatnonzero(mine & (g["found"] == 0) & (total < 200))[:2]] + \
                [int(k) for k in np.flatnonzero(mine & (g["generated"] == 0))]
        for k in picks:
            c = fixture_case(k)
            args = [list(c["start"]), list(c["target"]), list(c["boundary"]), c["grid"], search.grid_collide if k % 2 else None,
                    c["extension_step"], c["max_iter"]] + ([c["radius"]] if kind == R.RRT_STAR else [])
            path, tree = cls.plan(*args, seed=c["seed"])
            assert isinstance(path, list) and len(path) == len(c["path"]), g["name"][k]
            if path:
                assert all(isinstance(p, list) and len(p) == 2 for p in path)
                assert np.abs(np.float64(path) - c["path"]).max() <= 1e-9, g["name"][k]
            trees = tree if kind == R.RRT_CONNECT else (tree,)
            assert isinstance(tree, tuple if kind == R.RRT_CONNECT else list)
            for got, xy, parent in zip(trees, (c["xy"], c["xy_b"]), (c["parent"], c["parent_b"])):
                assert len(got) == len(xy) and all(isinstance(n, tuple) and len(n) == (4 if kind == R.RRT_STAR else 3) for n in got)
                assert got[0][2] is None and [(-1 if n[2] is None else n[2]) for n in got] == parent.tolist(), g["name"][k]
                assert np.abs(np.float64([n[:2] for n in got]) - xy).max() <= 1e-9
            if kind == R.RRT_STAR:
                assert np.abs(np.float64([n[3] for n in tree]) - c["cost"]).max() <= 1e-9


def test_plan_grows_its_buffers_and_raises_for_an_invalid_row(torch, monkeypatch):
    from tactics2d_amd import search
    grid = np.ones((40, 40))
    grid[30:33, 30:33] = np.inf
    grid[31, 31] = 1.0   # (the target walled in: the tree grows until max_iter)
    args = ([2.0, 2.0], [31.0, 31.0], [0.0, 40.0, 0.0, 40.0], grid, None, 0.3, 5000)
    path, tree = search.RRT.plan(*args, seed=5)
    want = R.solve(R.RRT, grid, args[0], args[1], args[2], 5, 0.3, max_iter=5000, max_nodes=8192, max_path=1024)
    assert want["status"] == R.MAX_ITER and want["nodes"][0] > 4096 and want["path_len"] > 0      # more than plan's first buffer
    assert len(tree) == want["nodes"][0] and len(path) == want["path_len"] and path[-1] == list(tree[-1][:2])
    assert np.float64(path).tobytes() == want["path"][:want["path_len"]].tobytes()
    # a path longer than plan's first 256 points comes back whole
    corridor = np.ones((3, 300))
    path, tree = search.RRT.plan([1.0, 1.0], [298.0, 1.0], [0.0, 299.0, 1.0, 1.0], corridor, None, 1.0, 20000, seed=9)
    assert len(path) > 256 and path[0] == [1.0, 1.0] and path[-1] == [298.0, 1.0]
    monkeypatch.setattr(search, "SAMPLE_PLAN_MAX_NODES", 4096)
    with pytest.raises(RuntimeError) as ei:
        search.RRT.plan(*args, seed=5)
    assert "not finished" in str(ei.value)
    with pytest.raises(ValueError):
        search.RRTConnect.plan([float("nan"), 1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], np.ones((5, 5)), seed=1)


@pytest.mark.parametrize("kind", range(3), ids=KINDS)
def test_a_fresh_random_batch_equals_the_specification(torch, kind):
    """not in the fixture: 256 queries on other 8 x 8 grids, a cell size and an origin that are not 1 and 0, another radius"""
    rng = np.random.RandomState(20261021 + kind)
    step, cs, origin, radius, max_iter = 0.6, 0.8, (-1.5, 2.25), 1.7, 120
    rows = []
    for _ in range(256):
        grid = rng.randint(1, 6, size=(8, 8)).astype(float)
        grid[rng.rand(8, 8) < rng.choice([0.0, 0.1, 0.25])] = np.inf
        if rng.rand() < 0.3:
            grid[rng.randint(8), rng.randint(8)] = np.nan
        free = np.argwhere(np.isfinite(grid))
        (r0, c0), (r1, c1) = free[rng.randint(len(free))], free[rng.randint(len(free))]
        boundary = [origin[0] - 0.4, origin[0] + 7.5 * cs, origin[1] - 0.4, origin[1] + 7.5 * cs]
        rows.append((grid, [origin[0] + c0 * cs, origin[1] + r0 * cs], [origin[0] + c1 * cs, origin[1] + r1 * cs], boundary,
                     int(rng.randint(0, 2 ** 62))))
    out = _raw(torch, kind, rows, step, max_iter, radius, 256, 64, cs, origin)
    statuses = set()
    for i, r in enumerate(rows):
        want = R.solve(kind, r[0], r[1], r[2], r[3], r[4], step, radius, cs, origin, max_iter=max_iter, max_nodes=256, max_path=64)
        _same(out[i], want, i)
        statuses.add(want["status"])
    assert {R.FOUND, R.MAX_ITER} <= statuses
