"""t2d_prm_plan on the device: every case of the fixture made by running the reference's PRM.plan (tests/golden/prm.npz) with at most
256 nodes as ragged batches through the C interface into sentinel-filled buffers with guard regions and a patterned workspace;
status, path, path length, edge count, every edge and its cost, dist and the nodes BIT-EQUAL to the specification (tests/prm_ref.py),
nothing written past the counts; the same cases in reversed order with identical rows; the case at the reference's defaults (1002
nodes); the shapes at which the kernel takes another turn (one node past a wave, past the workgroup, at the cap; k_nearest 1, 16 and
above the node count; exactly max_degree neighbours and one more; no edge at all; coincident nodes; max_path 0, 2 and exactly the
path's length; INVALID rows of each kind at both ends of a 130-row batch of grids of different sizes); equal and different seeds;
device tensors in and out on a side stream; PRM.plan against the recorded reference lists; a fresh random batch of 256 queries per
mode; and a PRM path as the route traffic follows."""
import numpy as np
import pytest

import prm_ref as R
from test_prm import COST_TOL, _by_name, fixture, fixture_case, max_degree_of, max_path_of, n_cases, spec_case

pytestmark = pytest.mark.gpu
SENTINEL, PAD = -12345.0, 7.0e30   # outputs start as SENTINEL; PAD fills the weights no kernel may read
GUARD = 64
FREE = 0x5a   # the workspace's pattern


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def _raw(torch, rows, n_samples, k_nearest=10, radius=None, max_degree=32, max_path=64, cell_size=1.0, origin=(0.0, 0.0), hw=None):
    """t2d_prm_plan through the C interface; rows: (grid, start, target, boundary, seed) each.  Outputs are sentinel-filled with a
    guard region behind them (checked here), the workspace is filled with a pattern, and what a row may not write is checked to
    hold it still -> a list of dicts shaped like the specification's, one per row"""
    from tactics2d_amd import _ffi
    lib = _ffi.lib()
    n = len(rows)
    stride = max(r[0].size for r in rows)
    w = np.full((n, stride), PAD)
    for i, r in enumerate(rows):
        w[i, :r[0].size] = r[0].reshape(-1)
    hw = np.int32([r[0].shape for r in rows]) if hw is None else np.int32(hw)
    t = lambda v, dt: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    w_d, hw_d = t(w, np.float64), t(hw, np.int32)
    s_d, t_d, b_d = (t(np.float64([r[i] for r in rows]), np.float64) for i in (1, 2, 3))
    seed_d = t(np.array([int(r[4]) for r in rows], np.uint64).view(np.int64), np.int64)
    k = k_nearest if radius is None else max_degree
    need = lib.t2d_prm_plan_workspace_bytes(n, n_samples, k)
    nn, ne, o_nodes, o_dist, o_cost, o_ij, o_scratch, row = R.row_layout(n_samples, k)
    assert need == n * row
    ws = torch.full((need + GUARD,), FREE, dtype=torch.uint8, device="cuda")
    path = torch.full((n * max_path * 2 + GUARD,), SENTINEL, dtype=torch.float64, device="cuda")
    small = [torch.full((n + GUARD,), -7, dtype=torch.int32, device="cuda") for _ in range(4)]
    torch.cuda.synchronize()
    rc = lib.t2d_prm_plan(0, n, w_d.data_ptr(), hw_d.data_ptr(), stride, s_d.data_ptr(), t_d.data_ptr(), b_d.data_ptr(), seed_d.data_ptr(),
                          n_samples, k_nearest, 0.0 if radius is None else radius, max_degree, cell_size, origin[0], origin[1], max_path,
                          ws.data_ptr(), need, path.data_ptr(), *(x.data_ptr() for x in small), None)
    torch.cuda.synchronize()
    assert rc == 0, lib.t2d_last_error(None).decode()
    path, ws = path.cpu().numpy(), ws.cpu().numpy()
    path_len, status, n_edges, sweeps = (x.cpu().numpy() for x in small)
    assert (path[n * max_path * 2:] == SENTINEL).all() and all((x[n:] == -7).all() for x in (path_len, status, n_edges, sweeps))
    assert (ws[need:] == FREE).all()
    path = path[:n * max_path * 2].reshape(n, max_path, 2)
    out = []
    for i in range(n):
        mem = ws[i * row:(i + 1) * row]
        m, st = int(n_edges[i]), int(status[i])
        nodes = mem[o_nodes:o_dist].view(np.float64).reshape(nn, 2)
        dist = mem[o_dist:o_cost].view(np.float64)
        cost = mem[o_cost:o_ij].view(np.float64)
        ij = mem[o_ij:o_scratch].view(np.int32).reshape(ne, 2)
        assert 0 <= m <= ne and (mem[o_scratch + 4 * ne:] == FREE).all()
        assert (cost[m:].view(np.uint8) == FREE).all() and (ij[m:].view(np.uint8) == FREE).all()   # nothing past the counts
        if st == R.INVALID:
            assert (mem == FREE).all()
        if st in (R.INVALID, R.OVERFLOW):
            assert m == 0 and (dist.view(np.uint8) == FREE).all()
        out.append(dict(status=st, path=path[i], path_len=int(path_len[i]), n_edges=m, sweeps=int(sweeps[i]),
                        nodes=np.zeros((0, 2)) if st == R.INVALID else nodes.copy(), edge_ij=ij[:m].copy(), edge_cost=cost[:m].copy(),
                        dist=None if st in (R.INVALID, R.OVERFLOW) else dist.copy()))
    return out


def _same(got, want, what):
    """one row of _raw against a specification dict (or another row of _raw)"""
    key = lambda d: (d["status"], d["path_len"], d["n_edges"], d["sweeps"])
    assert key(got) == key(want), (what, key(got), key(want))
    m = min(got["path_len"], len(got["path"]))
    assert got["path"][:m].tobytes() == want["path"][:m].tobytes(), what
    assert np.isnan(got["path"][m:]).all() and np.isnan(want["path"][m:]).all(), what
    for name in ("nodes", "edge_ij", "edge_cost"):
        assert np.ascontiguousarray(got[name]).tobytes() == np.ascontiguousarray(want[name], got[name].dtype).tobytes(), (what, name)
    if got["status"] in (R.FOUND, R.TRUNCATED):   # every walk ends at the start, coincident nodes or not
        assert got["path_len"] >= 2 and (m == 0 or got["path"][0].tobytes() == got["nodes"][0].tobytes()), what
        assert m < got["path_len"] or got["path"][m - 1].tobytes() == got["nodes"][1].tobytes(), what
    assert (got["dist"] is None) == (want["dist"] is None) and (got["dist"] is None or got["dist"].tobytes() == want["dist"].tobytes()), what


def _row(k):
    c = fixture_case(k)
    return (c["grid"], c["start"], c["target"], c["boundary"], c["seed"])


def _groups(limit=256):
    """fixture cases that can share a launch: the same n_samples, k_nearest and radius"""
    out = {}
    for k in range(n_cases()):
        c = fixture_case(k)
        if c["n_samples"] + 2 <= limit:
            out.setdefault((c["n_samples"], c["k_nearest"] if c["radius"] is None else 0, c["radius"]), []).append(k)
    return out


def _launch(torch, ks, **kw):
    c = fixture_case(ks[0])
    params = dict(k_nearest=c["k_nearest"], radius=c["radius"], max_degree=max_degree_of(c), max_path=max_path_of(c))
    params.update(kw)
    return _raw(torch, [_row(k) for k in ks], c["n_samples"], **params)


@pytest.fixture(scope="module")
def forward(torch):
    """every fixture case of at most 256 nodes, one launch per group -> {case: row of _raw}"""
    rows = {}
    for ks in _groups().values():
        for k, got in zip(ks, _launch(torch, ks)):
            rows[k] = got
    return rows


def test_the_fixture_is_bit_equal_to_the_specification(forward):
    assert len(forward) == n_cases() - 1   # (all but the case at the reference's defaults)
    found = [0, 0]
    for k, got in forward.items():
        c = fixture_case(k)
        _same(got, spec_case(k), c["name"])
        assert got["status"] == (R.FOUND if c["found"] else R.NO_PATH), c["name"]
        found[c["radius"] is not None] += got["status"] == R.FOUND
    assert min(found) >= 25


def test_reversed_order_changes_no_row(torch, forward):
    for ks in _groups().values():
        ks = ks[::-1]
        for k, got in zip(ks, _launch(torch, ks)):
            _same(got, forward[k], fixture()["name"][k])


def test_the_case_at_the_references_defaults(torch):
    k = _by_name("the_reference_defaults")
    got = _launch(torch, [k, k])
    for row in got:
        _same(row, spec_case(k), "1002 nodes, k 10")
    assert got[0]["status"] == R.FOUND and got[0]["n_edges"] > 3000


def _scene(seed, side=12, proportion=0.12):
    rng = np.random.RandomState(seed)
    grid = rng.randint(1, 6, size=(side, side)).astype(float)
    grid[rng.rand(side, side) < proportion] = np.inf
    grid[:2, :2] = grid[-2:, -2:] = 1.0
    return grid, [0.5, 0.5], [side - 1.25, side - 1.5], [0.0, float(side), 0.0, float(side)]


@pytest.mark.parametrize("n_samples,k", [(1, 10), (62, 10), (63, 10), (254, 10), (255, 10), (1022, 10), (120, 1), (120, 16), (9, 16), (14, 15)],
                         ids=lambda v: str(v))
def test_node_counts_and_k_at_the_turns_of_the_kernel(torch, n_samples, k):
    """65 nodes: one past a wave; 256 and 257: the workgroup's width and one past it; 1024: the cap; k_nearest 1 and 16; k_nearest
    above and at the node count"""
    rows = [_scene(40 + i) + (1000 + 7 * i,) for i in range(3 if n_samples < 1000 else 2)]
    out = _raw(torch, rows, n_samples, k, max_path=48)
    for i, r in enumerate(rows):
        want = R.solve(r[0], r[1], r[2], r[3], r[4], n_samples, k, max_path=48)
        _same(out[i], want, i)
        assert want["status"] in (R.FOUND, R.NO_PATH) and len(want["nodes"]) == n_samples + 2
    if n_samples >= 62 and k >= 10:   # (a node joined to its one nearest makes islands, not a roadmap)
        assert any(o["status"] == R.FOUND for o in out)


def test_radius_mode_at_exactly_max_degree_and_one_more_beside_good_rows(torch):
    rows = [_scene(60 + i) + (2000 + i,) for i in range(5)]
    radius, n_samples = 2.0, 100
    specs = [R.solve(*r, n_samples, 10, radius, max_degree=n_samples + 2, max_path=48) for r in rows]
    tops = [max(len(R.neighbours(s["nodes"], i, 0, radius)) for i in range(n_samples + 2)) for s in specs]
    assert len(set(tops)) >= 2
    cap = sorted(tops)[len(tops) // 2]   # some rows have a node with more, some have not, one has a node with exactly this many
    out = _raw(torch, rows, n_samples, radius=radius, max_degree=cap, max_path=48)
    seen = set()
    for i, r in enumerate(rows):
        want = R.solve(*r, n_samples, 10, radius, max_degree=cap, max_path=48)
        _same(out[i], want, i)
        assert want["status"] == (R.OVERFLOW if tops[i] > cap else specs[i]["status"])
        seen.add((tops[i] > cap) - (tops[i] < cap))
    assert {0, 1} <= seen
    out = _raw(torch, rows, n_samples, radius=radius, max_degree=cap - 1, max_path=48)
    assert out[tops.index(cap)]["status"] == R.OVERFLOW   # one more than the cap


def test_no_edge_at_all_and_coincident_nodes(torch):
    grid, start, target, boundary = _scene(77)
    out = _raw(torch, [(grid, start, target, boundary, 5)] * 2, 40, radius=1e-4, max_degree=4, max_path=8)
    want = R.solve(grid, start, target, boundary, 5, 40, 10, 1e-4, max_degree=4, max_path=8)
    assert (want["status"], want["n_edges"], want["sweeps"]) == (R.NO_PATH, 0, 1)
    for row in out:
        _same(row, want, "no edge")
    # start == target, and a boundary one ulp wide each way -- the narrowest the reference accepts: every sample lands on one of its
    # four corners, so most nodes coincide exactly and the smaller index is the nearer
    free = np.ones((6, 6))
    a, b = 2.25, 3.5
    tiny = [a, float(np.nextafter(a, 9.0)), b, float(np.nextafter(b, 9.0))]
    rows = [(free, [a, b], [a, b], tiny, 9), (free, [a, b], [tiny[1], tiny[3]], tiny, 10), (free, [1.0, 1.0], [1.0, 1.0], [0.0, 6.0, 0.0, 6.0], 11)]
    for k, radius in ((3, None), (16, None), (10, 1e-12)):
        out = _raw(torch, rows, 30, k, radius, max_degree=32, max_path=8)
        for i, r in enumerate(rows):
            want = R.solve(*r, 30, k, radius, max_degree=32, max_path=8)
            _same(out[i], want, (k, radius, i))
        assert out[0]["status"] == R.FOUND and out[0]["path_len"] == 2 and out[0]["dist"][1] == 0.0
        assert len(np.unique(out[0]["nodes"], axis=0)) <= 4
        assert out[2]["status"] == R.FOUND and tuple(out[2]["edge_ij"][0]) == (0, 1) and out[2]["edge_cost"][0] == 0.0


def test_max_path_0_2_and_exactly_the_paths_length(torch):
    k = _by_name("wall_with_one_gap_k")
    full = spec_case(k)
    assert full["status"] == R.FOUND and full["path_len"] > 2
    for max_path, status in ((0, R.TRUNCATED), (2, R.TRUNCATED), (full["path_len"] - 1, R.TRUNCATED), (full["path_len"], R.FOUND)):
        got = _launch(torch, [k, k], max_path=max_path)
        c = fixture_case(k)
        want = R.solve(c["grid"], c["start"], c["target"], c["boundary"], c["seed"], c["n_samples"], c["k_nearest"], max_path=max_path)
        assert want["status"] == status and want["path_len"] == full["path_len"]
        for row in got:
            _same(row, want, max_path)


def test_invalid_rows_of_each_kind_at_both_ends_of_a_130_row_batch_of_grids_of_different_sizes(torch):
    nan, inf = float("nan"), float("inf")
    good = []
    for i in range(120):
        side = 6 + i % 7
        good.append(_scene(300 + i, side) + (3000 + i,))
    g, s, t, b = _scene(299, 9)
    bad = [(g, [nan, 1.0], t, b, 1), (g, s, [1.0, inf], b, 1), (g, s, t, [0.0, 4e150, 0.0, 9.0], 1), (g, s, t, [0.0, 9.0, -inf, 9.0], 1),
           (g, s, t, [9.0, 0.0, 0.0, 9.0], 1), (g, s, t, [0.0, 9.0, 4.0, 4.0], 1), (g, [-1e-6, 0.5], t, b, 1), (g, s, [4.0, 9.0 + 1e-6], b, 1),
           (g, [9.5, 0.5], t, b, 1), (g, s, [4.0, -0.5], b, 1)]
    rows = bad[:5] + good + bad[5:]
    assert len(rows) == 130
    out = _raw(torch, rows, 30, 6, max_path=32)
    statuses = set()
    for i, r in enumerate(rows):
        want = R.solve(*r, 30, 6, max_path=32)
        _same(out[i], want, i)
        assert (want["status"] == R.INVALID) == (i < 5 or i >= 125)
        statuses.add(want["status"])
    assert {R.FOUND, R.NO_PATH, R.INVALID} <= statuses
    # an hw that does not fit its row: INVALID, the neighbours as before
    hw = [r[0].shape for r in rows]
    stride = max(r[0].size for r in rows)
    hw[5], hw[60], hw[124] = (0, 5), (-3, 4), (stride, 2)
    again = _raw(torch, rows, 30, 6, max_path=32, hw=hw)
    for i in range(len(rows)):
        if i in (5, 60, 124):
            assert (again[i]["status"], again[i]["path_len"], again[i]["n_edges"], again[i]["sweeps"]) == (R.INVALID, 0, 0, 0)
            assert np.isnan(again[i]["path"]).all()
        else:
            _same(again[i], out[i], i)


def test_equal_seeds_give_equal_rows_and_different_seeds_different_roadmaps(torch):
    grid, start, target, boundary = _scene(88)
    seeds = [4242, 12345, 4242, 2 ** 64 - 1, 12345, 0]
    out = _raw(torch, [(grid, start, target, boundary, s) for s in seeds], 90, 8, max_path=40)
    for i, s in enumerate(seeds):
        _same(out[i], R.solve(grid, start, target, boundary, s, 90, 8, max_path=40), s)
    _same(out[2], out[0], "equal seeds")
    _same(out[4], out[1], "equal seeds")
    assert len({out[i]["nodes"][2:4].tobytes() for i in (0, 1, 3, 5)}) == 4 and len({out[i]["edge_ij"].tobytes() for i in (0, 1, 3, 5)}) == 4


def test_tensors_in_and_out_on_a_side_stream_and_an_integer_for_the_seeds(torch):
    from tactics2d_amd import search
    scenes = [_scene(500 + i) for i in range(6)]
    seeds = np.array([77 + i for i in range(6)], np.uint64)
    dev = lambda v: torch.as_tensor(np.ascontiguousarray(v, np.float64), device="cuda")
    weights, starts = dev(np.stack([s[0] for s in scenes])), dev([s[1] for s in scenes])
    targets, bounds = dev([s[2] for s in scenes]), dev([s[3] for s in scenes])
    seed_t = torch.as_tensor(seeds.view(np.int64), device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    for kw in (dict(k_nearest=7), dict(connection_radius=2.5, max_degree=40)):
        out = search.PRM.plan_batch(starts, targets, bounds, weights, seed_t, n_samples=80, max_path=40, stream=side, **kw)
        side.synchronize()
        assert out._inputs[0].data_ptr() == weights.data_ptr() and out._inputs[2].data_ptr() == starts.data_ptr()
        assert out._inputs[3].data_ptr() == targets.data_ptr() and out._inputs[5].data_ptr() == seed_t.data_ptr()
        for x, dt in ((out.path, torch.float64), (out.path_len, torch.int32), (out.status, torch.int32), (out.n_edges, torch.int32),
                      (out.sweeps, torch.int32), (out.nodes, torch.float64), (out.edge_ij, torch.int32), (out.edge_cost, torch.float64),
                      (out.dist, torch.float64)):
            assert x.is_cuda and x.dtype == dt
        max_edges = 82 * min(kw.get("max_degree", kw.get("k_nearest")), 81)
        assert out.path.shape == (6, 40, 2) and out.nodes.shape == (6, 82, 2) and out.dist.shape == (6, 82)
        assert out.edge_ij.shape == (6, max_edges, 2) and out.edge_cost.shape == (6, max_edges)
        for i, s in enumerate(scenes):
            want = R.solve(*s, int(seeds[i]), 80, kw.get("k_nearest", 10), kw.get("connection_radius"), kw.get("max_degree", 32), max_path=40)
            m = want["n_edges"]
            got = dict(status=int(out.status[i]), path=out.path[i].cpu().numpy(), path_len=int(out.path_len[i]), n_edges=int(out.n_edges[i]),
                       sweeps=int(out.sweeps[i]), nodes=out.nodes[i].cpu().numpy(), edge_ij=out.edge_ij[i, :m].cpu().numpy(),
                       edge_cost=out.edge_cost[i, :m].cpu().numpy(), dist=out.dist[i].cpu().numpy())
            _same(got, want, i)
            nodes, edges = out.roadmap(i)
            assert nodes == want["nodes"].tolist() and edges == [(int(a), int(b), float(c)) for (a, b), c in zip(want["edge_ij"], want["edge_cost"])]
    # numpy in, one boundary for all rows, ONE integer for the seeds (row_seeds), the default stream
    again = search.prm_plan_batch(np.float64([s[1] for s in scenes]), np.float64([s[2] for s in scenes]), scenes[0][3],
                                  np.stack([s[0] for s in scenes]), 77, n_samples=80, k_nearest=7, max_path=40)
    derived = search.row_seeds(77, 6)
    assert derived.tolist() == R.row_seeds(77, 6).tolist()
    for i, s in enumerate(scenes):
        want = R.solve(*s, int(derived[i]), 80, 7, max_path=40)
        assert (int(again.status[i]), int(again.path_len[i]), int(again.n_edges[i])) == (want["status"], want["path_len"], want["n_edges"])
        assert again.nodes[i].cpu().numpy().tobytes() == want["nodes"].tobytes()
        assert again.path[i].cpu().numpy()[:want["path_len"]].tobytes() == want["path"][:want["path_len"]].tobytes()


def test_an_empty_batch_gives_empty_tensors_of_the_same_shapes(torch):
    from tactics2d_amd import search
    for kw, max_edges in ((dict(k_nearest=7), 82 * 7), (dict(connection_radius=2.0, max_degree=200), 82 * 81)):
        out = search.prm_plan_batch(np.zeros((0, 2)), np.zeros((0, 2)), np.zeros((0, 4)), np.ones((0, 5, 5)), np.zeros(0, np.uint64),
                                    n_samples=80, max_path=12, **kw)
        torch.cuda.synchronize()
        assert out.path.shape == (0, 12, 2) and out.nodes.shape == (0, 82, 2) and out.dist.shape == (0, 82)
        assert out.edge_ij.shape == (0, max_edges, 2) and out.edge_cost.shape == (0, max_edges)
        assert all(x.shape == (0,) and x.dtype == torch.int32 for x in (out.path_len, out.status, out.n_edges, out.sweeps))
        assert out.nodes.dtype == out.dist.dtype == out.edge_cost.dtype == torch.float64 and out.edge_ij.dtype == torch.int32
        assert all(x.is_cuda for x in (out.path, out.nodes, out.dist, out.edge_ij, out.edge_cost))


def test_plan_returns_the_reference_lists(torch):
    from tactics2d_amd import search
    g = fixture()
    picks = [int(np.flatnonzero((g["has_cost"] == 1) & (g["found"] == 1) & (g["radius"] == 0) & (g["n_samples"] >= 126))[0]),
             int(np.flatnonzero((g["has_cost"] == 1) & (g["found"] == 1) & (g["radius"] > 0) & (g["n_samples"] >= 62))[0]),
             _by_name("wall_without_a_gap"), _by_name("radius_too_small_for_any_edge")]
    for k in picks:
        c = fixture_case(k)
        path, (nodes, edges) = search.PRM.plan(list(c["start"]), list(c["target"]), list(c["boundary"]), c["grid"],
                                               search.grid_collide if k % 2 else None, c["n_samples"], c["k_nearest"], c["radius"], seed=c["seed"])
        assert isinstance(path, list) and isinstance(nodes, list) and isinstance(edges, list)
        assert len(path) == len(c["path"]) and (len(path) > 0) == bool(c["found"]), c["name"]
        assert all(isinstance(p, list) and len(p) == 2 for p in path + nodes) and np.float64(path).reshape(-1, 2).tobytes() == c["path"].tobytes()
        assert len(nodes) == c["n_samples"] + 2 and nodes[0] == list(c["start"]) and nodes[1] == list(c["target"])
        assert all(isinstance(e, tuple) and len(e) == 3 and isinstance(e[2], float) for e in edges) and len(edges) == len(c["edge_ij"])
        got = {(i, j): w for i, j, w in edges}
        if c["radius"] is None:
            assert [(i, j) for i, j, _ in edges] == [tuple(e) for e in c["edge_ij"].tolist()], c["name"]
        assert set(got) == {tuple(e) for e in c["edge_ij"].tolist()}, c["name"]
        for (i, j), w in zip(c["edge_ij"].tolist(), c["edge_cost"]):
            assert abs(got[(i, j)] - w) <= COST_TOL * w, (c["name"], i, j)
    # a max_iter the reference's search could run into is refused, one at the bound is not
    c = fixture_case(picks[0])
    args = (list(c["start"]), list(c["target"]), list(c["boundary"]), c["grid"], None, c["n_samples"], c["k_nearest"], None)
    with pytest.raises(ValueError, match="binding max_iter is not modelled"):
        search.PRM.plan(*args, 2 * len(c["edge_ij"]), seed=c["seed"])
    assert search.PRM.plan(*args, 2 * len(c["edge_ij"]) + 1, seed=c["seed"])[0] == c["path"].tolist()


def test_plan_grows_its_buffers(torch, monkeypatch):
    from tactics2d_amd import search
    # radius mode with more than 32 neighbours per node: the room doubles until the roadmap fits
    grid = np.ones((6, 6))
    args = ([0.5, 0.5], [5.0, 5.0], [0.0, 6.0, 0.0, 6.0], grid, None, 150, 10, 3.0)
    path, (nodes, edges) = search.PRM.plan(*args, seed=3)
    want = R.solve(grid, args[0], args[1], args[2], 3, 150, 10, 3.0, max_degree=152)
    assert max(np.bincount(want["edge_ij"].reshape(-1))) > 32 and len(edges) == want["n_edges"]
    assert np.float64(path).tobytes() == want["path"][:want["path_len"]].tobytes()
    monkeypatch.setattr(search, "PRM_PLAN_MAX_DEGREE", 32)
    with pytest.raises(RuntimeError, match="not finished"):
        search.PRM.plan(*args, seed=3)
    monkeypatch.undo()
    # a path longer than plan's first buffer comes back whole (a roadmap of at most 1024 nodes has no path of 256 points worth the
    # name, so the first buffer is made 2 points here: plan asks once more with the path's length)
    real, asked = search.prm_plan_batch, []

    def small_first(*a, max_path=256, **kw):
        asked.append(max_path)
        return real(*a, max_path=2 if max_path == 256 else max_path, **kw)
    monkeypatch.setattr(search, "prm_plan_batch", small_first)
    scene = _scene(41)
    path, (nodes, edges) = search.PRM.plan(scene[1], scene[2], scene[3], scene[0], None, 120, 8, seed=6)
    want = R.solve(*scene, 6, 120, 8, max_path=122)
    assert want["path_len"] > 2 and asked == [256, want["path_len"]]
    assert len(path) == want["path_len"] and np.float64(path).tobytes() == want["path"][:want["path_len"]].tobytes()
    monkeypatch.undo()
    with pytest.raises(ValueError):
        search.PRM.plan([float("nan"), 1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], np.ones((5, 5)), seed=1)


@pytest.mark.parametrize("mode", ["k_nearest", "radius"])
def test_a_fresh_random_batch_equals_the_specification(torch, mode):
    """not in the fixture: 256 queries on other 8 x 8 grids, a cell size and an origin that are not 1 and 0"""
    rng = np.random.RandomState(20261021 + (mode == "radius"))
    cs, origin, n_samples = 0.8, (-1.5, 2.25), 45
    kw = dict(k_nearest=6) if mode == "k_nearest" else dict(radius=1.3, max_degree=14)
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
    out = _raw(torch, rows, n_samples, max_path=24, cell_size=cs, origin=origin, **kw)
    statuses = set()
    for i, r in enumerate(rows):
        want = R.solve(*r, n_samples, kw.get("k_nearest", 10), kw.get("radius"), kw.get("max_degree", 32), cs, origin, max_path=24)
        _same(out[i], want, i)
        statuses.add(want["status"])
    assert {R.FOUND, R.NO_PATH} <= statuses and (mode == "k_nearest" or R.OVERFLOW in statuses)


def test_a_prm_path_becomes_the_route(torch):
    """what tests/test_gpu_polyline_routes.py asks of an RRT path: the route vertices written on the device from `path` / `path_len`
    equal the same polylines installed from the host"""
    from route_writers import A, N_ENV, placeholder, route_pool
    from tactics2d_amd import search
    rng = np.random.RandomState(5)
    grids = np.ones((N_ENV, 16, 16))
    for e in range(N_ENV):
        grids[e][rng.rand(16, 16) < 0.08] = np.inf
        grids[e][:3, :3] = grids[e][12:, 12:] = 1.0
    starts = np.float64([[1.0, 1.0]] * N_ENV)
    targets = np.float64([[13.0 + 0.1 * e, 14.0] for e in range(N_ENV)])
    out = search.PRM.plan_batch(starts, targets, [0.0, 16.0, 0.0, 16.0], grids, 11, n_samples=200, k_nearest=8, max_path=64)
    assert (out.status.cpu().numpy() == search.PRM_FOUND).all() and out.path.shape == (N_ENV, 64, 2)
    pts, counts = out.path.cpu().numpy(), out.path_len.cpu().numpy()
    assert counts.min() >= 3
    caps = [int(c) + extra for c, extra in zip(counts, (0, 1, 9, 40, 0, 2, 5, 1))]
    z = np.zeros(N_ENV * A, np.float32)
    pool = route_pool(z, z, z, z)
    pool.set_routes([[placeholder(caps[e], e)] for e in range(N_ENV)], np.arange(N_ENV), 0, 1.5)
    count = pool.polyline_routes(out.path, out.path_len)
    pool.sync()
    assert count.cpu().tolist() == counts.tolist()
    host = route_pool(z, z, z, z)
    lines = []
    for e in range(N_ENV):
        xy = pts[e, :counts[e]].astype(np.float32)
        lines.append([np.concatenate([xy, np.repeat(xy[-1:], caps[e] - counts[e], 0)])])
    host.set_routes(lines, np.arange(N_ENV), 0, 1.5)
    assert np.array_equal(pool.route_vertices().cpu().numpy(), host.route_vertices().cpu().numpy())
    pool.close()
    host.close()
