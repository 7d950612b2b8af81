"""The probabilistic roadmap without a device: the specification (tests/prm_ref.py: the reference's phases on the build's counter
stream, the KD-tree as the k smallest squared distances by (d2, index), the heap as the min-plus fixed point with grid_pred's
predecessor rule) against the fixture made by running the reference's own PRM.plan on the same draws (tests/golden/prm.npz,
tests/golden/make_prm.py): node count, edge count, every edge, path length and every path node EQUAL (edges in order in k-nearest
mode, as sorted sets in radius mode), path coordinates bit-equal, edge costs within 4 ulp; the fixed point against a heap Dijkstra
written as the reference's loop; the findings; the host-side refusals of PRM.plan and prm_plan_batch; header <-> _ffi <-> layout;
the entry point's refusals, which need no device; the fixture reproduced byte for byte where the reference tree is present."""
import ctypes as C
import heapq
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import prm_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("TACTICS2D_REFERENCE", "/root/reference")
_CACHE = {}
ULP = 2.0 ** -52
COST_TOL = 4 * ULP   # both sides are a sqrt of a two-term sum of squares, with or without a fused multiply-add


def fixture():
    if "g" not in _CACHE:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "prm.npz")))
        g["grid_off"] = np.concatenate([[0], np.cumsum(g["hw"][:, 0] * g["hw"][:, 1])])
        g["path_off"] = np.concatenate([[0], np.cumsum(g["path_len"])])
        g["edge_off"] = np.concatenate([[0], np.cumsum(g["n_edges"])])
        g["cost_off"] = np.concatenate([[0], np.cumsum(np.where(g["has_cost"] == 1, g["n_edges"], 0))])
        _CACHE["g"] = g
    return _CACHE["g"]


def n_cases():
    return len(fixture()["name"])


def fixture_case(k):
    """dict(name, grid [H, W], start, target, boundary, n_samples, k_nearest, radius (None: k-nearest mode), seed, found, path
    [len, 2], edge_ij int [n_edges, 2], edge_cost [n_edges] or None) of case k"""
    g = fixture()
    h, w = (int(v) for v in g["hw"][k])
    radius = float(g["radius"][k])
    return dict(name=str(g["name"][k]), grid=g["grid"][g["grid_off"][k]:g["grid_off"][k + 1]].reshape(h, w), start=g["start"][k],
                target=g["target"][k], boundary=g["boundary"][k], n_samples=int(g["n_samples"][k]), k_nearest=int(g["k_nearest"][k]),
                radius=radius if radius > 0 else None, seed=int(g["seed"][k]), found=int(g["found"][k]),
                path=g["path"][g["path_off"][k]:g["path_off"][k + 1]], edge_ij=g["edge_ij"][g["edge_off"][k]:g["edge_off"][k + 1]].astype(np.int64),
                edge_cost=g["edge_cost"][g["cost_off"][k]:g["cost_off"][k + 1]] if g["has_cost"][k] else None)


def max_degree_of(c):
    """what the fixture's cases run with, here and on the device: radius mode without a binding cap, as the reference has none"""
    return c["n_samples"] + 2


def max_path_of(c):
    return 64 if c["n_samples"] + 2 > 64 else c["n_samples"] + 2   # (the fixture's longest path has fewer points)


def solve_case(c, **kw):
    params = dict(n_samples=c["n_samples"], k_nearest=c["k_nearest"], connection_radius=c["radius"], max_degree=max_degree_of(c),
                  max_path=max_path_of(c))
    params.update(kw)
    return R.solve(c["grid"], c["start"], c["target"], c["boundary"], c["seed"], **params)


def spec_case(k):
    """the specification's answer to fixture case k, computed once and shared (read only)"""
    if ("spec", k) not in _CACHE:
        _CACHE["spec", k] = solve_case(fixture_case(k))
    return _CACHE["spec", k]


def _by_name(name):
    return int(np.flatnonzero(fixture()["name"] == name)[0])


def heap_dijkstra(n_nodes, edges):
    """the reference's loop (prm.py:249-323) over the CSR rows of its symmetric matrix, run until the heap is empty instead of
    stopping at the target: dist, prev"""
    rows = [[] for _ in range(n_nodes)]
    for i, j, w in edges:
        rows[i].append((j, w))
        rows[j].append((i, w))
    for r in rows:
        r.sort()   # (CSR: a row's columns ascend)
    dist = [float("inf")] * n_nodes
    prev = [-1] * n_nodes
    dist[0] = 0.0
    pq = [(0.0, 0)]
    pops = 0
    while pq:
        pops += 1
        current_dist, current = heapq.heappop(pq)
        if current_dist > dist[current]:
            continue
        for neighbor, weight in rows[current]:
            new_dist = current_dist + weight
            if new_dist < dist[neighbor]:
                dist[neighbor] = new_dist
                prev[neighbor] = current
                heapq.heappush(pq, (new_dist, neighbor))
    return np.array(dist), np.array(prev), pops


# ---- the fixture itself ------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    g = fixture()
    radius, found, ns = g["radius"], g["found"], g["n_samples"]
    assert (radius == 0).sum() >= 100 and (radius > 0).sum() >= 60 and found.sum() >= 60 and (found == 0).sum() >= 60
    gen = g["generated"] == 1
    assert set(ns[gen]) == {1, 8, 62, 126, 254} and set(g["k_nearest"][gen & (radius == 0)]) == {3, 10} and set(radius[gen]) == {0.0, 2.5, 5.0}
    assert set((int(a), int(b)) for a, b in g["hw"][gen]) == {(6, 6), (9, 14), (16, 16), (24, 24)}
    assert set(g["obstacle_proportion"][gen]) == {0.0, 0.1, 0.3}
    names = set(str(v) for v in g["name"])
    assert {"one_sample_k", "one_sample_radius", "k_nearest_above_the_node_count", "no_obstacles_k", "radius_too_small_for_any_edge",
            "start_inside_an_obstacle", "target_inside_an_obstacle", "wall_with_one_gap_k", "wall_with_one_gap_radius",
            "the_reference_defaults", "nan_is_an_obstacle"} <= names
    k = _by_name("the_reference_defaults")
    assert (ns[k], g["k_nearest"][k], radius[k]) == (1000, 10, 0.0) and found[k] == 1
    assert g["n_edges"][_by_name("radius_too_small_for_any_edge")] == 0
    assert (g["n_edges"] <= 32767).all() and g["path_len"].max() <= 64
    # the costs are recorded for a stated subset
    assert g["has_cost"].sum() >= 40 and len(g["edge_cost"]) == g["n_edges"][g["has_cost"] == 1].sum()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "prm.npz")) <= os.path.getsize(os.path.join(ROOT, "tests", "golden", "sample_plan.npz"))


def test_the_specification_equals_the_reference_on_the_fixture():
    g = fixture()
    worst = 0.0
    for k in range(n_cases()):
        c, s = fixture_case(k), spec_case(k)
        name = c["name"]
        assert len(s["nodes"]) == c["n_samples"] + 2, name
        assert s["status"] == (R.FOUND if c["found"] else R.NO_PATH), name
        assert s["n_edges"] == len(c["edge_ij"]) == g["n_edges"][k], name
        got, want = s["edge_ij"].astype(np.int64), c["edge_ij"]
        key = lambda e: np.lexsort((e[:, 1], e[:, 0])) if len(e) else np.zeros(0, np.int64)
        if c["radius"] is None:
            assert np.array_equal(got, want), name                      # in the reference's order
        else:
            assert np.array_equal(got[key(got)], want[key(want)]), name   # as sorted sets
        assert s["path_len"] == len(c["path"]), name
        assert s["path"][:s["path_len"]].tobytes() == np.ascontiguousarray(c["path"]).tobytes(), name   # (the nodes themselves)
        if c["edge_cost"] is not None and len(want):
            mine = s["edge_cost"][key(got)] if c["radius"] is not None else s["edge_cost"]
            theirs = c["edge_cost"][key(want)] if c["radius"] is not None else c["edge_cost"]
            rel = np.abs(mine - theirs) / theirs
            assert rel.max() <= COST_TOL, (name, rel.max())
            worst = max(worst, float(rel.max()))
    print(f"largest relative difference of an edge cost over the fixture: {worst:.3g}")


def test_the_findings_the_fixture_records():
    g = fixture()
    # a sampled point is never collision-checked: a start or target inside an obstacle stays as an ISOLATED node, hence no path
    for name, node in (("start_inside_an_obstacle", 0), ("target_inside_an_obstacle", 1), ("target_inside_an_obstacle_radius", 1)):
        c = fixture_case(_by_name(name))
        assert not c["found"] and len(c["edge_ij"]) > 0 and not (c["edge_ij"] == node).any(), name
    # ... and so do samples inside obstacles, in most generated cases with obstacles
    seen = 0
    for k in np.flatnonzero((g["generated"] == 1) & (g["obstacle_proportion"] == 0.3) & (g["n_samples"] == 254) & (g["radius"] == 0))[:4]:
        c, s = fixture_case(k), spec_case(k)
        obst = R.obstacle_mask(c["grid"])
        inside = [i for i, (x, y) in enumerate(s["nodes"]) if 0 <= round(y) < obst.shape[0] and 0 <= round(x) < obst.shape[1]
                  and obst[int(round(y)), int(round(x))] and abs(x - round(x)) < 0.5 and abs(y - round(y)) < 0.5]
        assert inside and not np.isin(c["edge_ij"], inside).any(), c["name"]
        seen += 1
    assert seen >= 2
    # the asymmetric neighbour rule: some pair (i, j), i < j, has i among j's nearest and is NO edge because j is not among i's,
    # although its segment is free
    asym = 0
    for k in np.flatnonzero((g["generated"] == 1) & (g["obstacle_proportion"] == 0.0) & (g["n_samples"] == 126) & (g["k_nearest"] == 3)
                            & (g["radius"] == 0)):
        c, s = fixture_case(k), spec_case(k)
        edges = set(map(tuple, c["edge_ij"].tolist()))
        for j in range(len(s["nodes"])):
            for i in R.neighbours(s["nodes"], j, 3, None):
                asym += i < j and (int(i), j) not in edges
    assert asym >= 10
    # a radius too small for any edge: the reference skips its search and returns []
    c = fixture_case(_by_name("radius_too_small_for_any_edge"))
    assert not c["found"] and len(c["path"]) == 0
    s = spec_case(_by_name("radius_too_small_for_any_edge"))
    assert (s["status"], s["n_edges"], s["sweeps"]) == (R.NO_PATH, 0, 1) and s["dist"][0] == 0 and np.isinf(s["dist"][1:]).all()
    # k_nearest above the node count: every node is every other node's neighbour
    c = fixture_case(_by_name("k_nearest_above_the_node_count"))
    assert sorted(map(tuple, c["edge_ij"].tolist())) == [(i, j) for i in range(5) for j in range(i + 1, 5)]


def test_the_fixed_point_equals_the_references_heap_on_the_specifications_roadmaps():
    picks = list(range(0, n_cases(), 5)) + [_by_name(n) for n in ("the_reference_defaults", "wall_with_one_gap_k", "wall_without_a_gap")]
    connected = 0
    for k in picks:
        s = spec_case(k)
        edges = [(int(i), int(j), float(w)) for (i, j), w in zip(s["edge_ij"], s["edge_cost"])]
        dist, prev, pops = heap_dijkstra(len(s["nodes"]), edges)
        assert dist.tobytes() == s["dist"].tobytes(), fixture()["name"][k]   # g bit for bit
        assert np.array_equal(prev, s["pred"]), fixture()["name"][k]
        assert pops <= 2 * len(edges) + 1   # (what PRM.plan holds max_iter against)
        connected += int(np.isfinite(dist).sum() > 2)
    assert connected >= 20


def test_statuses_caps_and_build_defined_rows_of_the_specification():
    c = fixture_case(_by_name("wall_with_one_gap_k"))
    full = spec_case(_by_name("wall_with_one_gap_k"))
    assert full["status"] == R.FOUND and full["path_len"] >= 4
    assert tuple(full["path"][0]) == tuple(c["start"]) and tuple(full["path"][full["path_len"] - 1]) == tuple(c["target"])
    assert np.isnan(full["path"][full["path_len"]:]).all()
    cut = solve_case(c, max_path=2)
    assert cut["status"] == R.TRUNCATED and cut["path_len"] == full["path_len"] and cut["path"].tobytes() == full["path"][:2].tobytes()
    assert solve_case(c, max_path=0)["status"] == R.TRUNCATED and solve_case(c, max_path=full["path_len"])["status"] == R.FOUND
    # radius mode: exactly max_degree neighbours is fine, one more is OVERFLOW -- never a thinner roadmap
    r = fixture_case(_by_name("wall_with_one_gap_radius"))
    rfull = spec_case(_by_name("wall_with_one_gap_radius"))
    top = max(len(R.neighbours(rfull["nodes"], i, 0, r["radius"])) for i in range(len(rfull["nodes"])))
    at = solve_case(r, max_degree=top)
    assert at["status"] == rfull["status"] and at["edge_ij"].tobytes() == rfull["edge_ij"].tobytes()
    over = solve_case(r, max_degree=top - 1)
    assert (over["status"], over["n_edges"], over["path_len"], over["sweeps"]) == (R.OVERFLOW, 0, 0, 0) and over["dist"] is None
    assert over["nodes"].tobytes() == rfull["nodes"].tobytes() and np.isnan(over["path"]).all()
    nan, inf = float("nan"), float("inf")
    b = [float(v) for v in c["boundary"]]
    for change in (dict(start=[nan, 1.0]), dict(target=[1.0, inf]), dict(boundary=[0.0, 2e150, 0.0, 5.0]), dict(boundary=[0.0, nan, 0.0, 5.0]),
                   dict(boundary=[b[1], b[0], b[2], b[3]]), dict(boundary=[b[0], b[1], b[3], b[3]]), dict(start=[b[0] - 1e-6, 1.0]),
                   dict(target=[1.0, b[3] + 1e-6])):
        bad = solve_case(dict(c, **change))
        assert (bad["status"], bad["path_len"], bad["n_edges"], bad["sweeps"], len(bad["nodes"])) == (R.INVALID, 0, 0, 0, 0), change
    assert solve_case(dict(c, start=[b[0] - 5e-10, 1.0]))["status"] != R.INVALID   # (the closed boundary grown by 1e-9)
    assert solve_case(c, hw=(0, 4))["status"] == R.INVALID and solve_case(c, hw=(c["grid"].size, 2))["status"] == R.INVALID
    # coincident nodes (build-defined: the smaller index is the nearer): start == target is an edge of cost 0 and a path of two points
    same = solve_case(dict(c, target=c["start"]))
    assert same["status"] == R.FOUND and same["path_len"] == 2 and same["dist"][1] == 0.0 and tuple(same["edge_ij"][0]) == (0, 1)
    # an edge of cost 0 into a LOWER index: node 1 gets its value from node 5, which coincides with it and was settled a sweep
    # earlier.  The predecessor at equal g goes by the sweep, not by the index, so the walk from node 1 still ends at node 0
    ij, cost = np.array([(0, 5), (1, 5), (2, 5)], np.int32), np.array([1.0, 0.0, 0.0])
    g, sweeps, settled = R.fixed_point(6, ij, cost)
    assert g.tolist() == [0.0, 1.0, 1.0, np.inf, np.inf, 1.0] and sweeps == 3 and settled.tolist() == [0, 2, 2, 0, 0, 1]
    assert R.predecessors(g, ij, cost, settled).tolist() == [-1, 5, 5, -1, -1, 0]
    # every sample is a function of the seed and its index alone; the dead guard: every one of n_samples iterations appends
    a, b2 = solve_case(c, n_samples=20), solve_case(c, n_samples=50)
    assert a["nodes"].tobytes() == b2["nodes"][:22].tobytes() and len(b2["nodes"]) == 52
    import sample_plan_ref
    assert b2["nodes"][5, 0] == b[0] + (b[1] - b[0]) * sample_plan_ref.draw_at(c["seed"], 6)


def test_the_workspace_layout_of_the_specification_is_the_headers():
    from tactics2d_amd import _ffi, build
    build.build()
    lib = _ffi.lib()
    for n_samples, k in ((1, 1), (1, 16), (62, 10), (254, 3), (1000, 10), (1022, 16), (30, 32), (30, 1024), (1022, 1024)):
        n, e, o_nodes, o_dist, o_cost, o_ij, o_scratch, row = R.row_layout(n_samples, k)
        assert lib.t2d_prm_plan_workspace_bytes(3, n_samples, k) == 3 * row and row % 256 == 0
        assert (o_nodes, o_dist, o_cost, o_ij, o_scratch) == (0, 16 * n, 24 * n, 24 * n + 8 * e, 24 * n + 16 * e) and o_scratch + 4 * e <= row
        assert e == n * min(k, n - 1)
    for bad in ((-1, 10, 10), (1, 0, 10), (1, 1023, 10), (1, 10, 0)):
        assert lib.t2d_prm_plan_workspace_bytes(*bad) == -1
    assert lib.t2d_prm_plan_workspace_bytes(0, 10, 10) == 0


# ---- the Python interface before any device call -------------------------------------------------------------------------------------
def test_plan_refuses_what_the_reference_refuses_with_its_messages_before_any_device_call():
    from tactics2d_amd import search
    grid = np.ones((5, 5))
    args = ([1.0, 1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], grid)
    with pytest.raises(TypeError, match="collide_fn must be None or"):
        search.PRM.plan(*args, lambda a, b, o: False)
    with pytest.raises(TypeError, match="callback must be None"):
        search.PRM.plan(*args, None, callback=lambda state: None)
    with pytest.raises(TypeError):
        search.PRM.plan(*args, search.grid_collide, 1000, 10, None, 100000, print)
    with pytest.raises(ValueError):
        search.PRM.plan(*args[:3], np.ones(5))
    with pytest.raises(ValueError):
        search.PRM.plan([1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], grid)
    for kw, message in ((dict(boundary=[5.0, 0.0, 0.0, 5.0]), "Invalid boundary: [5. 0. 0. 5.]. Must satisfy x_min < x_max and y_min < y_max"),
                        (dict(boundary=[0.0, 5.0, 2.0, 2.0]), "Must satisfy x_min < x_max and y_min < y_max"),
                        (dict(start=[-1.0, 1.0]), "start x-coordinate -1.0 is outside boundary x-range [0.0, 5.0]"),
                        (dict(start=[1.0, 6.0]), "start y-coordinate 6.0 is outside boundary y-range [0.0, 5.0]"),
                        (dict(target=[5.5, 1.0]), "target x-coordinate 5.5 is outside boundary x-range [0.0, 5.0]"),
                        (dict(target=[1.0, -0.5]), "target y-coordinate -0.5 is outside boundary y-range [0.0, 5.0]"),
                        (dict(n_samples=0), "n_samples must be positive, got 0"),
                        (dict(k_nearest=0), "k_nearest must be positive, got 0"),
                        (dict(connection_radius=0.0), "connection_radius must be positive, got 0.0"),
                        (dict(connection_radius=-2.0), "connection_radius must be positive, got -2.0"),
                        (dict(max_iter=0), "max_iter must be positive, got 0")):
        call = dict(start=args[0], target=args[1], boundary=args[2], obstacles=grid)
        call.update(kw)
        with pytest.raises(ValueError) as ei:
            search.PRM.plan(**call)
        assert message in str(ei.value), (kw, str(ei.value))
    # the caps of the device are ValueErrors too
    with pytest.raises(ValueError, match="PRM_MAX_NODES"):
        search.PRM.plan(*args, None, 1023)
    with pytest.raises(ValueError, match="k_nearest"):
        search.PRM.plan(*args, None, 100, 17)
    sig = inspect.signature(search.PRM.plan)
    assert list(sig.parameters) == ["start", "target", "boundary", "obstacles", "collide_fn", "n_samples", "k_nearest", "connection_radius",
                                    "max_iter", "callback", "seed", "device_id"]
    assert [sig.parameters[p].default for p in ("collide_fn", "n_samples", "k_nearest", "connection_radius", "max_iter", "callback", "seed")] == \
        [None, 1000, 10, None, 100000, None, None]
    sig = inspect.signature(search.prm_plan_batch)
    assert list(sig.parameters) == ["starts", "targets", "boundaries", "weight_grids", "seeds", "hw", "n_samples", "k_nearest",
                                    "connection_radius", "max_degree", "cell_size", "origin", "max_path", "device_id", "stream"]
    assert [sig.parameters[p].default for p in ("n_samples", "k_nearest", "connection_radius", "max_degree", "max_path")] == [1000, 10, None, 32, 256]
    assert search.PRM.plan_batch is search.prm_plan_batch


def test_prm_plan_batch_refuses_bad_arguments_before_any_device_call():
    from tactics2d_amd import search
    z2, z4, w = np.zeros((2, 2)), np.zeros((2, 4)), np.ones((2, 4, 4))
    for kw in (dict(n_samples=0), dict(n_samples=1023), dict(k_nearest=0), dict(k_nearest=17), dict(connection_radius=0.0),
               dict(connection_radius=-1.0), dict(connection_radius=float("nan")), dict(connection_radius=1.0, max_degree=0),
               dict(cell_size=0.0), dict(cell_size=float("nan")), dict(origin=(0.0, float("inf"))), dict(max_path=-1)):
        with pytest.raises(ValueError):
            search.prm_plan_batch(z2, z2, z4, w, 1, **kw)
    for call in (lambda: search.prm_plan_batch(np.zeros((3, 2)), z2, z4, w, 1), lambda: search.prm_plan_batch(z2, np.zeros((2, 3)), z4, w, 1),
                 lambda: search.prm_plan_batch(z2, z2, z4, w, [1, 2, 3]), lambda: search.prm_plan_batch(z2, z2, z4, np.ones((2, 0, 4)), 1),
                 lambda: search.prm_plan_batch(z2, z2, z4, np.ones(4), 1)):
        with pytest.raises(ValueError):
            call()
    doc = search.__doc__
    assert "PRM.plan" in doc and "A*" in doc and "D*" in doc and "MCTS" in doc and "remain out" in doc


def test_the_seed_none_takes_one_draw_of_numpys_global_stream(monkeypatch):
    from tactics2d_amd import search
    seen = []

    def fake_batch(starts, targets, boundaries, grids, seeds, *a, **kw):
        seen.append(int(seeds[0]))
        raise KeyError("stop here")
    monkeypatch.setattr(search, "prm_plan_batch", fake_batch)
    args = ([1.0, 1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], np.ones((5, 5)))
    np.random.seed(11)
    with pytest.raises(KeyError):
        search.PRM.plan(*args)
    after = np.random.uniform()
    np.random.seed(11)
    want = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))
    assert after == np.random.uniform() and seen[-1] == want   # (ONE draw was taken, the one the other planners take)
    with pytest.raises(KeyError):
        search.PRM.plan(*args, seed=2 ** 64 - 3)
    assert seen[-1] == 2 ** 64 - 3


# ---- header <-> _ffi <-> layout, and the entry point's refusals ----------------------------------------------------------------------
def test_header_ffi_and_layout_agree():
    from tactics2d_amd import _ffi, build, layout as L, search
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for name in ("PRM_FOUND", "PRM_NO_PATH", "PRM_TRUNCATED", "PRM_OVERFLOW", "PRM_INVALID", "PRM_MAX_NODES", "PRM_MAX_K"):
        assert vals["T2D_" + name] == getattr(L, name) == getattr(search, name), name
    assert (R.FOUND, R.NO_PATH, R.TRUNCATED, R.OVERFLOW, R.INVALID) == (L.PRM_FOUND, L.PRM_NO_PATH, L.PRM_TRUNCATED, L.PRM_OVERFLOW, L.PRM_INVALID)
    assert (R.MAX_NODES, R.MAX_K) == (L.PRM_MAX_NODES, L.PRM_MAX_K) == (1024, 16)
    assert vals["T2D_ABI_VERSION"] == L.ABI_VERSION   # additions only
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
    for name in ("t2d_prm_plan", "t2d_prm_plan_workspace_bytes"):
        res, params = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)", text).groups()
        want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params.split(",")]
        assert _ffi.SYMBOLS[name] == (ctype[res], want), name
    dev = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_prm_dev.h")).read()
    assert re.search(r"kPrmMaxNodes = (\d+)", dev).group(1) == str(L.PRM_MAX_NODES)
    assert re.search(r"kPrmMaxK = (\d+)", dev).group(1) == str(L.PRM_MAX_K)
    assert "t2d_prm.hip" in build.SOURCES and "t2d_prm_dev.h" in build.HEADERS
    # the LDS of a query: x, y and two planes of g, 32 bytes per node, and two words per node: three queries in one CU's 160 KiB
    assert 3 * (32 + 8) * L.PRM_MAX_NODES + 3 * 64 <= 160 * 1024


def test_the_entry_point_refuses_bad_scalars_pointers_and_a_small_workspace_without_a_launch():
    """the checks come before the first HIP call and read no pointer, so they can be seen without a device"""
    from tactics2d_amd import _ffi, build
    build.build()
    lib = _ffi.lib()
    p = 4096   # (an aligned non-null address nothing reads)
    need = lib.t2d_prm_plan_workspace_bytes(3, 100, 10)
    need_r = lib.t2d_prm_plan_workspace_bytes(3, 100, 32)

    def call(n=3, cells=16, n_samples=100, k=10, radius=0.0, degree=32, cell=1.0, ox=0.0, oy=0.0, max_path=8, ws=p, ws_bytes=need, weight=p,
             path=p, status=p, start=p, seed=p, sweeps=p):
        return lib.t2d_prm_plan(0, n, weight, p, cells, start, p, p, seed, n_samples, k, radius, degree, cell, ox, oy, max_path, ws, ws_bytes,
                                path, p, status, p, sweeps, None)

    for bad in (dict(n=-1), dict(cells=0), dict(max_path=-1), dict(n_samples=0), dict(n_samples=1023), dict(k=0), dict(k=17),
                dict(radius=-0.5), dict(radius=float("nan")), dict(radius=float("inf")), dict(radius=1.0, degree=0, ws_bytes=need_r),
                dict(cell=0.0), dict(cell=float("nan")), dict(ox=float("inf")), dict(oy=float("nan")), dict(ws=None), dict(ws=p + 8),
                dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(radius=1.0, ws_bytes=need_r - 1), dict(weight=None), dict(weight=p + 4),
                dict(path=None), dict(status=p + 2), dict(start=None), dict(seed=None), dict(seed=p + 4), dict(sweeps=None)):
        assert call(**bad) == _ffi.ERR_INVALID, bad
        assert "t2d_prm_plan" in lib.t2d_last_error(None).decode()
    assert call(ws_bytes=need - 1) == _ffi.ERR_INVALID and str(need) in lib.t2d_last_error(None).decode()
    assert call(n=0, ws_bytes=0) == _ffi.OK
    assert call(n=0, path=None, max_path=0, ws_bytes=0, radius=2.0, k=0) == _ffi.OK   # (radius mode does not read k_nearest)
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {"t2d_prm_plan", "t2d_prm_plan_workspace_bytes"} <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "tactics2d")), reason="the reference tree is not present")
def test_the_fixture_reproduces_byte_for_byte_from_its_script(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_prm.py"), "--ref", REF, "--out", str(tmp_path)], check=True,
                   env=env, capture_output=True)
    with open(tmp_path / "prm.npz", "rb") as a, open(os.path.join(ROOT, "tests", "golden", "prm.npz"), "rb") as b:
        assert a.read() == b.read()
