"""The sampling planners without a device: the specification (tests/sample_plan_ref.py: the reference's three loops on the build's
counter stream, hypot as a plain sqrt, the collision test over the cells near the segment) against the fixture made by running the
reference's own RRT.plan, RRTStar.plan and RRTConnect.plan on the same draws (tests/golden/sample_plan.npz,
tests/golden/make_sample_plan.py): the status of every case, and where the decisions are the same (iterations, node counts, every
parent, path length) every coordinate and cost to 1e-9; the cases whose decisions differ are counted against a cap of 2 % (0
today); the findings; the specification's own invariants; the plan methods' argument handling; header <-> _ffi <-> layout; the
entry point's refusals and polyline_routes' argument checks, which need no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import sample_plan_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
# what every fixture case is run with, here and on the device (the fixture's largest tree has 581 nodes)
MAX_PATH, MAX_NODES = 128, 1024
KINDS = ("rrt", "rrt_star", "rrt_connect")


def fixture():
    if "g" not in _CACHE:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "sample_plan.npz")))
        total = g["nodes"].sum(axis=1)
        g["grid_off"] = np.concatenate([[0], np.cumsum(g["hw"][:, 0] * g["hw"][:, 1])])
        g["path_off"] = np.concatenate([[0], np.cumsum(g["path_len"])])
        g["node_off"] = np.concatenate([[0], np.cumsum(total)])
        g["cost_off"] = np.concatenate([[0], np.cumsum(np.where(g["kind"] == R.RRT_STAR, total, 0))])
        _CACHE["g"] = g
    return _CACHE["g"]


def n_cases():
    return len(fixture()["name"])


def fixture_case(k):
    """dict(kind, grid [H, W], start, target, boundary, extension_step, radius, max_iter, seed, path [len, 2], status, iterations,
    nodes (a, b), xy / parent of tree a, xy_b / parent_b of tree b, cost (RRT* only, else None)) of case k"""
    g = fixture()
    h, w = (int(v) for v in g["hw"][k])
    na, nb = (int(v) for v in g["nodes"][k])
    o = int(g["node_off"][k])
    kind = int(g["kind"][k])
    return dict(kind=kind, grid=g["grid"][g["grid_off"][k]:g["grid_off"][k + 1]].reshape(h, w), start=g["start"][k], target=g["target"][k],
                boundary=g["boundary"][k], extension_step=float(g["extension_step"][k]), radius=float(g["radius"][k]),
                max_iter=int(g["max_iter"][k]), seed=int(g["seed"][k]), path=g["path"][g["path_off"][k]:g["path_off"][k + 1]],
                status=R.FOUND if g["found"][k] else R.MAX_ITER, iterations=int(g["iterations"][k]), nodes=(na, nb),
                xy=g["tree_xy"][o:o + na], parent=g["tree_parent"][o:o + na], xy_b=g["tree_xy"][o + na:o + na + nb],
                parent_b=g["tree_parent"][o + na:o + na + nb],
                cost=g["tree_cost"][g["cost_off"][k]:g["cost_off"][k + 1]] if kind == R.RRT_STAR else None)


def solve_case(c, **kw):
    params = dict(max_iter=c["max_iter"], max_nodes=MAX_NODES, max_path=MAX_PATH)
    params.update(kw)
    return R.solve(c["kind"], c["grid"], c["start"], c["target"], c["boundary"], c["seed"], c["extension_step"], c["radius"], **params)


def spec_case(k):
    """the specification's answer to fixture case k, computed once and shared (read only)"""
    if ("spec", k) not in _CACHE:
        rec = {}
        _CACHE["spec", k] = solve_case(fixture_case(k), record=rec)
        _CACHE["rec", k] = rec
    return _CACHE["spec", k]


# ---- the fixture itself ------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    g = fixture()
    kind, found, nodes = g["kind"], g["found"], g["nodes"]
    total = nodes.sum(axis=1)
    for q in range(3):
        assert ((kind == q) & (found == 1)).sum() >= 100 and ((kind == q) & (found == 0)).sum() >= 10, KINDS[q]
    assert (total > 64).sum() >= 5 and (total > 512).sum() >= 2
    # trees that outgrow the part the kernel keeps in LDS (RRT-Connect: half of it per tree)
    assert ((kind != R.RRT_CONNECT) & (nodes[:, 0] > R.LDS_NODES)).sum() + \
        ((kind == R.RRT_CONNECT) & (nodes.max(axis=1) > R.LDS_NODES // 2)).sum() >= 2
    assert (g["changed_parent"] > 0).sum() >= 20 and (g["rewired"] > 0).sum() >= 20
    connect = (kind == R.RRT_CONNECT) & (found == 1)
    assert (connect & (g["iterations"] % 2 == 1)).sum() >= 10 and (connect & (g["iterations"] % 2 == 0)).sum() >= 10
    assert g["max_iter"].max() <= 600 and g["max_iter"][(kind == R.RRT_STAR) & (g["generated"] == 1) & (g["hw"][:, 0] == 16)].max() <= 300
    assert g["path_len"].max() <= MAX_PATH and total.max() <= MAX_NODES
    names = set(str(v) for v in g["name"])
    for hand in ("max_iter_0", "max_iter_1", "target_within_one_step", "target_inside_an_obstacle", "corridor_one_cell_wide",
                 "step_larger_than_the_map", "boundary_smaller_than_the_grid", "boundary_wider_than_the_grid",
                 "touches_a_corner_diagonally", "runs_along_an_edge", "nan_is_an_obstacle"):
        assert all(f"{hand}_{q}" in names for q in KINDS), hand
    sizes = set((int(a), int(b)) for a, b in g["hw"][g["generated"] == 1])
    assert sizes == {(3, 3), (3, 7), (7, 3), (1, 9), (5, 5), (8, 8), (6, 13), (16, 16)}
    assert set(g["obstacle_proportion"][g["generated"] == 1]) == {0.0, 0.1, 0.2, 0.3} and set(g["extension_step"][g["generated"] == 1]) == {1.0, 0.5, 0.7}
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "sample_plan.npz")) < 1 << 20


def _by_name(name):
    g = fixture()
    return int(np.flatnonzero(g["name"] == name)[0])


def test_the_findings_the_fixture_records():
    g = fixture()
    # RRT and RRT* return the walk to the LAST node appended when max_iter runs out, never []
    stopped = np.flatnonzero((g["kind"] != R.RRT_CONNECT) & (g["found"] == 0))
    assert len(stopped) >= 20
    for k in stopped:
        c = fixture_case(k)
        assert len(c["path"]) >= 1 and tuple(c["path"][0]) == tuple(c["start"]) and tuple(c["path"][-1]) == tuple(c["xy"][-1]), g["name"][k]
    for q in ("rrt", "rrt_star"):
        c = fixture_case(_by_name("max_iter_0_" + q))
        assert c["path"].tolist() == [list(c["start"])] and c["nodes"] == (1, 0) and c["iterations"] == 0
    # RRT-Connect returns []
    stopped = np.flatnonzero((g["kind"] == R.RRT_CONNECT) & (g["found"] == 0))
    assert len(stopped) >= 10 and (g["path_len"][stopped] == 0).all()
    # a target inside an obstacle square is never connected; a touch of a corner or an edge is a collision, a pass beside is none
    for hand in ("target_inside_an_obstacle", "touches_a_corner_diagonally", "runs_along_an_edge"):
        assert all(g["found"][_by_name(f"{hand}_{q}")] == 0 for q in KINDS), hand
    assert all(g["found"][_by_name(f"passes_beside_the_square_{q}")] == 1 for q in KINDS)
    # the trees of RRT and RRT* have the same coordinates for the same draws (cases that share the grid differ in their seeds, so
    # this is asked of the specification: the same seed for both kinds)
    seen = 0
    for k in np.flatnonzero((g["kind"] == R.RRT) & (g["nodes"][:, 0] > 30))[:12]:
        c = fixture_case(k)
        a, b = solve_case(c), solve_case(dict(c, kind=R.RRT_STAR))
        assert a["xy"].tobytes() == b["xy"].tobytes() and a["iterations"] == b["iterations"], g["name"][k]
        seen += not np.array_equal(a["parent"], b["parent"])
    assert seen >= 6
    # stale costs: in some RRT* tree a node's cost is not its parent's cost plus the edge
    stale = 0
    for k in np.flatnonzero((g["kind"] == R.RRT_STAR) & (g["rewired"] > 0)):
        c = fixture_case(k)
        p = c["parent"]
        child = np.flatnonzero(p >= 0)
        edge = np.sqrt(((c["xy"][child] - c["xy"][p[child]]) ** 2).sum(axis=1))
        stale += bool((np.abs(c["cost"][p[child]] + edge - c["cost"][child]) > 1e-9).any())
        assert (c["cost"][child] > c["cost"][p[child]]).all(), g["name"][k]   # (strictly decreasing towards the root: no cycle)
    assert stale >= 10


def test_the_specification_equals_the_reference_on_the_fixture():
    g = fixture()
    differ, worst = [], 0.0
    for k in range(n_cases()):
        c, s = fixture_case(k), spec_case(k)
        assert s["status"] == c["status"], g["name"][k]
        same = s["iterations"] == c["iterations"] and tuple(s["nodes"]) == c["nodes"] and s["path_len"] == len(c["path"])
        same = same and np.array_equal(s["parent"], c["parent"]) and np.array_equal(s["parent_b"], c["parent_b"])
        if not same:
            differ.append(str(g["name"][k]))
            continue
        dev = max(np.abs(s["xy"] - c["xy"]).max(), np.abs(s["xy_b"] - c["xy_b"]).max() if c["nodes"][1] else 0.0,
                  np.abs(s["path"][:s["path_len"]] - c["path"]).max() if s["path_len"] else 0.0,
                  np.abs(s["cost"] - c["cost"]).max() if c["kind"] == R.RRT_STAR else 0.0)
        assert dev <= 1e-9, (g["name"][k], dev)
        worst = max(worst, dev)
    print(f"specification vs reference: {len(differ)} of {n_cases()} cases differ in a decision {differ}; largest deviation {worst:.3g}")
    assert len(differ) <= 0.02 * n_cases(), differ


def test_the_specifications_counts_are_the_makers():
    g = fixture()
    for k in np.flatnonzero(g["kind"] == R.RRT_STAR):
        spec_case(k)
        assert _CACHE["rec", k]["changed_parent"] == g["changed_parent"][k], g["name"][k]
        assert _CACHE["rec", k]["rewired"] >= g["rewired"][k], g["name"][k]   # (a node rewired twice counts twice here, once there)
    for k in np.flatnonzero((g["kind"] == R.RRT_CONNECT) & (g["found"] == 1)):
        spec_case(k)
        assert _CACHE["rec", k]["connect_side"] == ("a" if g["iterations"][k] % 2 == 1 else "b"), g["name"][k]


# ---- the specification's own invariants --------------------------------------------------------------------------------------------
def test_a_sample_is_a_function_of_the_seed_and_the_iteration_alone():
    s = 0x1234567890ABCDEF
    state, seq = s, []
    for _ in range(6):
        state = (state + R.GAMMA) & R.MASK
        seq.append((R._fin(state) >> 11) * (1.0 / 9007199254740992.0))
    assert [R.draw_at(s, k) for k in range(6)] == seq and all(0.0 <= u < 1.0 for u in seq)
    import trackgen_ref
    assert R.draw_at(s, 3) == trackgen_ref.draw_at(s, 3)
    assert R.row_seeds(5, 3).tolist() == [R._fin((5 + (i + 1) * R.GAMMA) & R.MASK) for i in range(3)]
    # a smaller max_iter gives a prefix of the same search
    c = fixture_case(_by_name("walled_in_target_step0.7_rrt"))
    long_, short = solve_case(c, max_iter=200), solve_case(c, max_iter=80)
    n = short["nodes"][0]
    assert short["iterations"] == 80 and long_["xy"][:n].tobytes() == short["xy"].tobytes()


def test_trees_paths_and_statuses_of_the_specification():
    g = fixture()
    for k in range(0, n_cases(), 7):
        c, s = fixture_case(k), spec_case(k)
        lo = np.array([c["boundary"][0], c["boundary"][2]])
        hi = np.array([c["boundary"][1], c["boundary"][3]])
        for xy, parent in ((s["xy"], s["parent"]), (s["xy_b"], s["parent_b"])):
            if len(xy) == 0:
                continue
            assert parent[0] == -1 and ((parent[1:] >= 0) & (parent[1:] < len(parent))).all()
            if c["kind"] != R.RRT_STAR:
                assert (parent[1:] < np.arange(1, len(parent))).all()
            body = xy[1:-1] if s["status"] == R.FOUND and c["kind"] != R.RRT_CONNECT else xy[1:]
            assert ((body >= lo) & (body <= hi)).all(), g["name"][k]
            step = np.sqrt(((xy[1:] - xy[parent[1:]]) ** 2).sum(axis=1))
            if c["kind"] != R.RRT_STAR:
                assert (step <= c["extension_step"] * (1 + 1e-12)).all()
        path = s["path"][:s["path_len"]]
        assert np.isnan(s["path"][s["path_len"]:]).all()
        if s["status"] == R.FOUND:
            assert tuple(path[0]) == tuple(c["start"]) and tuple(path[-1]) == tuple(c["target"])
            obst = R.obstacle_mask(c["grid"])
            for a, b in zip(path[:-1], path[1:]):
                assert not R.collides(obst, a[0], a[1], b[0], b[1], everywhere=True), g["name"][k]


def test_overflow_truncated_and_invalid_rows_of_the_specification():
    g = fixture()
    k = int(np.flatnonzero((g["kind"] == R.RRT) & (g["found"] == 1) & (g["path_len"] >= 8))[0])
    c, full = fixture_case(k), spec_case(k)
    cut = solve_case(c, max_path=5)
    assert cut["status"] == R.TRUNCATED and cut["path_len"] == full["path_len"] and cut["path"].tobytes() == full["path"][:5].tobytes()
    over = solve_case(c, max_nodes=full["nodes"][0] - 1)   # (the target's append is the one that does not fit)
    assert over["status"] == R.OVERFLOW and over["path_len"] == 0 and np.isnan(over["path"]).all() and over["nodes"] == (full["nodes"][0] - 1, 0)
    assert solve_case(c, max_nodes=full["nodes"][0])["status"] == R.FOUND
    k = int(np.flatnonzero((g["kind"] == R.RRT_CONNECT) & (g["found"] == 1) & (g["nodes"].min(axis=1) >= 4))[0])
    c, full = fixture_case(k), spec_case(k)
    over = solve_case(c, max_nodes=sum(full["nodes"]) - 1)
    assert over["status"] == R.OVERFLOW and sum(over["nodes"]) == sum(full["nodes"]) - 1 and over["path_len"] == 0
    assert solve_case(c, max_nodes=1)["status"] == R.OVERFLOW and solve_case(c, max_nodes=1)["nodes"] == (1, 0)
    # a walk that max_iter stopped is cut like a path and keeps its status
    k = int(np.flatnonzero((g["kind"] == R.RRT) & (g["found"] == 0) & (g["path_len"] >= 8))[0])
    cut = solve_case(fixture_case(k), max_path=3)
    assert cut["status"] == R.MAX_ITER and cut["path_len"] == spec_case(k)["path_len"] > 3
    nan, inf = float("nan"), float("inf")
    for change in (dict(start=[nan, 1.0]), dict(target=[1.0, inf]), dict(boundary=[0.0, 2e150, 0.0, 5.0]), dict(boundary=[0.0, nan, 0.0, 5.0])):
        bad = solve_case(dict(c, **change))
        assert (bad["status"], bad["path_len"], bad["iterations"], bad["nodes"]) == (R.INVALID, 0, 0, (0, 0)), change
    assert R.solve(R.RRT, c["grid"], c["start"], c["target"], c["boundary"], 1, hw=(0, 4))["status"] == R.INVALID
    assert R.solve(R.RRT, c["grid"], c["start"], c["target"], c["boundary"], 1, hw=(c["grid"].size, 2))["status"] == R.INVALID
    # a boundary with min > max is NOT invalid: no new point ever lies in it
    b = c["boundary"]
    for q in range(3):
        out = solve_case(dict(c, kind=q, boundary=[b[1], b[0], b[2], b[3]]), max_iter=30)
        assert out["status"] == R.MAX_ITER and out["iterations"] == 30 and sum(out["nodes"]) == (2 if q == R.RRT_CONNECT else 1)


# ---- the Python interface before any device call -------------------------------------------------------------------------------------
def test_plan_refuses_callbacks_other_collision_functions_and_bad_arguments_before_any_device_call():
    from tactics2d_amd import search
    grid = np.ones((5, 5))
    args = ([1.0, 1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], grid)
    for cls in (search.RRT, search.RRTStar, search.RRTConnect):
        with pytest.raises(TypeError):
            cls.plan(*args, lambda a, b, o: False)
        with pytest.raises(TypeError):
            cls.plan(*args, None, callback=lambda state: None)
        with pytest.raises(TypeError):
            cls.plan(*args, search.grid_collide, 1.0, 100, callback=print) if cls is not search.RRTStar else \
                cls.plan(*args, search.grid_collide, 1.0, 100, 3.0, print)
        with pytest.raises(ValueError):
            cls.plan(*args[:3], np.ones(5))
        with pytest.raises(ValueError):
            cls.plan([1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], grid)
    import inspect
    for cls, names in ((search.RRT, ["start", "target", "boundary", "obstacles", "collide_fn", "extension_step", "max_iter", "callback"]),
                       (search.RRTStar, ["start", "target", "boundary", "obstacles", "collide_fn", "extension_step", "max_iter", "radius",
                                         "callback"]),
                       (search.RRTConnect, ["start", "target", "boundary", "obstacles", "collide_fn", "extension_step", "max_iter",
                                            "callback"])):
        sig = inspect.signature(cls.plan)
        assert list(sig.parameters)[:len(names)] == names and list(sig.parameters)[len(names):] == ["seed", "device_id"]
        assert sig.parameters["extension_step"].default == 1.0 and sig.parameters["max_iter"].default == 100000
    assert inspect.signature(search.RRTStar.plan).parameters["radius"].default == 3.0
    z2, z4 = np.zeros((2, 2)), np.zeros((2, 4))
    for call in (lambda: search.sample_plan_batch("prm", z2, z2, z4, np.ones((2, 4, 4)), 1),
                 lambda: search.sample_plan_batch(7, z2, z2, z4, np.ones((2, 4, 4)), 1),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), 1, extension_step=0.0),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), 1, extension_step=float("nan")),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), 1, cell_size=-1.0),
                 lambda: search.sample_plan_batch("rrt_star", z2, z2, z4, np.ones((2, 4, 4)), 1, radius=-1.0),
                 lambda: search.sample_plan_batch("rrt_star", z2, z2, z4, np.ones((2, 4, 4)), 1, radius=float("nan")),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), 1, origin=(0.0, float("inf"))),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), 1, max_nodes=0),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), 1, max_path=-1),
                 lambda: search.sample_plan_batch("rrt", np.zeros((3, 2)), z2, z4, np.ones((2, 4, 4)), 1),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 4, 4)), [1, 2, 3]),
                 lambda: search.sample_plan_batch("rrt", z2, z2, z4, np.ones((2, 0, 4)), 1)):
        with pytest.raises(ValueError):
            call()
    assert search.row_seeds(5, 4).tolist() == R.row_seeds(5, 4).tolist() and search.stream_mix(12345) == R._fin(12345)
    assert "A*" in search.__doc__ and "remain out" in search.__doc__ and "sampling planners are not part" not in search.__doc__


def test_the_seed_none_takes_one_draw_of_numpys_global_stream(monkeypatch):
    from tactics2d_amd import search
    seen = []

    def fake_batch(kind, starts, targets, boundaries, grids, seeds, *a, **kw):
        seen.append(int(seeds[0]))
        raise KeyError("stop here")
    monkeypatch.setattr(search, "sample_plan_batch", fake_batch)
    args = ([1.0, 1.0], [3.0, 3.0], [0.0, 5.0, 0.0, 5.0], np.ones((5, 5)))
    for cls in (search.RRT, search.RRTStar, search.RRTConnect):
        np.random.seed(11)
        with pytest.raises(KeyError):
            cls.plan(*args)
        after = np.random.uniform()
        np.random.seed(11)
        with pytest.raises(KeyError):
            cls.plan(*args)
        np.random.seed(11)
        np.random.randint(0, 2 ** 63 - 1, dtype=np.int64)
        assert after == np.random.uniform()   # (ONE draw was taken)
        np.random.seed(12)
        with pytest.raises(KeyError):
            cls.plan(*args)
        with pytest.raises(KeyError):
            cls.plan(*args, seed=2 ** 64 - 3)
        assert seen[-4] == seen[-3] != seen[-2] and seen[-1] == 2 ** 64 - 3
    assert seen[0] == seen[4] == seen[8]   # (the same draw whatever the planner)


# ---- header <-> _ffi <-> layout, and the entry points' refusals ----------------------------------------------------------------------
def test_header_ffi_and_layout_agree():
    from tactics2d_amd import _ffi, build, layout as L, search
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for name in ("SAMPLE_RRT", "SAMPLE_RRT_STAR", "SAMPLE_RRT_CONNECT", "SAMPLE_FOUND", "SAMPLE_MAX_ITER", "SAMPLE_TRUNCATED",
                 "SAMPLE_OVERFLOW", "SAMPLE_INVALID", "SAMPLE_LDS_NODES"):
        assert vals["T2D_" + name] == getattr(L, name), name
    assert (R.RRT, R.RRT_STAR, R.RRT_CONNECT) == (L.SAMPLE_RRT, L.SAMPLE_RRT_STAR, L.SAMPLE_RRT_CONNECT)
    assert (R.FOUND, R.MAX_ITER, R.TRUNCATED, R.OVERFLOW, R.INVALID) == \
        (L.SAMPLE_FOUND, L.SAMPLE_MAX_ITER, L.SAMPLE_TRUNCATED, L.SAMPLE_OVERFLOW, L.SAMPLE_INVALID)
    assert R.LDS_NODES == L.SAMPLE_LDS_NODES and (search.SAMPLE_FOUND, search.SAMPLE_INVALID) == (L.SAMPLE_FOUND, L.SAMPLE_INVALID)
    assert vals["T2D_ABI_VERSION"] == L.ABI_VERSION   # additions only
    assert int(re.search(r"enum \{ T2D_PROFILE_POLYLINE_ROUTES = (\d+) \}", header).group(1)) == L.PROFILE_POLYLINE_ROUTES \
        == L.PROFILE_PLANVIEW_ROUTES + 1
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
    for name in ("t2d_sample_plan", "t2d_sample_plan_workspace_bytes", "t2d_polyline_routes"):
        res, params = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)", text).groups()
        want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params.split(",")]
        assert _ffi.SYMBOLS[name] == (ctype[res], want), name
    dev = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_sample_dev.h")).read()
    assert re.search(r"kSampleLdsNodes = (\d+)", dev).group(1) == str(L.SAMPLE_LDS_NODES)
    assert "t2d_sample.hip" in build.SOURCES and "t2d_sample_dev.h" in build.HEADERS
    # the LDS part of a query: 16 bytes per node, twenty queries in one CU's 160 KiB
    assert 20 * 16 * L.SAMPLE_LDS_NODES <= 160 * 1024


def test_the_entry_point_refuses_bad_scalars_pointers_and_a_small_workspace_without_a_launch():
    """the checks come before the first HIP call and read no pointer, so they can be seen without a device"""
    from tactics2d_amd import _ffi, build, layout as L
    build.build()
    lib = _ffi.lib()
    p = 4096   # (an aligned non-null address nothing reads)
    need = lib.t2d_sample_plan_workspace_bytes(3, 1000)
    assert need == 3 * lib.t2d_sample_plan_workspace_bytes(1, 1000) and need % 256 == 0
    assert 1000 * L.SAMPLE_NODE_BYTES <= lib.t2d_sample_plan_workspace_bytes(1, 1000) < 1000 * L.SAMPLE_NODE_BYTES + 256
    assert lib.t2d_sample_plan_workspace_bytes(-1, 10) == -1 and lib.t2d_sample_plan_workspace_bytes(1, 0) == -1
    assert lib.t2d_sample_plan_workspace_bytes(0, 10) == 0

    def call(n=3, kind=0, cells=16, step=1.0, radius=3.0, cell=1.0, ox=0.0, oy=0.0, max_iter=100, max_nodes=1000, max_path=8, ws=p,
             ws_bytes=need, weight=p, path=p, status=p, start=p, seed=p, nodes=p):
        return lib.t2d_sample_plan(0, n, kind, weight, p, cells, start, p, p, seed, step, radius, cell, ox, oy, max_iter, max_nodes, max_path,
                                   ws, ws_bytes, path, p, status, p, nodes, None)

    for bad in (dict(n=-1), dict(kind=3), dict(kind=-1), dict(cells=0), dict(max_path=-1), dict(max_nodes=0), dict(max_iter=-1),
                dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")), dict(radius=-0.5),
                dict(radius=float("nan")), dict(cell=0.0), dict(cell=float("nan")), dict(ox=float("inf")), dict(oy=float("nan")),
                dict(ws=None), dict(ws=p + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0), dict(weight=None), dict(weight=p + 4),
                dict(path=None), dict(status=p + 2), dict(start=None), dict(seed=None), dict(seed=p + 4), dict(nodes=None)):
        assert call(**bad) == _ffi.ERR_INVALID, bad
        assert "t2d_sample_plan" in lib.t2d_last_error(None).decode()
    assert call(ws_bytes=need - 1) == _ffi.ERR_INVALID and str(need) in lib.t2d_last_error(None).decode()
    with pytest.raises(_ffi.T2DError):
        _ffi.check(call(kind=5), None, lib)
    assert call(n=0, ws_bytes=0) == _ffi.OK
    assert call(n=0, path=None, max_path=0, ws_bytes=0, radius=0.0, kind=2) == _ffi.OK
    assert lib.t2d_polyline_routes(None, p, p, 4, 2, 0, p, None) == _ffi.ERR_INVALID


def test_the_library_exports_the_new_symbols():
    import subprocess
    from tactics2d_amd import _ffi, build
    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"t2d_sample_plan", "t2d_sample_plan_workspace_bytes", "t2d_polyline_routes"} <= names


def test_polyline_routes_checks_its_tensors_before_any_device_call():
    import torch
    from tactics2d_amd.pool import ParticipantPool

    class Stub:
        n_env, device_id = 3, 0
    pts, counts = torch.zeros((3, 5, 2), dtype=torch.float64), torch.zeros(3, dtype=torch.int32)
    for bad_pts, bad_counts in ((pts.float(), counts), (pts[:2], counts), (pts[:, :, :1], counts), (pts[:, :0], counts),
                                (torch.zeros((3, 5, 4), dtype=torch.float64)[:, :, :2], counts), (pts.numpy(), counts),
                                (pts.reshape(3, 10), counts), (pts, counts.long()), (pts, counts[:2]), (pts, counts.numpy()),
                                (pts, torch.zeros((3, 1), dtype=torch.int32))):
        with pytest.raises(ValueError):
            ParticipantPool.polyline_routes(Stub(), bad_pts, bad_counts)
