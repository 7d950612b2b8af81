"""Hybrid A* without a device: the specification (tests/hybrid_astar_ref.py: the reference's loop with the device's sincos, the
cost grid as depths, the collision test over the cells near the segment) against the fixture made by running the reference's own
HybridAStar.plan with its tests' grid collision checker (tests/golden/hybrid_astar.npz, tests/golden/make_hybrid_astar.py): the
status of every case, and where the decisions are the same (length, pops, nodes) every state to 1e-9; the cases whose decisions
differ are counted against a cap of 2 % (0 today); the specification's own invariants; HybridAStar.plan's argument handling;
header <-> _ffi <-> layout; and the entry point's refusals, which need no device."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import hybrid_astar_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}
# what every fixture case is run with, here and on the device (the fixture's longest path has 51 states, its largest search
# 21571 nodes and 1577 open entries)
MAX_PATH, MAX_NODES = 64, 24576


def fixture():
    if "g" not in _CACHE:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "hybrid_astar.npz")))
        g["grid_off"] = np.concatenate([[0], np.cumsum(g["hw"][:, 0] * g["hw"][:, 1])])
        g["path_off"] = np.concatenate([[0], np.cumsum(g["path_len"])])
        _CACHE["g"] = g
    return _CACHE["g"]


def n_cases():
    return len(fixture()["name"])


def fixture_case(k):
    """dict(grid [H, W], start, target, boundary, step_size, steering, wheelbase, max_iter, path [len, 3], status) of case k"""
    g = fixture()
    h, w = (int(v) for v in g["hw"][k])
    path = g["path"][g["path_off"][k]:g["path_off"][k + 1]]
    status = R.FOUND if len(path) else (R.NO_PATH if g["exhausted"][k] else R.MAX_ITER)
    return dict(grid=g["grid"][g["grid_off"][k]:g["grid_off"][k + 1]].reshape(h, w), start=g["start"][k], target=g["target"][k],
                boundary=g["boundary"][k], step_size=float(g["step_size"][k]), steering=[float(v) for v in g["steering"][k][:g["n_steer"][k]]],
                wheelbase=float(g["wheelbase"][k]), max_iter=int(g["max_iter"][k]), path=path, status=status)


def case_deltas(c):
    return R.steer_deltas(c["steering"], c["wheelbase"], c["step_size"])


def spec_case(k):
    """the specification's answer to fixture case k, computed once and shared (read only)"""
    if ("spec", k) not in _CACHE:
        c = fixture_case(k)
        _CACHE["spec", k] = R.solve(c["grid"], c["start"], c["target"], c["boundary"], case_deltas(c), c["step_size"], max_iter=c["max_iter"],
                                    max_nodes=MAX_NODES, max_path=MAX_PATH)
    return _CACHE["spec", k]


# ---- the fixture itself ------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    g = fixture()
    none = g["path_len"] == 0
    assert (g["path_len"] >= 3).sum() >= 150 and (none & (g["exhausted"] == 1)).sum() >= 100 and (none & (g["exhausted"] == 0)).sum() >= 10
    assert (g["open_peak"] > 64).sum() >= 5 and (g["open_peak"] > 256).sum() >= 2 and (g["nodes"] > 4096).sum() >= 2
    gen = g["generated"] == 1
    assert {tuple(v) for v in g["hw"][gen]} == {(3, 3), (3, 7), (7, 3), (1, 9), (5, 5), (8, 8), (6, 13), (11, 17), (16, 16), (24, 24)}
    assert set(np.round(g["obstacle_proportion"][gen], 2)) == {0.0, 0.1, 0.2, 0.3}
    assert set(g["step_size"][gen]) == {1.0, 0.5} and set(g["n_steer"][gen]) == {1, 3, 5}
    off = np.round(g["start"][gen, 2] - g["target"][gen, 2], 6)
    assert set(off) == {0.0, 0.4, -0.7}
    assert gen.sum() == 10 * 4 * 3 * 2 * 3
    names = set(g["name"][~gen])
    for name in ("goal_behind_start", "corridor_step1.0", "target_heading_two_pi_away", "two_primitives_one_cell_step1.0",
                 "boundary_cells_not_the_grid", "touches_a_corner_diagonally", "corridor_max_iter_3"):
        assert name in names, name
    # what the shared run parameters must hold
    assert g["path_len"].max() <= MAX_PATH and g["nodes"].max() <= MAX_NODES and g["open_peak"].max() <= R.MAX_OPEN
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "hybrid_astar.npz")) < 400_000


def test_the_findings_the_fixture_records():
    g = fixture()
    k = {str(n): i for i, n in enumerate(g["name"])}
    # a target heading 2 pi away from a reachable one is never reached: the goal test takes the heading as it is
    assert g["path_len"][k["target_heading_reachable"]] >= 3 and g["path_len"][k["target_heading_two_pi_away"]] == 0
    # the returned headings are not reduced to [0, 2 pi): this path keeps its start's -pi
    neg = fixture_case(k["negative_headings"])["path"]
    assert len(neg) >= 3 and (neg[:, 2] < 0).all()
    # the start is never collision-checked: a search from inside an obstacle square starts (and ends, every segment colliding)
    assert g["pops"][k["start_inside_an_obstacle"]] >= 1
    # max_iter stops a search that would succeed
    assert g["path_len"][k["corridor_step1.0"]] >= 3 and g["path_len"][k["corridor_max_iter_3"]] == 0 and g["pops"][k["corridor_max_iter_3"]] == 3


# ---- the specification against the reference ---------------------------------------------------------------------------------------
def test_the_specification_equals_the_reference_on_the_fixture():
    g = fixture()
    differing, worst = [], 0.0
    for k in range(n_cases()):
        c, o = fixture_case(k), spec_case(k)
        assert o["status"] == c["status"], (g["name"][k], o["status"], c["status"])
        same = o["path_len"] == len(c["path"]) and o["iterations"] == g["pops"][k] and o["nodes"] == g["nodes"][k]
        if not same:
            differing.append(str(g["name"][k]))
            continue
        assert o["open_peak"] == g["open_peak"][k], g["name"][k]
        if len(c["path"]):
            err = float(np.abs(o["path"][:len(c["path"])] - c["path"]).max())
            worst = max(worst, err)
            assert err <= 1e-9, (g["name"][k], err)
        assert np.isnan(o["path"][o["path_len"]:]).all()
    print(f"cases whose decisions differ from the reference's: {len(differing)} of {n_cases()} {differing}; worst state error {worst:.3g}")
    assert len(differing) <= 0.02 * n_cases()


# ---- the specification's own invariants --------------------------------------------------------------------------------------------
def _picks():
    g = fixture()
    return [k for k in range(n_cases()) if g["generated"][k] == 0 or k % 7 == 0]


def test_the_depth_grid_prunes_what_the_cost_grid_prunes_and_appends_in_the_order_of_the_primitives():
    """check_costs keeps the reference's fp64 cost grid beside the depths and asserts every prune decision equal; `record` shows
    the kept primitives of every expansion in increasing order, and a node's index is its place in that order"""
    g = fixture()
    dropped_by_a_sibling = 0
    for k in _picks():
        c, rec = fixture_case(k), []
        o = R.solve(c["grid"], c["start"], c["target"], c["boundary"], case_deltas(c), c["step_size"], max_iter=c["max_iter"],
                    max_nodes=MAX_NODES, max_path=MAX_PATH, check_costs=True, record=rec)
        want = spec_case(k)
        assert (o["status"], o["path_len"], o["iterations"], o["nodes"]) == (want["status"], want["path_len"], want["iterations"], want["nodes"])
        assert o["nodes"] == 1 + sum(len(kept) for _, kept in rec)
        assert all(kept == sorted(kept) and len(set(kept)) == len(kept) for _, kept in rec)
        if str(g["name"][k]).startswith("two_primitives_one_cell"):
            # from the start all primitives are free and new; the ones that share a cell with an earlier one are dropped
            first = rec[0][1]
            assert first[0] == 0 and len(first) < len(c["steering"])
            dropped_by_a_sibling += 1
    assert dropped_by_a_sibling >= 3


def test_g_is_a_strictly_increasing_function_of_the_depth():
    """the proof obligation of the 16-bit cost grid: g(d) = fl(g(d - 1) + step_size) grows at every depth the grid can hold, for every
    step_size the entry point admits -- so new_g >= cost[cell] is new_depth >= depth[cell]"""
    for step in (1e-150, 1e150, 1.0, 0.5, 0.1, 1.0 / 3.0, 4.9e-3, 7.3e11):
        g = 0.0
        for _ in range(R.EMPTY):
            nxt = g + step
            assert nxt > g and math.isfinite(nxt)
            g = nxt


def test_the_near_cells_give_the_full_loops_answer():
    rng = np.random.RandomState(11)
    checked = hits = 0
    for h, w, cs, origin in ((7, 9, 1.0, (0.0, 0.0)), (5, 5, 0.5, (1.0, -2.0)), (6, 4, 2.0, (-3.0, 0.5))):
        obst = rng.rand(h, w) < 0.3
        for _ in range(400):
            x1 = origin[0] + rng.uniform(-2, w + 1) * cs
            y1 = origin[1] + rng.uniform(-2, h + 1) * cs
            ang, length = rng.uniform(0, 2 * math.pi), rng.choice([0.5, 1.0, 3.0]) * cs
            x2, y2 = x1 + math.cos(ang) * length, y1 + math.sin(ang) * length
            if rng.rand() < 0.2:
                y2 = y1   # the degenerate branch
            if rng.rand() < 0.2:
                x1, x2 = round(x1 / cs * 2) * cs / 2, round(x1 / cs * 2) * cs / 2   # on an edge or a centre line
            near = R.collides(obst, x1, y1, x2, y2, cs, origin)
            assert near == R.collides(obst, x1, y1, x2, y2, cs, origin, everywhere=True)
            checked += 1
            hits += near
    assert 100 < hits < checked - 100


def test_overflow_truncated_and_invalid_rows_of_the_specification():
    g = fixture()
    k = int(np.argmax(g["path_len"]))
    c, full = fixture_case(k), spec_case(k)
    run = lambda **kw: R.solve(c["grid"], kw.pop("start", c["start"]), kw.pop("target", c["target"]), kw.pop("boundary", c["boundary"]),
                               kw.pop("deltas", case_deltas(c)), c["step_size"], max_iter=c["max_iter"],
                               **{"max_nodes": MAX_NODES, "max_path": MAX_PATH, **kw})
    o = run(max_path=5)
    assert o["status"] == R.TRUNCATED and o["path_len"] == full["path_len"] and (o["path"] == full["path"][:5]).all()
    o = run(max_nodes=full["nodes"])
    assert o["status"] == R.FOUND and o["path"].tobytes() == full["path"].tobytes()
    for kw in (dict(max_nodes=full["nodes"] // 2), dict(max_open=full["open_peak"] - 1), dict(max_nodes=1)):
        o = run(**kw)
        assert o["status"] == R.OVERFLOW and o["path_len"] == 0 and np.isnan(o["path"]).all() and 0 < o["iterations"] <= full["iterations"]
        assert o["nodes"] <= kw.get("max_nodes", MAX_NODES)
    x_min, x_max, y_min, y_max = c["boundary"]
    nan, inf = float("nan"), float("inf")
    for kw in (dict(start=[nan, 1, 0]), dict(start=[1, 1, inf]), dict(target=[1, -inf, 0]), dict(target=[1, 1, 2e9]), dict(start=[3e150, 1, 0]),
               dict(boundary=[x_max, x_min, y_min, y_max]), dict(boundary=[x_min, x_max, y_min, y_min]), dict(boundary=[x_min, nan, y_min, y_max]),
               dict(deltas=[0.0, nan]), dict(deltas=[0.0, 3e9]), dict(start=[x_min - 1.0, y_min, 0]), dict(start=[x_min, y_max + 1.0, 0]),
               dict(hw=(0, 4)), dict(hw=(c["grid"].shape[0] + 1, c["grid"].shape[1])), dict(hw=(-1, -1))):
        o = run(**kw)
        assert o["status"] == R.INVALID and o["path_len"] == o["iterations"] == o["nodes"] == 0 and np.isnan(o["path"]).all(), kw
    # a start just below x_min truncates to cell 0, as in the reference: not invalid
    assert run(start=[x_min - 0.1 * c["step_size"], y_min, 0.0])["status"] != R.INVALID
    # a cost grid above the cap: no search
    o = run(boundary=[0.0, 200.0, 0.0, 200.0])
    assert o["status"] == R.OVERFLOW and o["iterations"] == 0


# ---- HybridAStar.plan's host side --------------------------------------------------------------------------------------------------
def test_plan_refuses_another_collision_function_and_bad_arguments_before_any_device_call():
    from tactics2d_amd import search
    grid = np.ones((5, 5))
    with pytest.raises(TypeError) as ei:
        search.HybridAStar.plan([0, 0, 0], [3, 3, 0], [0, 5, 0, 5], grid, lambda p1, p2, obstacles: False)
    assert "grid_collide" in str(ei.value) and "device" in str(ei.value)
    with pytest.raises(ValueError):
        search.HybridAStar.plan([0, 0, 0], [3, 3, 0], [0, 5, 0, 5], np.ones(5), search.grid_collide)
    for kw in (dict(step_size=0.0), dict(step_size=-1.0), dict(step_size=float("nan")), dict(steering_angles=()),
               dict(steering_angles=[0.0] * 17), dict(wheelbase=0.0)):
        with pytest.raises(ValueError):
            search.HybridAStar.plan([0, 0, 0], [3, 3, 0], [0, 5, 0, 5], grid, None, **kw)
    for call in (lambda: search.HybridAStar.plan_batch(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 4)), np.ones(5)),
                 lambda: search.HybridAStar.plan_batch(np.zeros((3, 3)), np.zeros((2, 3)), np.zeros((2, 4)), np.ones((2, 4, 4))),
                 lambda: search.HybridAStar.plan_batch(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 4)), np.ones((2, 4, 4)), cell_size=0.0),
                 lambda: search.HybridAStar.plan_batch(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 4)), np.ones((2, 4, 4)), origin=(0.0, math.inf)),
                 lambda: search.HybridAStar.plan_batch(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 4)), np.ones((2, 4, 4)), max_nodes=0),
                 lambda: search.HybridAStar.plan_batch(np.zeros((2, 3)), np.zeros((2, 3)), np.zeros((2, 4)), np.ones((2, 4, 4)), max_path=-1)):
        with pytest.raises(ValueError):
            call()


def test_the_marker_is_the_reference_checker_over_the_grid():
    from tactics2d_amd import search
    rng = np.random.RandomState(5)
    grid = rng.randint(1, 6, size=(6, 8)).astype(float)
    grid[rng.rand(6, 8) < 0.25] = np.inf
    grid[1, 1] = np.nan
    obst = R.obstacle_mask(grid)
    seen = 0
    for _ in range(300):
        p1, p2 = rng.uniform(-1, 8, 2), rng.uniform(-1, 8, 2)
        got = search.grid_collide(list(p1), list(p2), grid)
        assert got == R.collides(obst, p1[0], p1[1], p2[0], p2[1], everywhere=True)
        seen += got
    assert 30 < seen < 270
    assert search.steer_deltas([-0.5, 0, 0.5], 2.5, 0.5) == R.steer_deltas([-0.5, 0, 0.5], 2.5, 0.5)


# ---- header <-> _ffi <-> layout, and the entry point's refusals ----------------------------------------------------------------------
def test_header_ffi_and_layout_agree():
    from tactics2d_amd import _ffi, build, layout as L, search
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for name in ("HYBRID_FOUND", "HYBRID_NO_PATH", "HYBRID_MAX_ITER", "HYBRID_TRUNCATED", "HYBRID_OVERFLOW", "HYBRID_INVALID",
                 "HYBRID_MAX_OPEN", "HYBRID_MAX_XY_CELLS", "HYBRID_MAX_STEER"):
        assert vals["T2D_" + name] == getattr(L, name), name
    assert (R.FOUND, R.NO_PATH, R.MAX_ITER, R.TRUNCATED, R.OVERFLOW, R.INVALID) == \
        (L.HYBRID_FOUND, L.HYBRID_NO_PATH, L.HYBRID_MAX_ITER, L.HYBRID_TRUNCATED, L.HYBRID_OVERFLOW, L.HYBRID_INVALID)
    assert (R.MAX_OPEN, R.MAX_XY_CELLS, R.MAX_STEER) == (L.HYBRID_MAX_OPEN, L.HYBRID_MAX_XY_CELLS, L.HYBRID_MAX_STEER)
    assert (search.HYBRID_FOUND, search.HYBRID_OVERFLOW, search.HYBRID_INVALID) == (L.HYBRID_FOUND, L.HYBRID_OVERFLOW, L.HYBRID_INVALID)
    assert vals["T2D_ABI_VERSION"] == L.ABI_VERSION   # additions only
    # six queries' open entries (an fp64 f and a node index each) fit one CU's 160 KiB of LDS
    assert 6 * 12 * L.HYBRID_MAX_OPEN <= 160 * 1024
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "int": C.c_int}
    for name in ("t2d_hybrid_astar", "t2d_hybrid_astar_workspace_bytes"):
        res, params = re.search(r"\b(\w+)\s+" + name + r"\s*\(([^)]*)\)", text).groups()
        want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params.split(",")]
        assert _ffi.SYMBOLS[name] == (ctype[res], want), name
    dev = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_hybrid_dev.h")).read()
    assert re.search(r"kHybridMaxOpen = (\d+)", dev).group(1) == str(L.HYBRID_MAX_OPEN)
    assert re.search(r"kHybridMaxXYCells = (\d+)", dev).group(1) == str(L.HYBRID_MAX_XY_CELLS)
    assert re.search(r"kHybridEmpty = (\d+)", dev).group(1) == str(R.EMPTY)
    assert "t2d_hybrid.hip" in build.SOURCES and "t2d_hybrid_dev.h" in build.HEADERS


def test_the_library_exports_the_two_symbols():
    import subprocess
    from tactics2d_amd import _ffi, build
    build.build()
    out = subprocess.run(["nm", "-D", "--defined-only", _ffi.LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert {"t2d_hybrid_astar", "t2d_hybrid_astar_workspace_bytes"} <= names
    assert not [n for n in names if "hybrid" in n and n not in ("t2d_hybrid_astar", "t2d_hybrid_astar_workspace_bytes") and n.startswith("t2d_")]


def test_the_entry_point_refuses_bad_scalars_pointers_and_a_small_workspace_without_a_launch():
    """the checks come before the first HIP call and read no pointer, so they can be seen without a device"""
    from tactics2d_amd import _ffi, build
    build.build()
    lib = _ffi.lib()
    p = 4096   # (an aligned non-null address nothing reads)
    need = lib.t2d_hybrid_astar_workspace_bytes(3, 1000)
    assert need == 3 * lib.t2d_hybrid_astar_workspace_bytes(1, 1000) and need % 256 == 0
    assert lib.t2d_hybrid_astar_workspace_bytes(1, 1000) >= 1000 * 40 + R.MAX_XY_CELLS * R.HEADING_CELLS * 2
    assert lib.t2d_hybrid_astar_workspace_bytes(-1, 10) == -1 and lib.t2d_hybrid_astar_workspace_bytes(1, 0) == -1
    assert lib.t2d_hybrid_astar_workspace_bytes(0, 10) == 0

    def call(n=3, cells=16, n_steer=3, step=1.0, cell=1.0, ox=0.0, oy=0.0, max_iter=100, max_nodes=1000, max_path=8, ws=p, ws_bytes=need,
             weight=p, path=p, status=p, start=p):
        return lib.t2d_hybrid_astar(0, n, weight, p, cells, start, p, p, p, n_steer, step, cell, ox, oy, max_iter, max_nodes, max_path, ws,
                                    ws_bytes, path, p, status, p, p, None)

    for bad in (dict(n=-1), dict(cells=0), dict(max_path=-1), dict(max_nodes=0), dict(n_steer=0), dict(n_steer=17), dict(step=0.0),
                dict(step=-1.0), dict(step=float("nan")), dict(step=float("inf")), dict(cell=0.0), dict(cell=float("nan")),
                dict(ox=float("inf")), dict(oy=float("nan")), dict(ws=None), dict(ws=p + 8), dict(ws_bytes=need - 1), dict(ws_bytes=0),
                dict(weight=None), dict(weight=p + 4), dict(path=None), dict(status=p + 2), dict(start=None)):
        assert call(**bad) == _ffi.ERR_INVALID, bad
        assert "t2d_hybrid_astar" in lib.t2d_last_error(None).decode()
    assert call(ws_bytes=need - 1) == _ffi.ERR_INVALID and str(need) in lib.t2d_last_error(None).decode()
    with pytest.raises(_ffi.T2DError):
        _ffi.check(call(n_steer=17), None, lib)
    assert call(n=0, ws_bytes=0) == _ffi.OK
    assert call(n=0, path=None, max_path=0, ws_bytes=0) == _ffi.OK
