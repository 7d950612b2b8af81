"""Grid A* without a device: the specification (tests/astar_ref.py, an explicit heap) against the fixture made by running the
reference's own AStar (tests/golden/grid_astar.npz, tests/golden/make_grid_astar.py) with tolerance 0 in every run -- path, plan
array, iterations, closed set, every came_from, g_score bit for bit --; what the fixture has to contain, counted; the host formulas
of the heuristic markers; AStar.plan's refusals with the reference's messages; header <-> _ffi <-> layout <-> search for the new
names; the fixture reproduced byte for byte where the reference tree is present."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import astar_ref as A
import grid_search_ref as R
from test_grid_search import fixture as dijkstra_fixture, fixture_case as dijkstra_case, n_cases as dijkstra_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("TACTICS2D_REFERENCE", "/root/reference")
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "grid_astar.npz")))
        cells = g["grid_hw"][:, 0] * g["grid_hw"][:, 1]
        g["grid_off"] = np.concatenate([[0], np.cumsum(cells)])
        g["table_off"] = np.concatenate([[0], np.cumsum(cells[g["table_grid"]])])
        g["path_off"] = np.concatenate([[0], np.cumsum(g["path_len"])])
        g["state_off"] = np.concatenate([[0], np.cumsum(cells[g["grid_id"]])])
        _CACHE["g"] = g
    return _CACHE["g"]


def n_runs():
    return len(fixture()["grid_id"])


def grid_of(k):
    g = fixture()
    return g["grid"][g["grid_off"][k]:g["grid_off"][k + 1]].reshape(tuple(g["grid_hw"][k]))


def run_inputs(r):
    """the arguments of astar_ref.solve (and of a row of t2d_grid_astar) for run r: dict(weight, source, target, kind, htarget,
    table, scale, connectivity, mult, max_iter).  A run whose heuristic_fn is astar_ref.wavy is a TABLE row: the callable evaluated
    per cell on the host against the run's htarget, as AStar.plan does it."""
    g = fixture()
    k = int(g["grid_id"][r])
    grid = grid_of(k)
    kind, table = int(g["kind"][r]), None
    htarget = (float(g["htarget"][r][0]), float(g["htarget"][r][1]))
    if g["table_id"][r] >= 0:
        t = int(g["table_id"][r])
        table = g["table"][g["table_off"][t]:g["table_off"][t + 1]]
    elif g["fn"][r]:
        w = grid.shape[1]
        kind, table = A.H_TABLE, np.array([A.wavy([v % w, v // w], list(htarget)) for v in range(grid.size)], np.float64)
    return dict(weight=grid, source=int(g["source"][r]), target=int(g["target"][r]), kind=kind, htarget=htarget, table=table,
                scale=float(g["scale"][r]), connectivity=int(g["grid_connectivity"][k]), mult=float(g["grid_mult"][k]),
                max_iter=int(g["max_iter"][r]))


def spec_run(r):
    """the specification's answer to run r with what `also` collects, computed once and shared (read only)"""
    if ("spec", r) not in _CACHE:
        also = {}
        _CACHE["spec", r] = (A.solve(also=also, **run_inputs(r)), also)
    return _CACHE["spec", r]


def recorded(r):
    """what the reference returned for run r: dict(found, cost, path (index path, or plan's int64 array), iteration, closed, g, parent)"""
    g = fixture()
    rec = g["path"][g["path_off"][r]:g["path_off"][r + 1]]
    s = slice(g["state_off"][r], g["state_off"][r + 1])
    return dict(found=int(g["found"][r]), cost=float(g["cost"][r]), path=rec[:, 0] if g["mode"][r] == 0 else rec,
                iteration=int(g["iteration"][r]), closed=g["closed"][s], g=g["g_score"][s], parent=g["came_from"][s])


def run_name(r):
    g = fixture()
    return f"run {r}: {g['grid_name'][g['grid_id'][r]]} mode {g['mode'][r]} kind {g['kind'][r]} scale {g['scale'][r]} max_iter {g['max_iter'][r]}"


def base_runs():
    """run index of the euclidean plan_graph run of every grid, in grid order"""
    g = fixture()
    first = {}
    for r in range(n_runs()):
        if g["mode"][r] == 0 and g["kind"][r] == A.H_EUCLIDEAN and g["scale"][r] == 1.0 and g["max_iter"][r] == 100000:
            first.setdefault(int(g["grid_id"][r]), r)
    return [first[k] for k in range(len(g["grid_name"]))]


# ---- the specification against the reference: tolerance 0 -----------------------------------------------------------------------
def test_the_specification_equals_the_reference_in_every_run():
    g = fixture()
    for r in range(n_runs()):
        want, (o, _) = recorded(r), spec_run(r)
        what = run_name(r)
        k = int(g["grid_id"][r])
        assert o["status"] in ((A.FOUND,) if want["found"] else (A.NO_PATH, A.MAX_ITER)), what
        assert o["iterations"] == want["iteration"], what
        assert (o["closed"] == want["closed"]).all() and o["expanded"] == int(want["closed"].sum()), what
        assert (o["parent"] == want["parent"]).all(), what
        assert o["g"].tobytes() == want["g"].tobytes(), what
        path = o["path"][:o["path_len"]]
        if g["mode"][r] == 0:
            assert (path == want["path"]).all() and len(path) == len(want["path"]), what
            assert (o["g"][int(g["target"][r])] == want["cost"]) if want["found"] else np.isinf(want["cost"]), what
        else:
            xy = R.world_path(path, grid_of(k).shape[1], g["grid_boundary"][k], g["grid_resolution"][k]) if want["found"] else \
                np.zeros((0, 2), np.int64)
            assert xy.dtype == want["path"].dtype and xy.shape == want["path"].shape and (xy == want["path"]).all(), what


def test_the_fixture_covers_what_it_should():
    g = fixture()
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "grid_astar.npz")) < 400_000
    hw = g["grid_hw"]
    assert (hw.prod(axis=1) == 4096).sum() == 1 and ((hw[:, 1] > 64) & (hw[:, 0] == 5)).sum() == 2 and hw.min() == 1
    runs = lambda mask: int(np.sum(mask))   # noqa: E731
    assert runs(g["mode"] == 0) >= len(hw) and runs(g["mode"] == 1) >= len(hw)
    for kind in (A.H_ZERO, A.H_MANHATTAN, A.H_OCTILE, A.H_TABLE):
        assert runs(g["kind"] == kind) >= 20, kind
    assert runs(g["scale"] == 2.5) >= 20 and runs(g["fn"] == 1) >= 10
    assert np.isinf(g["table"]).sum() >= 100 and not np.isnan(g["table"]).any()
    off_centre = (g["mode"] == 1) & (np.abs(g["htarget"] - np.round(g["htarget"])).max(axis=1) > 0.1)
    assert runs(off_centre) >= 40
    limited = g["max_iter"] < 100000
    assert runs(limited) >= 30 and {0, 1} <= set(g["max_iter"][limited])
    # a run stopped by max_iter whose value just above finds the path, and one stopped exactly behind a stale pop
    stopped = [r for r in np.flatnonzero(limited) if spec_run(r)[0]["status"] == A.MAX_ITER]
    assert len(stopped) >= 20
    assert any(spec_run(r)[1]["stale_at"] and spec_run(r)[1]["stale_at"][-1] == g["max_iter"][r] - 1 for r in stopped)
    assert sum(spec_run(r)[0]["status"] == A.NO_PATH for r in range(n_runs())) >= 20
    # the grids are make_grid_search.py's, case for case
    d = dijkstra_fixture()
    assert dijkstra_cases() == len(hw) - 3
    for k in range(dijkstra_cases()):
        grid, s, t, conn, mult = dijkstra_case(k)[:5]
        assert grid.tobytes() == grid_of(k).tobytes() and conn == g["grid_connectivity"][k] and mult == g["grid_mult"][k], d["name"][k]
        assert (g["grid_start"][k] == d["start"][k]).all() and (g["grid_goal"][k] == d["goal"][k]).all()


def test_the_counted_preconditions():
    """Why A* is not Dijkstra on these grids, counted over the euclidean plan_graph run of the grids shared with
    tests/golden/grid_search.npz: the numbers are those tests/golden/make_grid_astar.py's fixture holds."""
    g = fixture()
    base = base_runs()[:dijkstra_cases()]
    found = differs = dearer = stale = falling = ties = 0
    for k, r in enumerate(base):
        want, (o, also) = recorded(r), spec_run(r)
        d_path, d_cost = dijkstra_case(k)[5], dijkstra_case(k)[6]
        assert want["found"] == (len(d_path) > 0), run_name(r)
        if want["found"]:
            pops = also["popped"]
            found += 1
            stale += bool(also["stale_at"])
            falling += any(b[0] < a[0] for a, b in zip(pops[:-1], pops[1:]))
            ties += any(a[0] == b[0] and a[1] != b[1] for a, b in zip(pops[:-1], pops[1:]))
            differs += len(want["path"]) != len(d_path) or bool((want["path"] != d_path).any())
            dearer += want["cost"] > d_cost
            assert want["cost"] >= d_cost, run_name(r)
    print(f"found {found}, path differs {differs}, dearer {dearer}, stale pops {stale}, f falls {falling}, ties between cells {ties}")
    assert (found, differs, dearer, stale, falling, ties) == COUNTS


COUNTS = (168, 26, 11, 55, 43, 93)   # of the 208 shared grids: a path; of those: the rest


# ---- the host side ------------------------------------------------------------------------------------------------------------------
def test_the_markers_are_the_formulas_on_the_host():
    from tactics2d_amd import search
    rng = np.random.RandomState(5)
    for _ in range(200):
        a = [int(rng.randint(0, 70)), int(rng.randint(0, 70))]
        b = [float(rng.uniform(-3, 70)), float(rng.uniform(-3, 70))]
        assert search.zero_heuristic(a, b) == 0.0
        assert search.euclidean_heuristic(a, b) == np.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2) == A.heuristic(A.H_EUCLIDEAN, *a, *b)
        assert search.manhattan_heuristic(a, b) == abs(a[0] - b[0]) + abs(a[1] - b[1]) == A.heuristic(A.H_MANHATTAN, *a, *b)
        assert search.octile_heuristic(a, b) == A.heuristic(A.H_OCTILE, *a, *b)
    assert search.octile_heuristic([3, 0], [0.0, 4.0]) == 4.0 + (search.SQRT2 - 1.0) * 3.0


def test_plan_refuses_what_the_reference_refuses_in_its_words():
    from tactics2d_amd.search import AStar, euclidean_heuristic as h
    g = fixture()
    grid = np.ones((4, 5))
    calls = {
        "resolution_zero": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 0, 4], grid, h, 0.0),
        "resolution_negative": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 0, 4], grid, h, -1.0),
        "boundary_x": lambda: AStar.plan([0, 0], [1, 1], [5, 5, 0, 4], grid, h, 1.0),
        "boundary_y": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 4, 0], grid, h, 1.0),
        "start_outside": lambda: AStar.plan([5.5, 0], [1, 1], [0, 5, 0, 4], grid, h, 1.0),
        "start_below": lambda: AStar.plan([0, -0.5], [1, 1], [0, 5, 0, 4], grid, h, 1.0),
        "target_outside": lambda: AStar.plan([0, 0], [1, 4.5], [0, 5, 0, 4], grid, h, 1.0),
        "size_mismatch": lambda: AStar.plan([0, 0], [1, 1], [0, 6, 0, 4], grid, h, 1.0),
        "size_mismatch_resolution": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 0, 4], grid, h, 0.5),
    }
    assert sorted(calls) == sorted(g["refusal_name"])
    for name, message in zip(g["refusal_name"], g["refusal_message"]):
        with pytest.raises(ValueError) as ei:
            calls[str(name)]()
        assert str(ei.value) == str(message), name
    # one cell: the reference's one-point return, before any launch; a callback cannot run in a kernel
    xy = AStar.plan([1.2, 2.1], [0.9, 1.8], [0, 5, 0, 4], grid, h, 1.0)
    assert xy.shape == (1, 2) and xy.tolist() == [[1.2, 2.1]]
    with pytest.raises(TypeError):
        AStar.plan([0, 0], [3, 3], [0, 5, 0, 4], grid, h, 1.0, callback=print)
    assert AStar.plan_graph(7, 7, grid, h) == ([7], 0.0)
    for bad in (-1, 20):
        with pytest.raises(ValueError):
            AStar.plan_graph(bad, 3, grid, h)


def test_the_header_ffi_layout_and_package_agree():
    from tactics2d_amd import _ffi, layout as L, search
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    define = lambda name: int(re.search(rf"#define\s+{name}\s+(\d+)", header).group(1))   # noqa: E731
    assert define("T2D_GRID_MAX_ITER") == L.GRID_MAX_ITER == search.MAX_ITER == A.MAX_ITER
    assert L.GRID_MAX_ITER not in (L.GRID_FOUND, L.GRID_NO_PATH, L.GRID_TRUNCATED, L.GRID_INVALID, L.GRID_FIELD_ONLY)
    for name, spec in (("ZERO", A.H_ZERO), ("EUCLIDEAN", A.H_EUCLIDEAN), ("MANHATTAN", A.H_MANHATTAN), ("OCTILE", A.H_OCTILE),
                       ("TABLE", A.H_TABLE)):
        assert define("T2D_ASTAR_H_" + name) == getattr(L, "ASTAR_H_" + name) == spec
    assert (A.FOUND, A.NO_PATH, A.TRUNCATED, A.INVALID) == (L.GRID_FOUND, L.GRID_NO_PATH, L.GRID_TRUNCATED, L.GRID_INVALID)
    for symbol in ("t2d_grid_astar", "t2d_grid_astar_workspace_bytes"):
        assert symbol in _ffi.SYMBOLS and re.search(rf"\b{symbol}\(", header), symbol
    decl = re.search(r"int t2d_grid_astar\((.*?)\);", header, re.S).group(1)
    assert len(decl.split(",")) == len(_ffi.SYMBOLS["t2d_grid_astar"][1]) == 30
    assert _ffi.SYMBOLS["t2d_grid_astar_workspace_bytes"] == (C.c_int64, [C.c_int32] * 3)
    assert search.AStar.plan_batch is search.astar_plan_batch or search.AStar.plan_batch == search.astar_plan_batch
    for name in ("AStar", "AStarPaths", "astar_plan_batch", "euclidean_heuristic", "manhattan_heuristic", "octile_heuristic", "zero_heuristic"):
        assert hasattr(search, name), name
    assert "t2d_astar.hip" in __import__("tactics2d_amd.build", fromlist=["SOURCES"]).SOURCES


def test_the_library_exports_the_entry_points_and_sizes_the_workspace():
    """no device needed: the workspace has room for `connectivity` entries per cell -- the exact bound, so there is no overflow"""
    from tactics2d_amd import _ffi, layout as L
    lib = _ffi.lib()
    for n, cells, conn in ((1, 1, 4), (3, 100, 8), (4096, L.GRID_MAX_CELLS, 8)):
        need = lib.t2d_grid_astar_workspace_bytes(n, cells, conn)
        assert need % n == 0 and need // n >= cells * (8 * conn + 8 + 8 + 4) and need // n % 256 == 0
    for bad in ((-1, 10, 4), (1, 0, 4), (1, 10, 6), (1, L.GRID_MAX_CELLS + 1, 8)):
        assert lib.t2d_grid_astar_workspace_bytes(*bad) == -1


@pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "tactics2d")), reason="the reference tree is not present")
def test_the_fixture_reproduces_byte_for_byte_from_its_script(tmp_path):
    env = dict(os.environ, PYTHONDONTWRITEBYTECODE="1")
    subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "make_grid_astar.py"), "--ref", REF, "--out", str(tmp_path)],
                   check=True, env=env, capture_output=True)
    with open(tmp_path / "grid_astar.npz", "rb") as a, open(os.path.join(ROOT, "tests", "golden", "grid_astar.npz"), "rb") as b:
        assert a.read() == b.read()
