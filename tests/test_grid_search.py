"""Grid shortest paths without a device: the specification (tests/grid_search_ref.py: relax to the fixed point, then one
predecessor rule) against the fixture made by running the reference's own Dijkstra (tests/golden/grid_search.npz,
tests/golden/make_grid_search.py) -- cost BIT FOR BIT and the path cell for cell in every case, the ones with zero-weight edges
included (the reference walks graph[i].nonzero(), so such an edge is none; the specification says the same) --; the host
GridMapGenerator against the recorded grids, starts and goals; Dijkstra.plan's refusals with the reference's messages; header
<-> _ffi <-> layout for the new constants and the symbol; and the cap's refusal, which needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import grid_search_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CACHE = {}


def fixture():
    if "g" not in _CACHE:
        g = dict(np.load(os.path.join(ROOT, "tests", "golden", "grid_search.npz")))
        g["grid_off"] = np.concatenate([[0], np.cumsum(g["hw"][:, 0] * g["hw"][:, 1])])
        g["index_off"] = np.concatenate([[0], np.cumsum(g["index_len"])])
        g["plan_off"] = np.concatenate([[0], np.cumsum(g["plan_len"])])
        _CACHE["g"] = g
    return _CACHE["g"]


def fixture_case(k):
    """(grid [H, W], source, target, connectivity, mult, index path, cost, plan array or None, boundary, resolution) of case k"""
    g = fixture()
    h, w = (int(v) for v in g["hw"][k])
    grid = g["grid"][g["grid_off"][k]:g["grid_off"][k + 1]].reshape(h, w)
    plan = g["plan_path"][g["plan_off"][k]:g["plan_off"][k + 1]] if g["plan_len"][k] else None
    return (grid, int(g["start"][k][0] * w + g["start"][k][1]), int(g["goal"][k][0] * w + g["goal"][k][1]), int(g["connectivity"][k]),
            float(g["mult"][k]), g["index_path"][g["index_off"][k]:g["index_off"][k + 1]], float(g["cost"][k]), plan,
            [float(v) for v in g["boundary"][k]], float(g["resolution"][k]))


def spec_case(k):
    """the specification's answer to fixture case k, computed once and shared (read only)"""
    if ("spec", k) not in _CACHE:
        grid, s, t, conn, mult = fixture_case(k)[:5]
        _CACHE["spec", k] = R.solve(grid, s, t, conn, mult)
    return _CACHE["spec", k]


def n_cases():
    return len(fixture()["name"])


def has_zero_edge(grid, conn, mult):
    w = np.where(np.isnan(grid), np.inf, grid)
    return any((((w + R._shift(w, dr, dc, np.inf)) / 2.0) * (mult if k >= 4 else 1.0) == 0.0).any()
               for k, (dr, dc) in enumerate(R.ORTHOGONAL + (R.DIAGONAL if conn == 8 else ())))


# ---- the fixture itself ------------------------------------------------------------------------------------------------------------
def test_the_fixture_covers_what_it_should():
    g = fixture()
    assert n_cases() >= 200
    hw = g["hw"]
    assert hw.min() == 1 and hw.max() == 24 and (hw[:, 0] != hw[:, 1]).any() and (hw[:, 1] < 64).all()
    assert set(g["connectivity"]) == {4, 8} and {0, 1} <= set(g["min_cost"][g["generated"] == 1])
    assert set(np.round(g["obstacle_proportion"][g["generated"] == 1], 2)) == {0.1, 0.3, 0.45}
    assert (g["index_len"] == 0).sum() >= 10 and (g["index_len"] == 2).any()          # no path; source next to target
    assert np.isinf(g["cost"][g["index_len"] == 0]).all() and (g["plan_len"] == g["index_len"]).all()
    cells = hw[:, 0] * hw[:, 1]
    assert ((g["index_len"] * 2 >= cells - hw[:, 1]) & (cells > 256)).any()          # a serpentine: about half the cells
    zero = [has_zero_edge(*(fixture_case(k)[i] for i in (0, 3, 4))) for k in range(n_cases())]
    assert 20 <= sum(zero) < n_cases() // 2
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "grid_search.npz")) < 200_000


# ---- the specification against the reference ---------------------------------------------------------------------------------------
def test_the_field_at_the_target_is_the_reference_cost_bit_for_bit():
    for k in range(n_cases()):
        t, cost = fixture_case(k)[2], fixture_case(k)[6]
        o = spec_case(k)
        assert o["g"][t] == cost, (fixture()["name"][k], o["g"][t], cost)
        assert o["status"] == (R.FOUND if np.isfinite(cost) else R.NO_PATH), fixture()["name"][k]


def test_the_path_is_the_reference_path_where_every_weight_is_positive():
    """the claim of DESIGN.md 4.21: the heap of (g, index) tuples closes nodes in lexicographic order, and the strict < keeps the
    first of them that explains g[v]"""
    checked = 0
    for k in range(n_cases()):
        grid, s, t, conn, mult, want = fixture_case(k)[:6]
        if has_zero_edge(grid, conn, mult):
            continue
        o = spec_case(k)
        assert o["path_len"] == len(want) and (o["path"][:len(want)] == want).all(), fixture()["name"][k]
        checked += 1
    assert checked > 100


def test_with_zero_weight_edges_the_path_is_a_chain_of_the_same_cost_and_here_the_reference_path():
    checked = 0
    for k in range(n_cases()):
        grid, s, t, conn, mult, want, cost = fixture_case(k)[:7]
        if not has_zero_edge(grid, conn, mult):
            continue
        o = spec_case(k)
        path = o["path"][:o["path_len"]]
        if len(want):
            assert path[0] == s and path[-1] == t
            assert R.fold_cost(grid, path, conn, mult) == o["g"][t] == cost, fixture()["name"][k]
        # an edge of weight 0 is none in the reference either, so its path is pinned here too
        assert len(path) == len(want) and (path == want).all(), fixture()["name"][k]
        checked += 1
    assert checked >= 20


def test_world_coordinates_are_the_reference_array():
    for k in range(n_cases()):
        grid, s, t, conn, mult, want, cost, plan, boundary, res = fixture_case(k)
        if plan is None:
            continue
        got = R.world_path(want, grid.shape[1], boundary, res)
        assert got.dtype == plan.dtype and (got == plan).all(), fixture()["name"][k]


def test_truncation_field_only_and_invalid_rows_of_the_specification():
    g = fixture()
    k = int(np.argmax(g["index_len"]))
    grid, s, t, conn, mult, want = fixture_case(k)[:6]
    full = spec_case(k)
    o = R.solve(grid, s, t, conn, mult, max_path=7)
    assert o["status"] == R.TRUNCATED and o["path_len"] == len(want) and (o["path"] == want[:7]).all() and (o["g"] == full["g"]).all()
    o = R.solve(grid, s, -1, conn, mult, max_path=4)
    assert o["status"] == R.FIELD_ONLY and o["path_len"] == 0 and (o["path"] == -1).all() and (o["g"] == full["g"]).all()
    neg = grid.copy()
    neg[0, 1] = -1.0
    wall = np.flatnonzero(np.isinf(grid.reshape(-1)))[0]
    for bad in (R.solve(grid, -1, t, conn, mult), R.solve(grid, s, grid.size, conn, mult), R.solve(grid, s, -2, conn, mult),
                R.solve(neg, s, t, conn, mult), R.solve(grid, wall, t, conn, mult), R.solve(grid, s, wall, conn, mult)):
        assert bad["status"] == R.INVALID and np.isinf(bad["g"]).all() and bad["path_len"] == 0 and bad["sweeps"] == 0
    one = R.solve(grid, s, s, conn, mult)
    assert one["status"] == R.FOUND and one["path_len"] == 1 and one["path"][0] == s


# ---- the host generator ------------------------------------------------------------------------------------------------------------
def test_the_host_generator_draws_the_reference_grids_starts_and_goals():
    from tactics2d_amd.generator import GridMapGenerator
    g = fixture()
    state = np.random.get_state()
    try:
        for k in np.flatnonzero(g["generated"] == 1):
            grid, start, goal = GridMapGenerator(tuple(int(v) for v in g["hw"][k]), int(g["min_cost"][k]), int(g["max_cost"][k]),
                                                 float(g["obstacle_proportion"][k]), random_seed=int(g["seed"][k])).generate()
            assert grid.dtype == np.float64 and grid.tobytes() == fixture_case(k)[0].tobytes(), g["name"][k]
            assert tuple(start) == tuple(g["start"][k]) and tuple(goal) == tuple(g["goal"][k]), g["name"][k]
        # a batch is consecutive generate() calls on the same stream
        gen = GridMapGenerator((6, 9), 1, 5, 0.3, random_seed=5)
        singles = [gen.generate() for _ in range(3)]
        grids, starts, goals = GridMapGenerator((6, 9), 1, 5, 0.3, random_seed=5).generate_batch(3)
        assert grids.shape == (3, 6, 9) and starts.shape == goals.shape == (3, 2) and starts.dtype == np.int32
        for e, (gr, st, go) in enumerate(singles):
            assert (grids[e] == gr).all() and tuple(starts[e]) == st and tuple(goals[e]) == go
    finally:
        np.random.set_state(state)


# ---- Dijkstra.plan's host side -----------------------------------------------------------------------------------------------------
def _refusal_calls():
    from tactics2d_amd.search import Dijkstra
    grid = np.ones((4, 5))
    return {
        "resolution_zero": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 0, 4], grid, 0.0),
        "resolution_negative": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 0, 4], grid, -1.0),
        "boundary_x": lambda: Dijkstra.plan([0, 0], [1, 1], [5, 5, 0, 4], grid, 1.0),
        "boundary_y": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 4, 0], grid, 1.0),
        "start_outside": lambda: Dijkstra.plan([5.5, 0], [1, 1], [0, 5, 0, 4], grid, 1.0),
        "start_below": lambda: Dijkstra.plan([0, -0.5], [1, 1], [0, 5, 0, 4], grid, 1.0),
        "target_outside": lambda: Dijkstra.plan([0, 0], [1, 4.5], [0, 5, 0, 4], grid, 1.0),
        "size_mismatch": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 6, 0, 4], grid, 1.0),
        "size_mismatch_resolution": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 0, 4], grid, 0.5),
    }


def test_plan_refuses_with_the_reference_messages():
    g = fixture()
    calls = _refusal_calls()
    assert sorted(calls) == sorted(g["refusal_name"])
    for name, message in zip(g["refusal_name"], g["refusal_message"]):
        with pytest.raises(ValueError) as ei:
            calls[str(name)]()
        assert str(ei.value) == str(message), name


def test_plan_returns_the_start_point_when_both_ends_share_a_cell_without_a_device():
    from tactics2d_amd.search import Dijkstra
    out = Dijkstra.plan([1.2, 0.9], [0.8, 1.1], [0, 5, 0, 4], np.ones((4, 5)), 1.0)
    assert out.shape == (1, 2) and out.tolist() == [[1.2, 0.9]]


def test_plan_batch_refuses_bad_arguments_before_any_device_call():
    from tactics2d_amd import search
    for call in (lambda: search.plan_batch(np.ones((2, 3, 3)), [0, 0], connectivity=6),
                 lambda: search.plan_batch(np.ones((2, 3, 3)), [0, 0], connectivity=8, diagonal_cost_multiplier=-1.0),
                 lambda: search.plan_batch(np.ones((2, 3, 3)), [0, 0], diagonal_cost_multiplier=float("nan")),
                 lambda: search.plan_batch(np.ones(5), [0]),
                 lambda: search.plan_batch(np.ones((2, 3, 3)), [0, 0], [1, 1], max_path=-1)):
        with pytest.raises(ValueError):
            call()


# ---- header <-> _ffi <-> layout, and the cap -----------------------------------------------------------------------------------------
def test_header_ffi_and_layout_agree():
    from tactics2d_amd import _ffi, layout as L, search
    header = open(os.path.join(ROOT, "include", "t2d.h")).read()
    vals = {k: int(v) for k, v in re.findall(r"#define\s+(T2D_\w+)\s+(\d+)u?\b", header)}
    for name in ("GRID_FOUND", "GRID_NO_PATH", "GRID_TRUNCATED", "GRID_INVALID", "GRID_FIELD_ONLY", "GRID_MAX_CELLS"):
        assert vals["T2D_" + name] == getattr(L, name), name
    assert (R.FOUND, R.NO_PATH, R.TRUNCATED, R.INVALID, R.FIELD_ONLY) == (L.GRID_FOUND, L.GRID_NO_PATH, L.GRID_TRUNCATED, L.GRID_INVALID,
                                                                          L.GRID_FIELD_ONLY)
    assert (search.FOUND, search.FIELD_ONLY, search.MAX_CELLS) == (L.GRID_FOUND, L.GRID_FIELD_ONLY, L.GRID_MAX_CELLS)
    # two fp64 planes of the cap are what two workgroups per CU leave each of them (160 KiB per CU)
    assert 2 * (2 * 8 * L.GRID_MAX_CELLS) <= 160 * 1024
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    ctype = {"int32_t": C.c_int32, "double": C.c_double}
    params = re.search(r"\bint\s+t2d_grid_dijkstra\s*\(([^)]*)\)", text).group(1).split(",")
    want = [C.c_void_p if "*" in p else ctype[p.split()[0]] for p in params]
    assert _ffi.SYMBOLS["t2d_grid_dijkstra"] == (C.c_int, want)
    dev = open(os.path.join(ROOT, "tactics2d_amd", "csrc", "t2d_gridsearch_dev.h")).read()
    assert re.search(r"kGridMaxCells = (\d+)", dev).group(1) == str(L.GRID_MAX_CELLS)
    from tactics2d_amd import build
    assert "t2d_gridsearch.hip" in build.SOURCES and "t2d_gridsearch_dev.h" in build.HEADERS


def test_the_entry_point_refuses_a_grid_over_the_cap_and_bad_scalars_without_a_launch():
    """the checks come before the first HIP call and read no pointer, so they can be seen without a device"""
    from tactics2d_amd import _ffi, build, layout as L
    build.build()
    lib = _ffi.lib()
    p = 4096   # (an aligned non-null address nothing reads)
    call = lambda n=1, cells=L.GRID_MAX_CELLS + 1, conn=4, mult=1.5, max_path=8, g=p: lib.t2d_grid_dijkstra(
        0, n, p, p, p, p, cells, conn, mult, max_path, g, p, p, p, p, None)
    assert call() == _ffi.ERR_GEOMETRY
    message = lib.t2d_last_error(None).decode()
    assert str(L.GRID_MAX_CELLS) in message and "T2D_GRID_MAX_CELLS" in message and str(L.GRID_MAX_CELLS + 1) in message
    with pytest.raises(_ffi.GeometryError):
        _ffi.check(call(), None, lib)
    for bad in (dict(n=-1), dict(cells=0), dict(conn=6), dict(mult=-0.5), dict(mult=float("inf")), dict(max_path=-1), dict(g=None),
                dict(g=p + 4)):
        assert call(**{"cells": 16, **bad}) == _ffi.ERR_INVALID, bad
    assert call(n=0, cells=L.GRID_MAX_CELLS) == _ffi.OK
