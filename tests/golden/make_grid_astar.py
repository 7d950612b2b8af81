#!/usr/bin/env python3
"""Golden data for the grid A* -> grid_astar.npz, made by RUNNING the reference's own AStar.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
tactics2d/search/a_star.py, tactics2d/search/graph_utils.py and tactics2d/map/generator/generate_grid_map.py from their FILES,
unmodified (they need numpy and scipy only), and for every run calls grid_to_csr and AStar.plan_graph or AStar.plan with a callback
that keeps the LAST state it is handed.  The grids are those of make_grid_search.py, case for case (grid k here is case k there),
then one 64 x 64 serpentine (the cell cap) and two 5 x 65 grids (wider than a wave).

grid_astar.npz:
  grids: grid_name [G] str, grid_hw i32 [G, 2], grid_start / grid_goal i32 [G, 2] (row, col), grid_connectivity i32 [G], grid_mult f64 [G],
    grid_boundary f64 [G, 4], grid_resolution f64 [G]; grid f64 [sum H*W] concatenated
  tables (heuristic values per cell, +inf entries among them): table_grid i32 [T]; table f64 [sum H*W of their grids] concatenated
  runs, one row each (R runs): grid_id i32, mode i32 (0: plan_graph, 1: plan), kind i32 (astar_ref.H_*), scale f64, htarget f64 [R, 2]
    (the point the heuristic measures against, in cell units: plan's target_rasterized), table_id i32 (-1: none), fn i32 (1: the run's
    heuristic_fn is astar_ref.wavy, a callable no kind describes), max_iter i32, source / target i32 (cells), start_xy / target_xy
    f64 [R, 2] (plan's world arguments), and what the reference returned: found i32, cost f64 (plan_graph's; NaN for plan),
    path_len i32 (index path, or the rows of plan's array), iteration i32 (the last callback's);
    concatenated in run order: path i64 [sum path_len, 2] (plan's array; for plan_graph the cell index in column 0, -1 in column 1),
    and the last callback's state over the grid's cells: closed u8, g_score f64, came_from i32 (-1: the cell has none)
  refusal_name / refusal_message: the ValueError text of each invalid call of REFUSALS.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_grid_astar.py --ref REFERENCE_TREE [--out DIR]

The file is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import importlib.util
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import astar_ref as A   # noqa: E402  (the kinds' numbers, the arbitrary callable, and -- to CHOOSE max_iter values only -- the specification)
from make_grid_search import PROPORTIONS, RESOLUTIONS, SIZES, SQRT2, hand_made, serpentine, write_npz   # noqa: E402


def load_reference(ref):
    out = []
    for rel, name in (("search/a_star.py", "AStar"), ("search/graph_utils.py", "grid_to_csr"),
                      ("map/generator/generate_grid_map.py", "GridMapGenerator")):
        spec = importlib.util.spec_from_file_location("_ref_" + os.path.basename(rel)[:-3], os.path.join(ref, "tactics2d", rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out.append(getattr(mod, name))
    return out


def euclidean_heuristic(a, b):
    """the reference's tests/test_search.py: euclidean_heuristic, as written there"""
    return np.sqrt((a[0] - b[0]) ** 2 + (a[1] - b[1]) ** 2)


def point_heuristic(kind, scale, mult):
    """heuristic_fn(a, b) for AStar.plan: a = [x, y] of the cell, b the point"""
    if kind == A.H_ZERO:
        return lambda a, b: 0.0
    if kind == A.H_EUCLIDEAN and scale == 1.0:
        return euclidean_heuristic
    if kind == A.H_EUCLIDEAN:
        return lambda a, b: scale * euclidean_heuristic(a, b)
    if kind == A.H_MANHATTAN:
        return lambda a, b: abs(a[0] - b[0]) + abs(a[1] - b[1])
    if kind == A.H_OCTILE:
        return lambda a, b: max(abs(a[0] - b[0]), abs(a[1] - b[1])) + (mult - 1.0) * min(abs(a[0] - b[0]), abs(a[1] - b[1]))
    raise ValueError(kind)


def index_heuristic(fn, width):
    """the same for AStar.plan_graph, whose heuristic_fn takes (cell, target cell)"""
    return lambda i, t: fn([int(i) % width, int(i) // width], [float(int(t) % width), float(int(t) // width)])


def refusals(AStar, grid_to_csr):
    graph = grid_to_csr(np.ones((4, 5)), obstacle_value=np.inf)
    h = euclidean_heuristic
    calls = {
        "resolution_zero": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 0, 4], graph, h, 0.0),
        "resolution_negative": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 0, 4], graph, h, -1.0),
        "boundary_x": lambda: AStar.plan([0, 0], [1, 1], [5, 5, 0, 4], graph, h, 1.0),
        "boundary_y": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 4, 0], graph, h, 1.0),
        "start_outside": lambda: AStar.plan([5.5, 0], [1, 1], [0, 5, 0, 4], graph, h, 1.0),
        "start_below": lambda: AStar.plan([0, -0.5], [1, 1], [0, 5, 0, 4], graph, h, 1.0),
        "target_outside": lambda: AStar.plan([0, 0], [1, 4.5], [0, 5, 0, 4], graph, h, 1.0),
        "size_mismatch": lambda: AStar.plan([0, 0], [1, 1], [0, 6, 0, 4], graph, h, 1.0),
        "size_mismatch_resolution": lambda: AStar.plan([0, 0], [1, 1], [0, 5, 0, 4], graph, h, 0.5),
    }
    names, messages = [], []
    for name, call in calls.items():
        try:
            call()
        except ValueError as exc:
            names.append(name)
            messages.append(str(exc))
        else:
            raise SystemExit(f"the reference accepts {name}")
    return names, messages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    AStar, grid_to_csr, GridMapGenerator = load_reference(args.ref)

    grids = []   # (name, grid, start, goal, connectivity, mult): make_grid_search.py's cases in its order, then the large ones
    seed = 1000
    for size in SIZES:
        for conn in (4, 8):
            for min_cost in (1, 0):
                for prop in PROPORTIONS:
                    if size[0] * size[1] * (1 - prop) < 3:
                        continue
                    seed += 1
                    max_cost = 5 if (seed % 3) else 2
                    grid, start, goal = GridMapGenerator(size, min_cost, max_cost, prop, random_seed=seed).generate()
                    grids.append((f"generated_{size[0]}x{size[1]}_c{conn}_min{min_cost}_p{prop}", grid, start, goal, conn, SQRT2))
    grids += hand_made()
    n_shared = len(grids)
    g, s, t = serpentine(64, 64)
    grids.append(("serpentine_64x64_8", g, s, t, 8, SQRT2))
    rng = np.random.RandomState(20261021)
    for conn in (4, 8):
        g = rng.choice([0.5, 1.0, 2.0, 3.0], size=(5, 65))
        g[rng.rand(5, 65) < 0.2] = np.inf
        g[0, 0] = g[4, 64] = 1.0
        grids.append((f"wider_than_a_wave_5x65_{conn}", g, (0, 0), (4, 64), conn, SQRT2))

    boundaries, graphs = [], []
    for k, (name, grid, start, goal, conn, mult) in enumerate(grids):
        h, w = grid.shape
        res = RESOLUTIONS[k % len(RESOLUTIONS)]
        x_min, y_min = float(k % 5 - 2), float(3 - k % 7)
        boundaries.append(([x_min, x_min + w * res, y_min, y_min + h * res], res))
        graphs.append(grid_to_csr(np.asarray(grid, np.float64), obstacle_value=np.inf, connectivity=conn, diagonal_cost_multiplier=mult))

    tables, table_grid = [], []
    keys = ("grid_id", "mode", "kind", "scale", "htarget", "table_id", "fn", "max_iter", "source", "target", "start_xy", "target_xy",
            "found", "cost", "path_len", "iteration")
    rows = {k: [] for k in keys}
    paths, closeds, gs, parents = [], [], [], []

    def run(k, mode, kind=A.H_EUCLIDEAN, scale=1.0, table_id=-1, fn=0, max_iter=100000, off_start=(0.0, 0.0), off_target=(0.0, 0.0)):
        name, grid, start, goal, conn, mult = grids[k]
        h, w = grid.shape
        n = h * w
        (boundary, res), graph = boundaries[k], graphs[k]
        s_idx, t_idx = int(start[0] * w + start[1]), int(goal[0] * w + goal[1])
        inside = lambda cell, off: cell + (off if cell > 0 else abs(off))   # noqa: E731  (row or column 0: not below the boundary)
        start_xy = [inside(start[1], off_start[0]) * res + boundary[0], inside(start[0], off_start[1]) * res + boundary[2]]
        target_xy = [inside(goal[1], off_target[0]) * res + boundary[0], inside(goal[0], off_target[1]) * res + boundary[2]]
        last = {}

        def keep(state):
            last.clear()
            last.update(state)
        if mode == 0:
            htarget = [float(t_idx % w), float(t_idx // w)]
            if table_id >= 0:
                tab = tables[table_id]
                fn_i = lambda i, t: tab[int(i)]   # noqa: E731
            else:
                fn_i = index_heuristic(point_heuristic(kind, scale, mult), w)
            path, cost = AStar.plan_graph(s_idx, t_idx, graph, fn_i, max_iter, keep)
            found, rec = int(len(path) > 0), np.array([[c, -1] for c in path], np.int64).reshape(-1, 2)
            closed = np.zeros(n, np.uint8)
            closed[last["closed_indices"]] = 1
        else:
            htarget = [(target_xy[0] - boundary[0]) / res, (target_xy[1] - boundary[2]) / res]
            xy = AStar.plan(start_xy, target_xy, boundary, graph, A.wavy if fn else point_heuristic(kind, scale, mult), res, max_iter, keep)
            found, cost = int(xy is not None), float("nan")
            rec = np.zeros((0, 2), np.int64) if xy is None else np.asarray(xy)
            assert rec.dtype == np.int64
            closed = np.asarray(last["closed"], np.uint8)
        came = np.full(n, -1, np.int32)
        for child, par in last["came_from"].items():
            came[int(child)] = int(par)
        for key, val in zip(keys, (k, mode, kind, scale, htarget, table_id, fn, max_iter, s_idx, t_idx, start_xy, target_xy, found, cost,
                                   len(rec), int(last["iteration"]))):
            rows[key].append(val)
        paths.append(rec)
        closeds.append(closed)
        gs.append(np.asarray(last["g_score"], np.float64).copy())
        parents.append(came)
        return found, int(last["iteration"])

    for k in range(len(grids)):
        conn, mult = grids[k][4], grids[k][5]
        run(k, 0)                                  # every case under euclidean, through plan_graph ...
        run(k, 1)                                  # ... and through plan, start and target on cell centres
        if k >= n_shared:
            continue
        if k % 4 == 0:
            run(k, 0, A.H_ZERO)
        if k % 4 == 1:
            run(k, 0, A.H_MANHATTAN)
        if k % 4 == 2:
            run(k, 0, A.H_EUCLIDEAN, 2.5)
        if conn == 8 and k % 3 == 0:
            run(k, 0, A.H_OCTILE)
        if k % 5 == 0:                             # a table: the euclidean values with +inf entries among them
            h, w = grids[k][1].shape
            t_idx = int(grids[k][3][0] * w + grids[k][3][1])
            tab = np.array([euclidean_heuristic([v % w, v // w], [float(t_idx % w), float(t_idx // w)]) for v in range(h * w)])
            tab[(np.arange(h * w) * 7) % 11 == 3] = np.inf
            tables.append(tab)
            table_grid.append(k)
            run(k, 0, A.H_TABLE, table_id=len(tables) - 1)
        if k % 6 == 0:                             # off the cell centres: target_rasterized is no cell
            run(k, 1, off_start=(0.3, -0.2), off_target=(-0.4, 0.45))
        if k % 6 == 3:
            run(k, 1, A.H_MANHATTAN, off_start=(-0.45, 0.1), off_target=(0.25, -0.3))
        if k % 10 == 3:                            # a callable no kind describes
            run(k, 1, fn=1, off_target=(0.2, 0.2))

    # max_iter: 0, 1, around a stale pop, around the final iteration -- of the first cases that have stale pops
    chosen = 0
    for k in range(n_shared):
        name, grid, start, goal, conn, mult = grids[k]
        w = grid.shape[1]
        also = {}
        o = A.solve(grid, int(start[0] * w + start[1]), int(goal[0] * w + goal[1]), connectivity=conn, mult=mult, also=also)
        if not also.get("stale_at") or o["status"] != A.FOUND:
            continue
        stale = also["stale_at"][0]
        for m in sorted({0, 1, stale, stale + 1, o["iterations"], o["iterations"] + 1}):
            run(k, chosen % 2, max_iter=m)
        chosen += 1
        if chosen == 6:
            break
    assert chosen == 6

    arrays = {k: np.asarray(v, np.float64 if k in ("scale", "htarget", "cost", "start_xy", "target_xy") else np.int32) for k, v in rows.items()}
    arrays.update(path=np.concatenate(paths), closed=np.concatenate(closeds), g_score=np.concatenate(gs), came_from=np.concatenate(parents))
    arrays.update(grid_name=np.asarray([c[0] for c in grids]), grid_hw=np.int32([c[1].shape for c in grids]),
                  grid_start=np.int32([c[2] for c in grids]), grid_goal=np.int32([c[3] for c in grids]),
                  grid_connectivity=np.int32([c[4] for c in grids]), grid_mult=np.float64([c[5] for c in grids]),
                  grid_boundary=np.float64([b[0] for b in boundaries]), grid_resolution=np.float64([b[1] for b in boundaries]),
                  grid=np.concatenate([np.asarray(c[1], np.float64).reshape(-1) for c in grids]),
                  table_grid=np.int32(table_grid), table=np.concatenate(tables))
    names, messages = refusals(AStar, grid_to_csr)
    arrays.update(refusal_name=np.asarray(names), refusal_message=np.asarray(messages))
    out = os.path.join(args.out, "grid_astar.npz")
    write_npz(out, arrays)
    print(f"{len(grids)} grids, {len(rows['grid_id'])} runs ({int(np.sum(rows['found']))} with a path), {os.path.getsize(out)} bytes")


if __name__ == "__main__":
    main()
