#!/usr/bin/env python3
"""Golden data for the grid shortest paths -> grid_search.npz, made by RUNNING the reference's own Dijkstra.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
tactics2d/search/dijkstra.py, tactics2d/search/graph_utils.py and tactics2d/map/generator/generate_grid_map.py from their FILES,
unmodified (the tactics2d.map package itself needs shapely; the three files need numpy and scipy only), and for every case calls
grid_to_csr, Dijkstra.plan and Dijkstra.plan_graph.

grid_search.npz, one row per case (C cases; the generated ones first, then the hand-made ones):
  name [C] str, hw i32 [C, 2] (height, width), start i32 [C, 2] / goal i32 [C, 2] (row, col), connectivity i32 [C],
  mult f64 [C] (diagonal_cost_multiplier), boundary f64 [C, 4] (x_min, x_max, y_min, y_max), resolution f64 [C],
  generated i32 [C] (1: the grid, start and goal are GridMapGenerator's), seed / min_cost / max_cost i32 [C],
  obstacle_proportion f64 [C] (of the generated cases),
  cost f64 [C] = plan_graph's cost (inf: no path), index_len i32 [C] = the length of plan_graph's index path (0: none),
  plan_len i32 [C] = the rows of Dijkstra.plan's array (0: None);
  concatenated in case order: grid f64 [sum H*W], index_path i32 [sum index_len], plan_path i64 [sum plan_len, 2].
  refusal_name / refusal_message: the ValueError text of each invalid call of REFUSALS.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_grid_search.py --ref REFERENCE_TREE [--out DIR]

The file is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import importlib.util
import io
import os
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SQRT2 = 1.4142135623730951
# sizes where a kernel can still go wrong: narrower than a wave, H != W, one row, one column, more cells than a workgroup has lanes
SIZES = ((3, 3), (3, 7), (7, 3), (1, 9), (9, 1), (5, 5), (8, 8), (6, 13), (13, 6), (11, 17), (16, 16), (17, 23), (24, 24), (24, 9))
PROPORTIONS = (0.1, 0.3, 0.45)
RESOLUTIONS = (1.0, 0.5, 0.25, 2.0)


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def load_reference(ref):
    out = []
    for rel, name in (("search/dijkstra.py", "Dijkstra"), ("search/graph_utils.py", "grid_to_csr"),
                      ("map/generator/generate_grid_map.py", "GridMapGenerator")):
        spec = importlib.util.spec_from_file_location("_ref_" + os.path.basename(rel)[:-3], os.path.join(ref, "tactics2d", rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out.append(getattr(mod, name))
    return out


def serpentine(h, w):
    """walls on every second row with a gap at alternating ends: one corridor of about h * w / 2 cells"""
    g = np.ones((h, w))
    for r in range(1, h, 2):
        g[r, :] = np.inf
        g[r, w - 1 if (r // 2) % 2 == 0 else 0] = 1.0
    last = h - 1 if h % 2 else h - 2
    return g, (0, 0), (last, w - 1 if (last // 2) % 2 == 0 else 0)


def hand_made():
    """(name, grid, start, goal, connectivity, mult)"""
    rng = np.random.RandomState(20261020)
    cases = []
    for conn in (4, 8):
        cases.append((f"adjacent_{conn}", np.full((4, 5), 2.0), (1, 1), (1, 2), conn, SQRT2))
        cases.append((f"adjacent_diagonal_{conn}", np.full((4, 5), 2.0), (1, 1), (2, 2), conn, SQRT2))
        walled = np.ones((7, 7))
        walled[2, 2:5] = walled[4, 2:5] = walled[2:5, 2] = walled[2:5, 4] = np.inf
        cases.append((f"walled_in_{conn}", walled, (0, 0), (3, 3), conn, SQRT2))
        for h, w in ((24, 24), (9, 5), (8, 6)):
            g, s, t = serpentine(h, w)
            cases.append((f"serpentine_{h}x{w}_{conn}", g, s, t, conn, SQRT2))
        # routes of exactly equal cost, every weight positive: the choice among them is the tie rule
        cases.append((f"uniform_corner_to_corner_{conn}", np.ones((5, 5)), (0, 0), (4, 4), conn, SQRT2))
        cases.append((f"uniform_reverse_{conn}", np.ones((6, 4)), (5, 3), (0, 0), conn, SQRT2))
        cases.append((f"uniform_multiplier_2_{conn}", np.full((5, 6), 3.0), (0, 5), (4, 0), conn, 2.0))
        ring = np.ones((5, 5))
        ring[1:4, 1:4] = np.inf
        cases.append((f"ring_two_ways_{conn}", ring, (0, 2), (4, 2), conn, SQRT2))
        cases.append((f"ring_two_ways_sideways_{conn}", ring.copy(), (2, 0), (2, 4), conn, SQRT2))
        # weights whose sums round differently by order
        for k, (h, w) in enumerate(((9, 11), (12, 7), (6, 6))):
            g = rng.choice([0.1, 0.3, 0.7, 0.2], size=(h, w))
            cases.append((f"decimal_weights_{k}_{conn}", g, (0, 0), (h - 1, w - 1), conn, SQRT2))
        g = rng.choice([0.1, 0.3], size=(10, 10))
        g[rng.rand(10, 10) < 0.2] = np.inf
        g[0, 0] = g[9, 9] = 0.1
        cases.append((f"decimal_weights_obstacles_{conn}", g, (0, 0), (9, 9), conn, SQRT2))
        cases.append((f"one_row_{conn}", rng.randint(1, 6, size=(1, 12)).astype(float), (0, 11), (0, 0), conn, SQRT2))
        cases.append((f"one_column_{conn}", rng.randint(1, 6, size=(12, 1)).astype(float), (0, 0), (11, 0), conn, SQRT2))
        blocked = rng.randint(1, 6, size=(1, 9)).astype(float)
        blocked[0, 4] = np.inf
        cases.append((f"one_row_blocked_{conn}", blocked, (0, 0), (0, 8), conn, SQRT2))
        zeros = np.zeros((5, 5))
        zeros[2, :] = 1.0
        cases.append((f"zero_plateaus_{conn}", zeros, (0, 0), (4, 4), conn, SQRT2))
        nan = np.ones((4, 4))
        nan[1, 1] = nan[2, 2] = np.nan
        cases.append((f"nan_is_an_obstacle_{conn}", nan, (0, 0), (3, 3), conn, SQRT2))
    return cases


def refusals(Dijkstra, grid_to_csr):
    graph = grid_to_csr(np.ones((4, 5)), obstacle_value=np.inf)
    calls = {
        "resolution_zero": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 0, 4], graph, 0.0),
        "resolution_negative": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 0, 4], graph, -1.0),
        "boundary_x": lambda: Dijkstra.plan([0, 0], [1, 1], [5, 5, 0, 4], graph, 1.0),
        "boundary_y": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 4, 0], graph, 1.0),
        "start_outside": lambda: Dijkstra.plan([5.5, 0], [1, 1], [0, 5, 0, 4], graph, 1.0),
        "start_below": lambda: Dijkstra.plan([0, -0.5], [1, 1], [0, 5, 0, 4], graph, 1.0),
        "target_outside": lambda: Dijkstra.plan([0, 0], [1, 4.5], [0, 5, 0, 4], graph, 1.0),
        "size_mismatch": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 6, 0, 4], graph, 1.0),
        "size_mismatch_resolution": lambda: Dijkstra.plan([0, 0], [1, 1], [0, 5, 0, 4], graph, 0.5),
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
    Dijkstra, grid_to_csr, GridMapGenerator = load_reference(args.ref)

    cases = []   # (name, grid, start, goal, connectivity, mult, generated, seed, min_cost, max_cost, proportion)
    seed = 1000
    for k, size in enumerate(SIZES):
        for conn in (4, 8):
            for min_cost in (1, 0):
                for prop in PROPORTIONS:
                    if size[0] * size[1] * (1 - prop) < 3:
                        continue
                    seed += 1
                    max_cost = 5 if (seed % 3) else 2
                    grid, start, goal = GridMapGenerator(size, min_cost, max_cost, prop, random_seed=seed).generate()
                    cases.append((f"generated_{size[0]}x{size[1]}_c{conn}_min{min_cost}_p{prop}", grid, start, goal, conn, SQRT2, 1, seed,
                                  min_cost, max_cost, prop))
    for name, grid, start, goal, conn, mult in hand_made():
        cases.append((name, grid, start, goal, conn, mult, 0, 0, 0, 0, 0.0))

    rows = {k: [] for k in ("name", "hw", "start", "goal", "connectivity", "mult", "boundary", "resolution", "generated", "seed",
                            "min_cost", "max_cost", "obstacle_proportion", "cost", "index_len", "plan_len")}
    grids, index_paths, plan_paths = [], [], []
    t_ref = 0.0
    for k, (name, grid, start, goal, conn, mult, generated, sd, lo, hi, prop) in enumerate(cases):
        h, w = grid.shape
        res = RESOLUTIONS[k % len(RESOLUTIONS)]
        x_min, y_min = float(k % 5 - 2), float(3 - k % 7)
        boundary = [x_min, x_min + w * res, y_min, y_min + h * res]
        graph = grid_to_csr(grid, obstacle_value=np.inf, connectivity=conn, diagonal_cost_multiplier=mult)
        s_idx, t_idx = start[0] * w + start[1], goal[0] * w + goal[1]
        t0 = time.perf_counter()
        path, cost = Dijkstra.plan_graph(int(s_idx), int(t_idx), graph)
        xy = Dijkstra.plan([start[1] * res + x_min, start[0] * res + y_min], [goal[1] * res + x_min, goal[0] * res + y_min],
                           boundary, graph, res)
        t_ref += time.perf_counter() - t0
        xy = np.zeros((0, 2), np.int64) if xy is None else np.asarray(xy)
        assert xy.dtype == np.int64 and len(xy) == len(path), (name, xy.dtype, len(xy), len(path))
        for key, val in (("name", name), ("hw", (h, w)), ("start", start), ("goal", goal), ("connectivity", conn), ("mult", mult),
                         ("boundary", boundary), ("resolution", res), ("generated", generated), ("seed", sd), ("min_cost", lo),
                         ("max_cost", hi), ("obstacle_proportion", prop), ("cost", cost), ("index_len", len(path)),
                         ("plan_len", len(xy))):
            rows[key].append(val)
        grids.append(np.asarray(grid, np.float64).reshape(-1))
        index_paths.append(np.asarray(path, np.int32))
        plan_paths.append(xy.reshape(-1, 2))
    f64 = ("mult", "boundary", "resolution", "obstacle_proportion", "cost")
    arrays = {k: np.asarray(v) if k == "name" else np.asarray(v, np.float64 if k in f64 else np.int32) for k, v in rows.items()}
    arrays.update(grid=np.concatenate(grids), index_path=np.concatenate(index_paths), plan_path=np.concatenate(plan_paths))
    names, messages = refusals(Dijkstra, grid_to_csr)
    arrays.update(refusal_name=np.asarray(names), refusal_message=np.asarray(messages))
    out = os.path.join(args.out, "grid_search.npz")
    write_npz(out, arrays)
    found = int((arrays["index_len"] > 0).sum())
    print(f"{len(cases)} cases ({found} with a path), {os.path.getsize(out)} bytes, reference {1e3 * t_ref / len(cases):.1f} ms per case "
          f"(plan_graph + plan)")


if __name__ == "__main__":
    main()
