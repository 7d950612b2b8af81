#!/usr/bin/env python3
"""Golden data for the hybrid A* -> hybrid_astar.npz, made by RUNNING the reference's own HybridAStar.plan.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
tactics2d/search/hybrid_a_star.py and tactics2d/map/generator/generate_grid_map.py from their FILES, unmodified, and executes the
definition of create_grid_collision_checker out of the parsed tests/test_search.py (that module imports the whole package).  The
pops, the nodes and the open set's peak are counted by a wrapper put in the place of the loaded module's `heapq`.

hybrid_astar.npz, one row per case (C cases; the generated ones first, then the hand-made ones):
  name [C] str, hw i32 [C, 2] (height, width), start / target f64 [C, 3] (x, y, heading), boundary f64 [C, 4],
  step_size / wheelbase f64 [C], max_iter i32 [C], n_steer i32 [C], steering f64 [C, 5] (NaN past n_steer),
  generated i32 [C], seed i32 [C], obstacle_proportion f64 [C],
  path_len i32 [C] (0: the reference returned []), pops / nodes / open_peak i32 [C], exhausted i32 [C] (1: the open set ran empty);
  concatenated in case order: grid f64 [sum H*W], path f64 [sum path_len, 3].

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_hybrid_astar.py --ref REFERENCE_TREE [--out DIR]

The file is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import ast
import heapq
import importlib.util
import io
import math
import os
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((3, 3), (3, 7), (7, 3), (1, 9), (5, 5), (8, 8), (6, 13), (11, 17), (16, 16), (24, 24))
PROPORTIONS = (0.0, 0.1, 0.2, 0.3)
HEADING_OFFSETS = (0.0, 0.4, -0.7)
STEP_SIZES = (1.0, 0.5)
STEERING_SETS = ((0.0,), (-0.5, 0.0, 0.5), (-0.6, -0.3, 0.0, 0.3, 0.6))


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


class CountingHeap:
    """stands where the loaded module says `heapq`"""

    def __init__(self):
        self.pushes = self.pops = self.peak = 0

    def heappush(self, heap, item):
        heapq.heappush(heap, item)
        self.pushes += 1
        self.peak = max(self.peak, len(heap))

    def heappop(self, heap):
        self.pops += 1
        return heapq.heappop(heap)


def load_reference(ref):
    mods = []
    for rel in ("search/hybrid_a_star.py", "map/generator/generate_grid_map.py"):
        spec = importlib.util.spec_from_file_location("_ref_" + os.path.basename(rel)[:-3], os.path.join(ref, "tactics2d", rel))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        mods.append(mod)
    with open(os.path.join(ref, "tests", "test_search.py")) as fh:
        tree = ast.parse(fh.read())
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("create_grid_collision_checker", "extract_obstacles_from_grid"):
            exec(compile(ast.Module([node], []), "test_search.py", "exec"), ns)
    return mods[0], mods[1].GridMapGenerator, ns["create_grid_collision_checker"], ns["extract_obstacles_from_grid"]


def hand_made():
    """(name, grid, start, target, boundary, step_size, steering, max_iter)"""
    std = (-0.5, 0.0, 0.5)
    cases = []
    free = lambda h, w: np.ones((h, w))
    full = lambda g: [0.0, float(g.shape[1]), 0.0, float(g.shape[0])]
    g = free(20, 20)
    cases.append(("goal_behind_start", g, [12.0, 10.0, 0.0], [6.0, 10.0, 0.0], full(g), 1.0, std, 6000))
    cases.append(("goal_behind_start_facing_back", g, [12.0, 10.0, 0.0], [6.0, 10.0, math.pi], full(g), 1.0, std, 6000))
    corridor = np.full((5, 12), np.inf)
    corridor[2, :] = 1.0
    for step in STEP_SIZES:
        cases.append((f"corridor_step{step}", corridor, [1.0, 2.0, 0.0], [10.0, 2.0, 0.0], full(corridor), step, std, 5000))
    cases.append(("corridor_max_iter_3", corridor, [1.0, 2.0, 0.0], [10.0, 2.0, 0.0], full(corridor), 1.0, std, 3))
    cases.append(("corridor_max_iter_0", corridor, [1.0, 2.0, 0.0], [10.0, 2.0, 0.0], full(corridor), 1.0, std, 0))
    cases.append(("corridor_entered_askew", corridor, [1.0, 2.0, 0.2], [10.0, 2.0, 0.0], full(corridor), 0.5, std, 5000))
    g = free(8, 8)
    cases.append(("target_heading_reachable", g, [1.0, 4.0, 0.0], [6.0, 4.0, 0.0], full(g), 1.0, std, 3000))
    cases.append(("target_heading_two_pi_away", g, [1.0, 4.0, 0.0], [6.0, 4.0, 2 * math.pi], full(g), 1.0, std, 3000))
    cases.append(("start_heading_two_pi_away", g, [1.0, 4.0, 2 * math.pi], [6.0, 4.0, 0.0], full(g), 1.0, std, 3000))
    cases.append(("negative_headings", g, [6.0, 4.0, -math.pi], [1.0, 4.0, -math.pi], full(g), 1.0, std, 3000))
    for step in STEP_SIZES:
        cases.append((f"two_primitives_one_cell_step{step}", g, [1.0, 4.0, 0.1], [6.0, 4.5, 0.1], full(g), step, (-0.01, 0.0, 0.01), 3000))
    cases.append(("two_primitives_one_cell_five", g, [1.0, 4.0, 0.1], [6.0, 4.5, 0.1], full(g), 1.0, (-0.02, -0.01, 0.0, 0.01, 0.02), 3000))
    g = free(6, 9)
    g[2, 4] = g[3, 4] = np.inf
    cases.append(("boundary_cells_not_the_grid", g, [1.0, 2.0, 0.0], [6.5, 4.0, 0.3], [0.5, 7.25, 1.0, 4.5], 1.0, std, 4000))
    cases.append(("boundary_cells_not_the_grid_half_step", g, [1.0, 2.0, 0.0], [6.5, 4.0, 0.3], [0.5, 7.25, 1.0, 4.5], 0.5, std, 4000))
    cases.append(("boundary_wider_than_the_grid", g, [-1.0, 2.0, 0.0], [9.5, 4.0, 0.0], [-2.0, 11.0, -1.5, 7.0], 1.0, std, 4000))
    g = free(7, 7)
    g[3, 3] = np.inf
    # the square's corner (2.5, 2.5) lies on the line y = 5 - x; its edge y = 2.5 on the second one's
    cases.append(("touches_a_corner_diagonally", g, [1.5, 3.5, -math.pi / 4], [4.5, 0.5, -math.pi / 4], full(g), 1.0, (0.0,), 200))
    cases.append(("runs_along_an_edge", g, [0.5, 2.5, 0.0], [5.5, 2.5, 0.0], full(g), 1.0, (0.0,), 200))
    cases.append(("runs_along_an_edge_steering", g, [0.5, 2.5, 0.0], [5.5, 2.5, 0.0], full(g), 1.0, std, 3000))
    cases.append(("ends_on_a_corner", g, [1.5, 2.5, 0.0], [5.5, 2.5, 0.0], full(g), 1.0, (0.0,), 200))
    cases.append(("start_inside_an_obstacle", g, [3.0, 3.0, 0.0], [6.0, 3.0, 0.0], full(g), 1.0, std, 500))
    cases.append(("start_is_the_goal", g, [1.0, 1.0, 0.3], [1.2, 0.9, 0.4], full(g), 1.0, std, 500))
    nan = free(6, 6)
    nan[2, 3] = np.nan   # (not +inf: extract_obstacles_from_grid sees none -- recorded with the cell made +inf, see main)
    cases.append(("nan_is_an_obstacle", nan, [0.5, 2.0, 0.0], [5.0, 2.0, 0.0], full(nan), 1.0, std, 3000))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    ref_mod, GridMapGenerator, make_checker, extract = load_reference(args.ref)

    cases = []   # (name, grid, start, target, boundary, step, steering, max_iter, generated, seed, proportion)
    seed, k = 5000, 0
    for size in SIZES:
        for prop in PROPORTIONS:
            for off in HEADING_OFFSETS:
                for step in STEP_SIZES:
                    for steering in STEERING_SETS:
                        seed += 1
                        grid, start, goal = GridMapGenerator(size, 1, 5, prop, random_seed=seed).generate()
                        sx, sy, gx, gy = float(start[1]), float(start[0]), float(goal[1]), float(goal[0])
                        aim = math.atan2(gy - sy, gx - sx)
                        max_iter = 25 if k % 12 == 7 else 20000   # (every twelfth: stopped early, where it gets that far)
                        cases.append((f"generated_{size[0]}x{size[1]}_p{prop}_off{off}_step{step}_steer{len(steering)}", grid,
                                      [sx, sy, aim + off], [gx, gy, aim], [0.0, float(size[1]), 0.0, float(size[0])], step, steering,
                                      max_iter, 1, seed, prop))
                        k += 1
    for name, grid, start, target, boundary, step, steering, max_iter in hand_made():
        cases.append((name, grid, start, target, boundary, step, steering, max_iter, 0, 0, 0.0))

    keys = ("name", "hw", "start", "target", "boundary", "step_size", "wheelbase", "max_iter", "n_steer", "steering", "generated", "seed",
            "obstacle_proportion", "path_len", "pops", "nodes", "open_peak", "exhausted")
    rows = {key: [] for key in keys}
    grids, paths = [], []
    t_ref = 0.0
    t_by = {}
    for name, grid, start, target, boundary, step, steering, max_iter, generated, sd, prop in cases:
        seen = np.where(np.isnan(grid), np.inf, grid)   # (the reference's extractor asks np.isinf)
        obstacles = extract(seen)
        counter = CountingHeap()
        ref_mod.heapq = counter
        t0 = time.perf_counter()
        path = ref_mod.HybridAStar.plan(list(start), list(target), list(boundary), obstacles, make_checker(obstacles), step_size=step,
                                        max_iter=max_iter, steering_angles=list(steering), velocity=1.0, wheelbase=2.5)
        dt = time.perf_counter() - t0
        t_ref += dt
        if generated:
            key = (grid.shape, prop)
            t_by.setdefault(key, []).append((dt, counter.pops))
        pad = list(steering) + [np.nan] * (5 - len(steering))
        for key, val in (("name", name), ("hw", grid.shape), ("start", start), ("target", target), ("boundary", boundary),
                         ("step_size", step), ("wheelbase", 2.5), ("max_iter", max_iter), ("n_steer", len(steering)), ("steering", pad),
                         ("generated", generated), ("seed", sd), ("obstacle_proportion", prop), ("path_len", len(path)),
                         ("pops", counter.pops), ("nodes", counter.pushes), ("open_peak", counter.peak),
                         ("exhausted", int(not path and counter.pushes == counter.pops))):
            rows[key].append(val)
        grids.append(np.asarray(grid, np.float64).reshape(-1))
        paths.append(np.asarray(path, np.float64).reshape(-1, 3))
    f64 = ("start", "target", "boundary", "step_size", "wheelbase", "steering", "obstacle_proportion")
    arrays = {key: np.asarray(v) if key == "name" else np.asarray(v, np.float64 if key in f64 else np.int32) for key, v in rows.items()}
    arrays.update(grid=np.concatenate(grids), path=np.concatenate(paths))
    out = os.path.join(args.out, "hybrid_astar.npz")
    write_npz(out, arrays)

    found = int((arrays["path_len"] >= 3).sum())
    none = int(((arrays["path_len"] == 0) & (arrays["exhausted"] == 1)).sum())
    stopped = int(((arrays["path_len"] == 0) & (arrays["exhausted"] == 0)).sum())
    print(f"{len(cases)} cases: {found} found with three or more states, {none} without a path, {stopped} stopped by max_iter; "
          f"open-set peak > 64: {int((arrays['open_peak'] > 64).sum())}, > 256: {int((arrays['open_peak'] > 256).sum())}, "
          f"max {arrays['open_peak'].max()}; more than 4096 nodes: {int((arrays['nodes'] > 4096).sum())}, max {arrays['nodes'].max()}; "
          f"{os.path.getsize(out)} bytes")
    print(f"reference: {1e3 * t_ref / len(cases):.1f} ms per case, {1e6 * t_ref / arrays['pops'].sum():.1f} us per pop")
    for (shape, prop), v in sorted(t_by.items()):
        if shape in ((16, 16), (24, 24)) and prop in (0.1, 0.3):
            print(f"  generated {shape[0]} x {shape[1]} at {prop}: {1e3 * np.mean([a for a, _ in v]):.1f} ms per query, "
                  f"{np.mean([b for _, b in v]):.0f} pops per query")
    assert found >= 150 and none >= 100 and stopped >= 10, "the counts the fixture must have"
    assert (arrays["open_peak"] > 64).sum() >= 5 and (arrays["open_peak"] > 256).sum() >= 2 and (arrays["nodes"] > 4096).sum() >= 2


if __name__ == "__main__":
    main()
