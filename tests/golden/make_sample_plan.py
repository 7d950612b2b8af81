#!/usr/bin/env python3
"""Golden data for the sampling planners -> sample_plan.npz, made by RUNNING the reference's own RRT.plan, RRTStar.plan and
RRTConnect.plan.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
tactics2d/search/rrt.py, rrt_star.py, rrt_connect.py and tactics2d/map/generator/generate_grid_map.py from their FILES, unmodified
(the relative import `from .rrt import RRT` of the second and third is met by a stand-in package whose path is the directory, so
that search/__init__.py never runs), and executes the definitions of create_grid_collision_checker and extract_obstacles_from_grid
out of the parsed tests/test_search.py.  The draws are served by a shim put where the loaded modules say `np`: everything of numpy
but `random.uniform`, which returns low + (high - low) * u with u the next draw of the build's counter stream (t2d_rng.h) keyed by
the case's seed -- the stream tests/sample_plan_ref.py and the kernel read.  RRTStar._choose_parent is wrapped to count the calls
that did not keep the nearest node.

sample_plan.npz, one row per case (C cases; the generated ones first, then the hand-made ones):
  name [C] str, kind i32 [C] (0 RRT, 1 RRT*, 2 RRT-Connect), hw i32 [C, 2] (height, width), start / target f64 [C, 2],
  boundary f64 [C, 4], extension_step / radius f64 [C], max_iter i32 [C], seed u64 [C], generated i32 [C], grid_seed i32 [C],
  obstacle_proportion f64 [C], found i32 [C] (1: the search ended before max_iter), path_len i32 [C], iterations i32 [C] (draws / 2),
  nodes i32 [C, 2] (tree a, tree b), changed_parent / rewired i32 [C] (RRT*: appends whose parent is not the nearest node; nodes
  whose parent a rewire changed);
  concatenated in case order: grid f64 [sum H*W], path f64 [sum path_len, 2], tree_xy f64 [sum nodes, 2] and tree_parent i32
  [sum nodes] (tree a, then tree b; -1: a root), tree_cost f64 [sum of RRT*'s nodes].

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_sample_plan.py --ref REFERENCE_TREE [--out DIR]

The file is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import ast
import importlib
import io
import os
import sys
import time
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = ((3, 3), (3, 7), (7, 3), (1, 9), (5, 5), (8, 8), (6, 13), (16, 16))
PROPORTIONS = (0.0, 0.1, 0.2, 0.3)
STEPS = (1.0, 0.5, 0.7)
KINDS = ("rrt", "rrt_star", "rrt_connect")
N_SEEDS = 2
LDS_NODES = 512   # T2D_SAMPLE_LDS_NODES (RRT-Connect: half of it per tree)
MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def _fin(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


class CounterRandom:
    """stands where the loaded modules say `np.random`"""

    def __init__(self, seed):
        self.s, self.draws = seed & MASK, 0

    def uniform(self, low, high):
        self.s = (self.s + GAMMA) & MASK
        self.draws += 1
        u = (_fin(self.s) >> 11) * (1.0 / 9007199254740992.0)
        return float(low) + (float(high) - float(low)) * u


class NumpyShim:
    """stands where the loaded modules say `np`: numpy, but for `random`"""

    def __init__(self):
        self.random = None

    def __getattr__(self, name):
        return getattr(np, name)


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def load_reference(ref):
    pkg = types.ModuleType("_ref_search")
    pkg.__path__ = [os.path.join(ref, "tactics2d", "search")]   # (a package without its __init__: only the files asked for load)
    sys.modules["_ref_search"] = pkg
    mods = [importlib.import_module("_ref_search." + name) for name in KINDS]
    spec = importlib.util.spec_from_file_location("_ref_generate_grid_map",
                                                  os.path.join(ref, "tactics2d", "map", "generator", "generate_grid_map.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ref, "tests", "test_search.py")) as fh:
        tree = ast.parse(fh.read())
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("create_grid_collision_checker", "extract_obstacles_from_grid"):
            exec(compile(ast.Module([node], []), "test_search.py", "exec"), ns)
    return mods, gen.GridMapGenerator, ns["create_grid_collision_checker"], ns["extract_obstacles_from_grid"]


def hand_made():
    """(name, grid, start, target, boundary, extension_step, max_iter); each runs with all three kinds"""
    cases = []
    free = lambda h, w: np.ones((h, w))
    full = lambda g: [0.0, float(g.shape[1]), 0.0, float(g.shape[0])]
    g = free(5, 5)
    cases.append(("max_iter_0", g, [1.0, 1.0], [4.0, 3.0], full(g), 1.0, 0))
    cases.append(("max_iter_1", g, [1.0, 1.0], [4.0, 3.0], full(g), 1.0, 1))
    cases.append(("target_within_one_step", g, [1.0, 1.0], [1.5, 1.25], full(g), 1.0, 50))
    cases.append(("step_larger_than_the_map", g, [0.5, 0.5], [4.5, 4.0], full(g), 50.0, 50))
    g = free(7, 7)
    g[3, 3] = np.inf
    cases.append(("target_inside_an_obstacle", g, [1.0, 1.0], [3.0, 3.0], full(g), 1.0, 80))
    # a boundary that is ONE point makes every sample the start itself: the only segment ever tested towards the target is start ->
    # target.  The square's corner (2.5, 2.5) lies on the line y = 5 - x; its edge y = 2.5 on the second line.
    cases.append(("touches_a_corner_diagonally", g, [1.5, 3.5], [4.5, 0.5], [1.5, 1.5, 3.5, 3.5], 10.0, 5))
    cases.append(("runs_along_an_edge", g, [0.5, 2.5], [5.5, 2.5], [0.5, 0.5, 2.5, 2.5], 10.0, 5))
    cases.append(("passes_beside_the_square", g, [0.5, 2.25], [5.5, 2.25], [0.5, 0.5, 2.25, 2.25], 10.0, 5))
    corridor = np.full((5, 12), np.inf)
    corridor[2, :] = 1.0
    cases.append(("corridor_one_cell_wide", corridor, [1.0, 2.0], [10.0, 2.0], full(corridor), 1.0, 400))
    cases.append(("corridor_half_step", corridor, [1.0, 2.0], [6.0, 2.0], full(corridor), 0.5, 400))
    g = free(6, 9)
    g[2, 4] = g[3, 4] = np.inf
    cases.append(("boundary_smaller_than_the_grid", g, [1.0, 2.0], [6.5, 4.0], [0.5, 7.25, 1.0, 4.5], 1.0, 300))
    cases.append(("boundary_wider_than_the_grid", g, [-1.0, 2.0], [9.5, 4.0], [-2.0, 11.0, -1.5, 7.0], 1.0, 300))
    # the target walled in by its eight neighbours on an otherwise free map: nearly every iteration appends, so the tree outgrows the
    # kernel's LDS part (T2D_SAMPLE_LDS_NODES nodes; for RRT-Connect half of them per tree) within 600 iterations
    g = free(16, 16)
    g[13:16, 13:16] = np.inf
    g[14, 14] = 1.0
    cases.append(("walled_in_target_step0.5", g, [2.0, 2.0], [14.0, 14.0], full(g), 0.5, 600))
    cases.append(("walled_in_target_step0.7", g, [8.0, 8.0], [14.0, 14.0], full(g), 0.7, 600))
    nan = free(6, 6)
    nan[2, 3] = np.nan   # (not +inf: extract_obstacles_from_grid sees none -- recorded with the cell made +inf, see main)
    cases.append(("nan_is_an_obstacle", nan, [0.5, 2.0], [5.0, 2.0], full(nan), 1.0, 300))
    return cases


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    mods, GridMapGenerator, make_checker, extract = load_reference(args.ref)
    planners = (mods[0].RRT, mods[1].RRTStar, mods[2].RRTConnect)
    shim = NumpyShim()
    for mod in mods:
        mod.np = shim
    choose = mods[1].RRTStar._choose_parent
    changed = [0]

    def counting_choose(tree, new_node, nearest_idx, radius, obstacles, collide_fn):
        best_parent, best_cost = choose(tree, new_node, nearest_idx, radius, obstacles, collide_fn)
        changed[0] += best_parent != nearest_idx
        return best_parent, best_cost
    mods[1].RRTStar._choose_parent = staticmethod(counting_choose)

    cases = []   # (name, kind, grid, start, target, boundary, step, max_iter, generated, grid_seed, proportion)
    grid_seed, k = 7000, 0
    for size in SIZES:
        for prop in PROPORTIONS:
            for step in STEPS:
                for rep in range(N_SEEDS):
                    grid_seed += 1
                    grid, start, goal = GridMapGenerator(size, 1, 5, prop, random_seed=grid_seed).generate()
                    sx, sy, gx, gy = float(start[1]), float(start[0]), float(goal[1]), float(goal[0])
                    for kind in range(3):
                        # most cases stop early, so that the trees of the unreachable ones stay small in the file; every seventh may
                        # run long, and RRT* on the largest grid is cut at 300 (the reference takes seconds there)
                        max_iter = 600 if k % 7 == 3 else (40 if k % 7 == 5 else 150)
                        if kind == 1 and size == (16, 16):
                            max_iter = min(max_iter, 300)
                        cases.append((f"generated_{size[0]}x{size[1]}_p{prop}_step{step}_{rep}_{KINDS[kind]}", kind, grid, [sx, sy],
                                      [gx, gy], [0.0, float(size[1]), 0.0, float(size[0])], step, max_iter, 1, grid_seed, prop))
                        k += 1
    for name, grid, start, target, boundary, step, max_iter in hand_made():
        for kind in range(3):
            cases.append((f"{name}_{KINDS[kind]}", kind, grid, start, target, boundary, step, max_iter, 0, 0, 0.0))

    keys = ("name", "kind", "hw", "start", "target", "boundary", "extension_step", "radius", "max_iter", "seed", "generated", "grid_seed",
            "obstacle_proportion", "found", "path_len", "iterations", "nodes", "changed_parent", "rewired")
    rows = {key: [] for key in keys}
    grids, paths, tree_xy, tree_parent, tree_cost = [], [], [], [], []
    t_by = {}
    for index, (name, kind, grid, start, target, boundary, step, max_iter, generated, gs, prop) in enumerate(cases):
        seen = np.where(np.isnan(grid), np.inf, grid)   # (the reference's extractor asks np.isinf)
        obstacles = extract(seen)
        seed = _fin((0x5A3F1E + index * GAMMA) & MASK)
        shim.random = CounterRandom(seed)
        changed[0] = 0
        kw = dict(extension_step=step, max_iter=max_iter)
        if kind == 1:
            kw["radius"] = 3.0
        t0 = time.perf_counter()
        path, tree = planners[kind].plan(list(start), list(target), list(boundary), obstacles, make_checker(obstacles), **kw)
        dt = time.perf_counter() - t0
        assert shim.random.draws % 2 == 0
        iterations = shim.random.draws // 2
        trees = tree if kind == 2 else (tree, [])
        if generated:
            t_by.setdefault((kind, grid.shape), []).append((dt, iterations))
        if kind == 2:
            found = int(len(path) > 0)
        else:   # (the reference's own mark of success is the target as the last node, appended by the goal test)
            found = int(iterations < max_iter or (len(tree) >= 2 and tree[-1][2] == len(tree) - 2 and
                                                  (tree[-1][0], tree[-1][1]) == (float(target[0]), float(target[1]))))
        rewired = sum(1 for i, node in enumerate(tree) if node[2] is not None and node[2] > i) if kind == 1 else 0
        for key, val in (("name", name), ("kind", kind), ("hw", grid.shape), ("start", start), ("target", target), ("boundary", boundary),
                         ("extension_step", step), ("radius", 3.0), ("max_iter", max_iter), ("seed", seed), ("generated", generated),
                         ("grid_seed", gs), ("obstacle_proportion", prop), ("found", found), ("path_len", len(path)),
                         ("iterations", iterations), ("nodes", (len(trees[0]), len(trees[1]))), ("changed_parent", changed[0]),
                         ("rewired", rewired)):
            rows[key].append(val)
        grids.append(np.asarray(grid, np.float64).reshape(-1))
        paths.append(np.asarray(path, np.float64).reshape(-1, 2))
        for t in trees:
            tree_xy.append(np.array([(n[0], n[1]) for n in t], np.float64).reshape(-1, 2))
            tree_parent.append(np.array([-1 if n[2] is None else n[2] for n in t], np.int32))
        if kind == 1:
            tree_cost.append(np.array([n[3] for n in tree], np.float64))
    f64 = ("start", "target", "boundary", "extension_step", "radius", "obstacle_proportion")
    arrays = {key: np.asarray(v) if key == "name" else np.asarray(v, np.float64 if key in f64 else (np.uint64 if key == "seed" else np.int32))
              for key, v in rows.items()}
    arrays.update(grid=np.concatenate(grids), path=np.concatenate(paths), tree_xy=np.concatenate(tree_xy),
                  tree_parent=np.concatenate(tree_parent), tree_cost=np.concatenate(tree_cost))
    out = os.path.join(args.out, "sample_plan.npz")
    write_npz(out, arrays)

    kind, found, nodes = arrays["kind"], arrays["found"], arrays["nodes"]
    total = nodes.sum(axis=1)
    print(f"{len(cases)} cases, {int(total.sum())} nodes, {os.path.getsize(out)} bytes")
    for q in range(3):
        m = kind == q
        print(f"  {KINDS[q]}: {int((m & (found == 1)).sum())} found, {int((m & (found == 0)).sum())} stopped by max_iter, "
              f"largest tree {int(total[m].max())}")
        for shape in ((8, 8), (16, 16)):
            v = t_by[(q, shape)]
            print(f"    generated {shape[0]} x {shape[1]}: {1e3 * np.mean([a for a, _ in v]):.1f} ms per query (the slowest "
                  f"{1e3 * max(a for a, _ in v):.0f} ms), {np.mean([b for _, b in v]):.0f} iterations per query")
    outgrow = int(((kind != 2) & (nodes[:, 0] > LDS_NODES)).sum() + ((kind == 2) & (nodes.max(axis=1) > LDS_NODES // 2)).sum())
    side_a = int(((kind == 2) & (found == 1) & (arrays["iterations"] % 2 == 1)).sum())
    side_b = int(((kind == 2) & (found == 1) & (arrays["iterations"] % 2 == 0)).sum())
    print(f"  trees above 64 nodes: {int((total > 64).sum())}, above 512: {int((total > 512).sum())}, outgrowing the LDS part: {outgrow}; "
          f"RRT* cases with a parent that is not the nearest node: {int((arrays['changed_parent'] > 0).sum())}, with a rewired "
          f"parent: {int((arrays['rewired'] > 0).sum())}; RRT-Connect connections from a: {side_a}, from b: {side_b}")
    for q in range(3):
        assert ((kind == q) & (found == 1)).sum() >= 100 and ((kind == q) & (found == 0)).sum() >= 10, "the counts the fixture must have"
    assert (total > 64).sum() >= 5 and (total > 512).sum() >= 2 and outgrow >= 2
    assert (arrays["changed_parent"] > 0).sum() >= 20 and (arrays["rewired"] > 0).sum() >= 20
    assert side_a >= 10 and side_b >= 10
    assert os.path.getsize(out) < 1 << 20


if __name__ == "__main__":
    main()
