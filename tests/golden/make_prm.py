#!/usr/bin/env python3
"""Golden data for the probabilistic roadmap -> prm.npz, made by RUNNING the reference's own PRM.plan.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
tactics2d/search/prm.py and tactics2d/map/generator/generate_grid_map.py from their FILES, unmodified, and executes the definitions
of create_grid_collision_checker and extract_obstacles_from_grid out of the parsed tests/test_search.py.  The draws are served by a
shim put where the loaded module says `np`: everything of numpy but `random.uniform`, which returns low + (high - low) * u with u the
next draw of the build's counter stream (t2d_rng.h) keyed by the case's seed -- the stream tests/prm_ref.py and the kernel read.

Every case is also run through the specification (tests/prm_ref.py), and the script STOPS with the case's name when the two disagree
in a decision: the node count, an edge (in order in k-nearest mode, as a set in radius mode) or a path node.  No case is dropped.
REMOVED_FOR_A_TIE names the cases taken out because two distances differ in the last place between the KD-tree and the restatement;
it is empty.  The generated cases take ONE grid seed per (size, proportion, n_samples) -- the trial behind the issue took two over 480
combinations -- and radius mode is recorded only where n_samples <= 62 or the expected degree (N pi r^2 / area) stays at or below 20:
the reference's radius mode has no cap, and all pairs of hundreds of nodes would push the file past the size its sibling
sample_plan.npz has.  Denser radius roadmaps are left to the device tests' fresh batches against the specification.  Exactly coincident nodes are not
recorded here: the KD-tree's order among equal distances is its own.

prm.npz, one row per case (C cases; the generated ones first, then the hand-made ones):
  name [C] str, hw i32 [C, 2] (height, width), start / target f64 [C, 2], boundary f64 [C, 4], n_samples i32 [C], k_nearest i32 [C],
  radius f64 [C] (0: k-nearest mode), seed u64 [C], generated i32 [C], grid_seed i32 [C], obstacle_proportion f64 [C], found i32 [C],
  path_len i32 [C], n_edges i32 [C], has_cost i32 [C] (1: the case's edge costs are recorded -- every COST_EVERY-th case and the
  hand-made ones but the one at the reference's defaults);
  concatenated in case order: grid f64 [sum H*W], path f64 [sum path_len, 2], edge_ij i16 [sum n_edges, 2], edge_cost f64 [sum of
  n_edges over the cases with has_cost].

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_prm.py --ref REFERENCE_TREE [--out DIR] [--time]

--time also prints the reference's time for ONE query at the settings scripts/time_prm.py measures (nothing of it is recorded).
The file is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import ast
import importlib.util
import io
import math
import os
import sys
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
SIZES = ((6, 6), (9, 14), (16, 16), (24, 24))
PROPORTIONS = (0.0, 0.1, 0.3)
N_SAMPLES = (1, 8, 62, 126, 254)
K_NEAREST = (3, 10)
RADII = (2.5, 5.0)
COST_EVERY = 8
REMOVED_FOR_A_TIE = ()   # (name, reason)
MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def _fin(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


class CounterRandom:
    """stands where the loaded module says `np.random`"""

    def __init__(self, seed):
        self.s, self.draws = seed & MASK, 0

    def uniform(self, low, high):
        self.s = (self.s + GAMMA) & MASK
        self.draws += 1
        u = (_fin(self.s) >> 11) * (1.0 / 9007199254740992.0)
        return float(low) + (float(high) - float(low)) * u


class NumpyShim:
    """stands where the loaded module says `np`: numpy, but for `random`"""

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


def _load_file(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def load_reference(ref):
    prm = _load_file("_ref_prm", os.path.join(ref, "tactics2d", "search", "prm.py"))
    gen = _load_file("_ref_generate_grid_map", os.path.join(ref, "tactics2d", "map", "generator", "generate_grid_map.py"))
    with open(os.path.join(ref, "tests", "test_search.py")) as fh:
        tree = ast.parse(fh.read())
    ns = {"np": np}
    for node in tree.body:
        if isinstance(node, ast.FunctionDef) and node.name in ("create_grid_collision_checker", "extract_obstacles_from_grid"):
            exec(compile(ast.Module([node], []), "test_search.py", "exec"), ns)
    return prm, gen.GridMapGenerator, ns["create_grid_collision_checker"], ns["extract_obstacles_from_grid"]


def radius_is_recorded(size, n_samples, radius):
    """radius mode has no cap on a node's degree in the reference: the dense combinations (all pairs of hundreds of nodes) would
    fill the file with edges and are left to the fresh random batches of the device tests"""
    expected_degree = (n_samples + 2) * math.pi * radius * radius / (size[0] * size[1])
    return n_samples <= 62 or expected_degree <= 20.0


def hand_made():
    """(name, grid, start, target, boundary, n_samples, k_nearest, radius or None)"""
    cases = []
    free = lambda h, w: np.ones((h, w))
    full = lambda g: [0.0, float(g.shape[1]), 0.0, float(g.shape[0])]
    g = free(8, 8)
    cases.append(("one_sample_k", g, [1.0, 1.0], [6.0, 5.0], full(g), 1, 10, None))
    cases.append(("one_sample_radius", g, [1.0, 1.0], [6.0, 5.0], full(g), 1, 10, 20.0))
    cases.append(("k_nearest_above_the_node_count", g, [1.0, 1.0], [6.0, 5.0], full(g), 3, 10, None))
    cases.append(("no_obstacles_k", g, [0.5, 0.5], [7.0, 7.0], full(g), 40, 5, None))
    cases.append(("no_obstacles_radius", g, [0.5, 0.5], [7.0, 7.0], full(g), 40, 5, 2.0))
    cases.append(("radius_too_small_for_any_edge", g, [1.0, 1.0], [6.0, 5.0], full(g), 30, 10, 1e-3))
    g = free(9, 9)
    g[4, 4] = np.inf
    cases.append(("start_inside_an_obstacle", g, [4.0, 4.0], [7.0, 7.0], full(g), 60, 10, None))
    cases.append(("target_inside_an_obstacle", g, [1.0, 1.0], [4.25, 3.75], full(g), 60, 10, None))
    cases.append(("target_inside_an_obstacle_radius", g, [1.0, 1.0], [4.25, 3.75], full(g), 60, 10, 3.0))
    wall = free(12, 12)
    wall[:, 6] = np.inf
    wall[3, 6] = 1.0
    cases.append(("wall_with_one_gap_k", wall, [1.0, 9.0], [10.0, 9.0], full(wall), 200, 10, None))
    cases.append(("wall_with_one_gap_radius", wall, [1.0, 9.0], [10.0, 9.0], full(wall), 200, 10, 2.0))
    shut = wall.copy()
    shut[3, 6] = np.inf
    cases.append(("wall_without_a_gap", shut, [1.0, 9.0], [10.0, 9.0], full(shut), 120, 10, None))
    nan = free(6, 6)
    nan[2, 3] = np.nan   # (not +inf: extract_obstacles_from_grid sees none -- recorded with the cell made +inf, see main)
    cases.append(("nan_is_an_obstacle", nan, [0.5, 2.0], [5.0, 2.0], full(nan), 30, 4, None))
    g = free(6, 9)
    g[2, 4] = g[3, 4] = np.inf
    cases.append(("boundary_smaller_than_the_grid", g, [1.0, 2.0], [6.5, 4.0], [0.5, 7.25, 1.0, 4.5], 50, 6, None))
    cases.append(("boundary_wider_than_the_grid", g, [-1.0, 2.0], [9.5, 4.0], [-2.0, 11.0, -1.5, 7.0], 50, 6, None))
    return cases


def run_reference(prm, shim, make_checker, extract, grid, start, target, boundary, seed, n_samples, k_nearest, radius):
    seen = np.where(np.isnan(grid), np.inf, grid)   # (the reference's extractor asks np.isinf)
    obstacles = extract(seen)
    shim.random = CounterRandom(seed)
    t0 = time.perf_counter()
    path, (nodes, edges) = prm.PRM.plan(list(start), list(target), list(boundary), obstacles, make_checker(obstacles), n_samples=n_samples,
                                        k_nearest=k_nearest, connection_radius=radius)
    dt = time.perf_counter() - t0
    assert shim.random.draws == 2 * n_samples
    return path, nodes, edges, dt


def compare(name, R, grid, start, target, boundary, seed, n_samples, k_nearest, radius, path, nodes, edges):
    """the specification against the reference's lists: stops with the case's name at the first decision that differs"""
    s = R.solve(grid, start, target, boundary, seed, n_samples, k_nearest, radius, max_degree=n_samples + 2, max_path=n_samples + 2)
    if len(nodes) != len(s["nodes"]):
        sys.exit(f"{name}: {len(nodes)} nodes in the reference, {len(s['nodes'])} in the specification")
    ref_ij = [(int(i), int(j)) for i, j, _ in edges]
    spec_ij = [tuple(int(v) for v in p) for p in s["edge_ij"]]
    if radius is None and ref_ij != spec_ij or radius is not None and sorted(ref_ij) != sorted(spec_ij):
        differ = sorted(set(ref_ij) ^ set(spec_ij))[:4]
        sys.exit(f"{name}: the edge lists differ ({len(ref_ij)} in the reference, {len(spec_ij)} in the specification; {differ})")
    if len(path) != s["path_len"] or any(tuple(p) != tuple(q) for p, q in zip(path, s["path"])):
        sys.exit(f"{name}: the paths differ ({len(path)} points in the reference, {s['path_len']} in the specification)")
    if not edges:
        return 0.0
    by = {(i, j): c for (i, j), c in zip(spec_ij, s["edge_cost"])}
    return max(abs(c - by[(int(i), int(j))]) / c for i, j, c in edges if c > 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="a checkout of the reference")
    ap.add_argument("--out", default=HERE)
    ap.add_argument("--time", action="store_true")
    args = ap.parse_args()
    import prm_ref as R
    prm, GridMapGenerator, make_checker, extract = load_reference(args.ref)
    shim = NumpyShim()
    prm.np = shim

    cases = []   # (name, grid, start, target, boundary, n_samples, k_nearest, radius, generated, grid_seed, proportion)
    grid_seed = 9000
    for size in SIZES:
        for prop in PROPORTIONS:
            for n_samples in N_SAMPLES:
                grid_seed += 1
                grid, start, goal = GridMapGenerator(size, 1, 5, prop, random_seed=grid_seed).generate()
                sx, sy, gx, gy = float(start[1]), float(start[0]), float(goal[1]), float(goal[0])
                boundary = [0.0, float(size[1]), 0.0, float(size[0])]
                for k in K_NEAREST:
                    cases.append((f"generated_{size[0]}x{size[1]}_p{prop}_n{n_samples}_k{k}", grid, [sx, sy], [gx, gy], boundary, n_samples,
                                  k, None, 1, grid_seed, prop))
                for radius in RADII:
                    if radius_is_recorded(size, n_samples, radius):
                        cases.append((f"generated_{size[0]}x{size[1]}_p{prop}_n{n_samples}_r{radius}", grid, [sx, sy], [gx, gy], boundary,
                                      n_samples, 10, radius, 1, grid_seed, prop))
    for name, grid, start, target, boundary, n_samples, k, radius in hand_made():
        cases.append((name, grid, start, target, boundary, n_samples, k, radius, 0, 0, 0.0))
    grid, start, goal = GridMapGenerator((24, 24), 1, 5, 0.1, random_seed=8999).generate()
    cases.append(("the_reference_defaults", grid, [float(start[1]), float(start[0])], [float(goal[1]), float(goal[0])], [0.0, 24.0, 0.0, 24.0],
                  1000, 10, None, 0, 8999, 0.1))
    cases = [c for c in cases if c[0] not in dict(REMOVED_FOR_A_TIE)]

    keys = ("name", "hw", "start", "target", "boundary", "n_samples", "k_nearest", "radius", "seed", "generated", "grid_seed",
            "obstacle_proportion", "found", "path_len", "n_edges", "has_cost")
    rows = {key: [] for key in keys}
    grids, paths, edge_ij, edge_cost = [], [], [], []
    worst, total_s = 0.0, 0.0
    for index, (name, grid, start, target, boundary, n_samples, k, radius, generated, gs, prop) in enumerate(cases):
        seed = _fin((0x9D2C5680 + index * GAMMA) & MASK)
        path, nodes, edges, dt = run_reference(prm, shim, make_checker, extract, grid, start, target, boundary, seed, n_samples, k, radius)
        total_s += dt
        worst = max(worst, compare(name, R, grid, start, target, boundary, seed, n_samples, k, radius, path, nodes, edges))
        has_cost = int(index % COST_EVERY == 0 or (not generated and name != "the_reference_defaults"))
        for key, val in (("name", name), ("hw", grid.shape), ("start", start), ("target", target), ("boundary", boundary),
                         ("n_samples", n_samples), ("k_nearest", k), ("radius", 0.0 if radius is None else radius), ("seed", seed),
                         ("generated", generated), ("grid_seed", gs), ("obstacle_proportion", prop), ("found", int(len(path) > 0)),
                         ("path_len", len(path)), ("n_edges", len(edges)), ("has_cost", has_cost)):
            rows[key].append(val)
        grids.append(np.asarray(grid, np.float64).reshape(-1))
        paths.append(np.asarray(path, np.float64).reshape(-1, 2))
        edge_ij.append(np.array([(i, j) for i, j, _ in edges], np.int16).reshape(-1, 2))
        if has_cost:
            edge_cost.append(np.array([c for _, _, c in edges], np.float64))
    f64 = ("start", "target", "boundary", "radius", "obstacle_proportion")
    arrays = {key: np.asarray(v) if key == "name" else np.asarray(v, np.float64 if key in f64 else (np.uint64 if key == "seed" else np.int32))
              for key, v in rows.items()}
    arrays.update(grid=np.concatenate(grids), path=np.concatenate(paths), edge_ij=np.concatenate(edge_ij), edge_cost=np.concatenate(edge_cost))
    out = os.path.join(args.out, "prm.npz")
    write_npz(out, arrays)

    found, radius = arrays["found"], arrays["radius"]
    print(f"{len(cases)} cases ({int((radius == 0).sum())} k-nearest, {int((radius > 0).sum())} radius), {int(found.sum())} with a path, "
          f"{int(arrays['n_edges'].sum())} edges, {int((arrays['n_edges'] == 0).sum())} cases without an edge, {os.path.getsize(out)} bytes; "
          f"the reference took {total_s:.1f} s")
    print(f"largest relative difference of an edge cost, specification vs reference: {worst:.3g}")
    assert found.sum() >= 60 and (found == 0).sum() >= 60, "the counts the fixture must have"
    assert os.path.getsize(out) <= os.path.getsize(os.path.join(HERE, "sample_plan.npz"))

    if args.time:
        # ONE query per setting of scripts/time_prm.py, on this machine's CPU
        for side in (16, 24):
            for prop in (0.1, 0.3):
                grid, start, goal = GridMapGenerator((side, side), 1, 5, prop, random_seed=7).generate()
                for n_samples, k, rad in ((126, 10, None), (254, 10, None), (1000, 10, None), (254, 10, 2.5)):
                    _, _, edges, dt = run_reference(prm, shim, make_checker, extract, grid, [float(start[1]), float(start[0])],
                                                    [float(goal[1]), float(goal[0])], [0.0, float(side), 0.0, float(side)], 12345, n_samples,
                                                    k, rad)
                    print(f"  reference, one query: {side} x {side}, p {prop}, n_samples {n_samples}, "
                          f"{'k ' + str(k) if rad is None else 'radius ' + str(rad)}: {1e3 * dt:.1f} ms, {len(edges)} edges")


if __name__ == "__main__":
    main()
