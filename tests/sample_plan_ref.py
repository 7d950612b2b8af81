"""The sampling planners of t2d_sample_plan (include/t2d.h) as a plain-Python specification: the reference's
`RRT.plan` (search/rrt.py:74-164), `RRTStar.plan` with `_choose_parent` (search/rrt_star.py:22-201) and `RRTConnect.plan`
(search/rrt_connect.py:72-206) statement by statement, with the grid collision checker its test suite pairs with them
(tests/test_search.py: create_grid_collision_checker) evaluated over the cells near the segment only (hybrid_astar_ref.collides),
`np.hypot` and `np.linalg.norm` written as sqrt(dx * dx + dy * dy), and `np.random.uniform` served by the build's counter stream
(t2d_rng.h, restated as in trackgen_ref.py): iteration k of a query takes draws 2k (x) and 2k + 1 (y) of the stream whose state
is the query's seed.  fp64, one rounding per operation: every number here has the device's bits.

What the reference does and its docstrings do not say is kept: RRT and RRT* return the walk from the start to the LAST node
appended when max_iter runs out (never []), a rewired node's descendants keep their stale costs, RRT-Connect tries ONE segment
to the other tree per append."""
import math

import numpy as np

from hybrid_astar_ref import collides, obstacle_mask

RRT, RRT_STAR, RRT_CONNECT = range(3)
FOUND, MAX_ITER, TRUNCATED, OVERFLOW, INVALID = range(5)
XY_LIMIT = 1e150
LDS_NODES = 512        # kSampleLdsNodes: the nodes whose coordinates the kernel keeps in LDS (nothing here depends on it)
MASK = (1 << 64) - 1
GAMMA = 0x9E3779B97F4A7C15


def _fin(z):
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def draw_at(seed, k):
    """draw k (0 first) of the stream whose state is `seed`"""
    return (_fin((seed + (k + 1) * GAMMA) & MASK) >> 11) * (1.0 / 9007199254740992.0)


def row_seeds(seed, n):
    """the seeds sample_plan_batch derives from ONE integer: row i gets splitmix64's output i + 1 of the state `seed`"""
    return np.array([_fin((int(seed) + (i + 1) * GAMMA) & MASK) for i in range(n)], np.uint64)


def _bad(v):
    return not (abs(v) <= XY_LIMIT)


def solve(kind, grid, start, target, boundary, seed, extension_step=1.0, radius=3.0, cell_size=1.0, origin=(0.0, 0.0), max_iter=600,
          max_nodes=4096, max_path=256, hw=None, stride=None, record=None):
    """One row of t2d_sample_plan -> dict(status, path float64 [max_path, 2] (NaN past the end), path_len, iterations, nodes (a, b),
    xy float64 [nodes, 2], parent int32 [nodes] (-1: a root), cost float64 [nodes] (RRT* only, else None), and for RRT-Connect
    xy_b / parent_b of the tree from the target).  record: a dict that receives the counts `kept_nearest`, `changed_parent`,
    `rewired`, `connect_side` of the run."""
    step = float(extension_step)
    out = dict(status=INVALID, path=np.full((max_path, 2), np.nan), path_len=0, iterations=0, nodes=(0, 0), xy=np.zeros((0, 2)),
               parent=np.zeros(0, np.int32), cost=np.zeros(0) if kind == RRT_STAR else None, xy_b=np.zeros((0, 2)), parent_b=np.zeros(0, np.int32))
    grid = np.asarray(grid, np.float64)
    H, W = (int(v) for v in (hw if hw is not None else grid.shape))
    stride = grid.size if stride is None else stride
    sx, sy = (float(v) for v in start)
    tx, ty = (float(v) for v in target)
    x_min, x_max, y_min, y_max = (float(v) for v in boundary)
    if any(_bad(v) for v in (sx, sy, tx, ty, x_min, x_max, y_min, y_max)) or H < 1 or W < 1 or H * W > stride:
        return out
    obst = obstacle_mask(grid.reshape(-1)[:H * W].reshape(H, W))
    seed = int(seed) & MASK
    r2 = radius * radius
    rec = record if record is not None else {}
    rec.update(kept_nearest=0, changed_parent=0, rewired=0, connect_side=None)

    def hit(x1, y1, x2, y2):
        return collides(obst, x1, y1, x2, y2, cell_size, origin)

    def dist2(tree, px, py):
        """dx * dx + dy * dy from every node of the tree, elementwise in fp64 (numpy rounds each operation once, as the loop would)"""
        pts = (coords_b if tree is tree_b else coords_a)[:len(tree)]
        dx = pts[:, 0] - px
        dy = pts[:, 1] - py
        return dx * dx + dy * dy

    def nearest(tree, px, py):
        return int(np.argmin(dist2(tree, px, py)))   # (the first minimum)

    def walk(tree, idx):
        pts = []
        for _ in range(len(tree)):   # (the bound on the walk: no node twice)
            if idx == -1:
                break
            pts.append((tree[idx][0], tree[idx][1]))
            idx = tree[idx][2]
        return pts[::-1]

    # a node: [x, y, parent, cost]
    tree_a = [[sx, sy, -1, 0.0]]
    tree_b = []
    coords_a, coords_b = np.zeros((max(max_iter, 0) + 2, 2)), np.zeros((max(max_iter, 0) + 2, 2))   # (the trees' x, y once more, for numpy)
    coords_a[0] = sx, sy
    coords_b[0] = tx, ty
    status, iterations, path = None, 0, None
    if kind == RRT_CONNECT:
        if max_nodes < 2:
            status = OVERFLOW
        else:
            tree_b = [[tx, ty, -1, 0.0]]
    it = 0
    while status is None and it < max_iter:
        iterations = it + 1
        rx = x_min + (x_max - x_min) * draw_at(seed, 2 * it)
        ry = y_min + (y_max - y_min) * draw_at(seed, 2 * it + 1)
        from_b = kind == RRT_CONNECT and it % 2 == 1
        from_tree, to_tree = (tree_b, tree_a) if from_b else (tree_a, tree_b)
        it += 1
        ni = nearest(from_tree, rx, ry)
        nx0, ny0 = from_tree[ni][0], from_tree[ni][1]
        dx = rx - nx0
        dy = ry - ny0
        dist = math.sqrt(dx * dx + dy * dy)
        if dist < step:
            new_x, new_y = rx, ry
        else:
            new_x = nx0 + step * dx / dist
            new_y = ny0 + step * dy / dist
        if not (x_min <= new_x <= x_max and y_min <= new_y <= y_max):
            continue
        if hit(nx0, ny0, new_x, new_y):
            continue
        if len(tree_a) + len(tree_b) + 1 > max_nodes:
            status = OVERFLOW
            break
        parent, cost = ni, 0.0
        if kind == RRT_STAR:
            # _choose_parent: in index order, strictly cheaper only
            ddx = new_x - nx0
            ddy = new_y - ny0
            cost = tree_a[ni][3] + math.sqrt(ddx * ddx + ddy * ddy)
            near = np.nonzero(dist2(tree_a, new_x, new_y) <= r2)[0].tolist()
            for i in near:
                px, py, _, c = tree_a[i]
                if not hit(px, py, new_x, new_y):
                    fx = new_x - px
                    fy = new_y - py
                    nc = c + math.sqrt(fx * fx + fy * fy)
                    if nc < cost:
                        parent, cost = i, nc
            rec["kept_nearest" if parent == ni else "changed_parent"] += 1
        (coords_b if from_b else coords_a)[len(from_tree)] = new_x, new_y
        from_tree.append([new_x, new_y, parent, cost])
        new_idx = len(from_tree) - 1
        if kind == RRT_STAR:
            for i in near:   # (the new node is not among them; the distances have not changed)
                px, py, _, c = tree_a[i]
                if not hit(px, py, new_x, new_y):
                    fx = new_x - px
                    fy = new_y - py
                    alt = cost + math.sqrt(fx * fx + fy * fy)
                    if alt < c:
                        tree_a[i][2] = new_idx
                        tree_a[i][3] = alt
                        rec["rewired"] += 1
        if kind == RRT_CONNECT:
            j = nearest(to_tree, new_x, new_y)
            if not hit(new_x, new_y, to_tree[j][0], to_tree[j][1]):
                ia, ib = (j, new_idx) if from_b else (new_idx, j)
                path = walk(tree_a, ia) + walk(tree_b, ib)[::-1]
                rec["connect_side"] = "b" if from_b else "a"
                status = FOUND
        else:
            gx = new_x - tx
            gy = new_y - ty
            gd = math.sqrt(gx * gx + gy * gy)
            if gd < step and not hit(new_x, new_y, tx, ty):
                if len(tree_a) + 1 > max_nodes:
                    status = OVERFLOW
                    break
                tree_a.append([tx, ty, new_idx, cost + gd])
                status = FOUND
    if status is None:
        status = MAX_ITER
    out.update(iterations=iterations, nodes=(len(tree_a), len(tree_b)),
               xy=np.array([n[:2] for n in tree_a], np.float64).reshape(-1, 2), parent=np.array([n[2] for n in tree_a], np.int32),
               cost=np.array([n[3] for n in tree_a], np.float64) if kind == RRT_STAR else None,
               xy_b=np.array([n[:2] for n in tree_b], np.float64).reshape(-1, 2), parent_b=np.array([n[2] for n in tree_b], np.int32))
    if status == OVERFLOW:
        out["status"] = OVERFLOW
        return out
    if kind != RRT_CONNECT:
        path = walk(tree_a, len(tree_a) - 1)   # (in EVERY case: rrt.py:147)
    elif path is None:
        path = []
    length = len(path)
    for k, p in enumerate(path[:max_path]):
        out["path"][k] = p
    if status == FOUND and length > max_path:
        status = TRUNCATED
    out.update(status=status, path_len=length)
    return out
