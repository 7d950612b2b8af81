"""The probabilistic roadmap of t2d_prm_plan (include/t2d.h) as a plain-Python specification: the reference's
`PRM.plan` (search/prm.py:52-344) phase by phase, with the grid collision checker its test suite pairs with it
(tests/test_search.py: create_grid_collision_checker) evaluated over the cells near the segment only (hybrid_astar_ref.collides),
the KD-tree restated as the k smallest dx * dx + dy * dy by (d2, index), `np.linalg.norm` written as sqrt(dx * dx + dy * dy), the CSR
matrix and the heap restated as the min-plus fixed point over the edge list with the predecessor rule of grid_pred, and
`np.random.uniform` served by the build's counter stream (t2d_rng.h): sample s takes draws 2 s (x) and 2 s + 1 (y) of the stream whose
state is the query's seed.  fp64, one rounding per operation: every number here has the device's bits.

What the reference does and its docstring does not say is kept: a sampled point is never collision-checked, so a node inside an
obstacle stays in the roadmap as an isolated node; only j > i becomes an edge, so an edge exists because j is near i, not because i is
near j; the guard `iteration < 2 * n_samples` of the sampling loop can never bind, every iteration appends."""
import math

import numpy as np

from hybrid_astar_ref import collides, obstacle_mask
from sample_plan_ref import GAMMA, MASK, draw_at, row_seeds  # noqa: F401  (the stream, shared with the sampling planners)

FOUND, NO_PATH, TRUNCATED, OVERFLOW, INVALID = range(5)
MAX_NODES = 1024
MAX_K = 16
XY_LIMIT = 1e150
EPS = 1e-9


def _bad(v):
    return not (abs(v) <= XY_LIMIT)


def degree_cap(n_nodes, k):
    """the neighbours one node keeps at most: K of the workspace layout"""
    return min(k, n_nodes - 1)


def row_layout(n_samples, k):
    """(N, E, offsets of nodes, dist, edge_cost, edge_ij, scratch, bytes of the row) of one query's share of the workspace"""
    n = n_samples + 2
    e = n * degree_cap(n, k)
    return n, e, 0, 16 * n, 24 * n, 24 * n + 8 * e, 24 * n + 16 * e, (24 * n + 20 * e + 255) & ~255


def sample_nodes(start, target, boundary, seed, n_samples):
    x_min, x_max, y_min, y_max = (float(v) for v in boundary)
    nodes = np.empty((n_samples + 2, 2))
    nodes[0] = start
    nodes[1] = target
    for s in range(n_samples):
        nodes[2 + s, 0] = x_min + (x_max - x_min) * draw_at(seed, 2 * s)
        nodes[2 + s, 1] = y_min + (y_max - y_min) * draw_at(seed, 2 * s + 1)
    return nodes


def neighbours(nodes, i, k_nearest, radius):
    """node i's neighbours in the reference's order (k-nearest mode) or in ascending index (radius mode)"""
    dx = nodes[:, 0] - nodes[i, 0]
    dy = nodes[:, 1] - nodes[i, 1]
    d2 = dx * dx + dy * dy
    if radius is not None:
        near = np.flatnonzero(np.sqrt(d2) <= radius)
        return near[near != i]
    k = min(k_nearest + 1, len(nodes))
    order = np.argsort(d2, kind="stable")[:k]   # (stable: the smaller index first among equal distances)
    return order[order != i]


def fixed_point(n_nodes, ij, cost):
    """g float64 [n_nodes], the sweeps, and per node the sweep that gave it the value it has (0 for the start and for a node never
    reached): every sweep reads the field of the sweep before it"""
    g = np.full(n_nodes, np.inf)
    g[0] = 0.0
    sweeps = 0
    settled = np.zeros(n_nodes, np.int64)
    i, j = (ij[:, 0], ij[:, 1]) if len(ij) else (np.zeros(0, np.int64), np.zeros(0, np.int64))
    while True:
        new = g.copy()
        if len(ij):
            np.minimum.at(new, j, g[i] + cost)
            np.minimum.at(new, i, g[j] + cost)
        sweeps += 1
        if np.array_equal(new, g):
            return g, sweeps, settled
        settled[new != g] = sweeps
        g = new


def predecessors(g, ij, cost, settled):
    """grid_pred's rule over the edge list: of v the u with the smallest (g[u], u) among the neighbours with fl(g[u] + w) == g[v]
    that precede v -- g[u] < g[v], or, at equal g (an edge of cost 0 between coincident nodes), u settled in an earlier sweep than
    v; -1 where there is none.  Whoever gave v its value precedes it, so every walk ends at node 0."""
    pred = np.full(len(g), -1, np.int64)
    if not len(ij):
        return pred
    u = np.concatenate([ij[:, 0], ij[:, 1]]).astype(np.int64)
    v = np.concatenate([ij[:, 1], ij[:, 0]]).astype(np.int64)
    w = np.concatenate([cost, cost])
    gu, gv = g[u], g[v]
    with np.errstate(invalid="ignore"):
        ok = (gv < np.inf) & (gu + w == gv) & ((gu < gv) | ((gu == gv) & (settled[u] < settled[v])))
    u, v, gu = u[ok], v[ok], gu[ok]
    for k in np.lexsort((u, gu))[::-1]:   # (descending: the smallest (g[u], u) is written last)
        pred[v[k]] = u[k]
    return pred


def solve(grid, start, target, boundary, seed, n_samples=1000, k_nearest=10, connection_radius=None, max_degree=32, cell_size=1.0,
          origin=(0.0, 0.0), max_path=256, hw=None, stride=None):
    """One row of t2d_prm_plan -> dict(status, path float64 [max_path, 2] (NaN past the end), path_len, n_edges, sweeps, nodes
    float64 [N, 2], edge_ij int32 [n_edges, 2], edge_cost float64 [n_edges], dist float64 [N], pred int64 [N]).  An INVALID row has
    no nodes, an OVERFLOW row nodes only (dist None)."""
    assert n_samples >= 1 and n_samples + 2 <= MAX_NODES and (connection_radius is not None or 1 <= k_nearest <= MAX_K)
    assert connection_radius is None or (connection_radius > 0 and max_degree >= 1)
    out = dict(status=INVALID, path=np.full((max_path, 2), np.nan), path_len=0, n_edges=0, sweeps=0, nodes=np.zeros((0, 2)),
               edge_ij=np.zeros((0, 2), np.int32), edge_cost=np.zeros(0), dist=None, pred=None)
    grid = np.asarray(grid, np.float64)
    H, W = (int(v) for v in (hw if hw is not None else grid.shape))
    stride = grid.size if stride is None else stride
    sx, sy = (float(v) for v in start)
    tx, ty = (float(v) for v in target)
    x_min, x_max, y_min, y_max = (float(v) for v in boundary)
    if any(_bad(v) for v in (sx, sy, tx, ty, x_min, x_max, y_min, y_max)) or x_min >= x_max or y_min >= y_max:
        return out
    if not (x_min - EPS <= sx <= x_max + EPS and y_min - EPS <= sy <= y_max + EPS and x_min - EPS <= tx <= x_max + EPS
            and y_min - EPS <= ty <= y_max + EPS):
        return out
    if H < 1 or W < 1 or H * W > stride:
        return out
    obst = obstacle_mask(grid.reshape(-1)[:H * W].reshape(H, W))
    seed = int(seed) & MASK
    # 1. the nodes
    nodes = sample_nodes((sx, sy), (tx, ty), (x_min, x_max, y_min, y_max), seed, n_samples)
    n = len(nodes)
    out["nodes"] = nodes
    # 2. - 4. neighbours, collision, the edge list in the reference's order
    radius = None if connection_radius is None else float(connection_radius)
    lists = [neighbours(nodes, i, k_nearest, radius) for i in range(n)]
    if radius is not None and max(len(v) for v in lists) > max_degree:
        out["status"] = OVERFLOW
        return out
    ij, cost = [], []
    for i in range(n):
        for j in lists[i]:
            if i >= j:
                continue
            if not collides(obst, nodes[i, 0], nodes[i, 1], nodes[j, 0], nodes[j, 1], cell_size, origin):
                dx = nodes[i, 0] - nodes[j, 0]
                dy = nodes[i, 1] - nodes[j, 1]
                ij.append((i, int(j)))
                cost.append(math.sqrt(dx * dx + dy * dy))
    ij = np.array(ij, np.int32).reshape(-1, 2)
    cost = np.array(cost, np.float64)
    # 5. the search
    g, sweeps, settled = fixed_point(n, ij, cost)
    pred = predecessors(g, ij, cost, settled)
    path = []
    if g[1] < np.inf:
        v = 1
        while v != -1 and len(path) < n:
            path.append(nodes[v])
            v = pred[v]
        path = path[::-1]
    for k, p in enumerate(path[:max_path]):
        out["path"][k] = p
    length = len(path)
    out.update(status=NO_PATH if length == 0 else (TRUNCATED if length > max_path else FOUND), path_len=length, n_edges=len(ij),
               sweeps=sweeps, edge_ij=ij, edge_cost=cost, dist=g, pred=pred)
    return out
