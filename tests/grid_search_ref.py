"""The grid shortest-path solver of t2d_grid_dijkstra (include/t2d.h) as a numpy specification: relax every cell
against its neighbours until nothing changes, then choose each cell's predecessor by one rule, then walk the path back.

What it restates: search/dijkstra.py (Dijkstra.plan / plan_graph) over the graph of search/graph_utils.py (grid_to_csr).
  * edge weight of two neighbouring free cells: (w[a] + w[b]) / 2.0, times diagonal_cost_multiplier for a diagonal (fp64, one
    rounding per operation; the sum of two doubles does not depend on their order);
  * an edge whose weight is exactly 0 is NOT an edge: the reference walks `graph[i].nonzero()`, which drops stored zeros;
  * g is the min-plus fixed point g[v] = min_u fl(g[u] + e(u, v)), g[source] = 0: rounded addition is monotone, so every order of
    relaxation ends in the bits the reference's heap loop ends in;
  * predecessor of v: among the neighbours u with fl(g[u] + e(u, v)) == g[v] and (g[u], u) < (g[v], v), the one with the
    smallest (g[u], u) -- the order in which the heap closes nodes when every edge is > 0.
"""
import numpy as np

FOUND, NO_PATH, TRUNCATED, INVALID, FIELD_ONLY = 0, 1, 2, 3, 4
ORTHOGONAL = ((0, 1), (1, 0), (0, -1), (-1, 0))
DIAGONAL = ((1, 1), (1, -1), (-1, 1), (-1, -1))


def _shift(a, dr, dc, fill):
    """out[r, c] = a[r + dr, c + dc], `fill` outside the grid"""
    h, w = a.shape
    out = np.full_like(a, fill)
    r0, r1, c0, c1 = max(0, -dr), min(h, h - dr), max(0, -dc), min(w, w - dc)
    if r0 < r1 and c0 < c1:
        out[r0:r1, c0:c1] = a[r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out


def edges(w, connectivity, mult):
    """[(dr, dc, e)]: e[r, c] = weight of the edge between (r, c) and (r + dr, c + dc); +inf where there is none"""
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for k, (dr, dc) in enumerate(ORTHOGONAL + (DIAGONAL if connectivity == 8 else ())):
            e = (w + _shift(w, dr, dc, np.inf)) / 2.0
            if k >= 4:
                e = e * mult
            out.append((dr, dc, np.where(e == 0.0, np.inf, e)))
    return out


def solve(weight, source, target, connectivity=4, mult=1.4142135623730951, max_path=None):
    """One grid: dict(g [H*W], path [max_path] (-1 past the end), path_len, status, sweeps)"""
    weight = np.asarray(weight, np.float64)
    h, wd = weight.shape
    n = h * wd
    max_path = n if max_path is None else max_path
    out = dict(g=np.full(n, np.inf), path=np.full(max_path, -1, np.int32), path_len=0, status=INVALID, sweeps=0)
    w = np.where(np.isnan(weight), np.inf, weight)
    if n == 0 or not 0 <= source < n or not -1 <= target < n or (w < 0).any():
        return out
    if np.isinf(w.flat[source]) or (target >= 0 and np.isinf(w.flat[target])):
        return out
    es = edges(w, connectivity, mult)
    g = np.full((h, wd), np.inf)
    g.flat[source] = 0.0
    sweeps = 0
    with np.errstate(invalid="ignore"):
        while True:
            sweeps += 1
            best = g.copy()
            for dr, dc, e in es:
                cand = _shift(g, dr, dc, np.inf) + e
                best = np.where(cand < best, cand, best)
            if (best == g).all():
                break
            g = best
    out.update(g=g.reshape(-1).copy(), sweeps=sweeps)
    if target < 0:
        out["status"] = FIELD_ONLY
        return out
    # the predecessor of every cell: smallest (g[u], u) among the neighbours that explain g[v] and precede v
    idx = np.arange(n).reshape(h, wd)
    best_g, best_u = np.full((h, wd), np.inf), np.full((h, wd), -1)
    with np.errstate(invalid="ignore"):
        for dr, dc, e in es:
            gu, u = _shift(g, dr, dc, np.inf), _shift(idx, dr, dc, -1)
            ok = (u >= 0) & np.isfinite(g) & (gu + e == g) & ((gu < g) | ((gu == g) & (u < idx)))
            take = ok & ((gu < best_g) | ((gu == best_g) & ((best_u < 0) | (u < best_u))))
            best_g, best_u = np.where(take, gu, best_g), np.where(take, u, best_u)
    pred = best_u.reshape(-1)
    chain, cur = [target], target
    while cur != source and pred[cur] >= 0:
        cur = int(pred[cur])
        chain.append(cur)
    if cur != source:
        out["status"] = NO_PATH
        return out
    chain.reverse()
    k = min(len(chain), max_path)
    out["path"][:k] = chain[:k]
    out.update(path_len=len(chain), status=FOUND if len(chain) <= max_path else TRUNCATED)
    return out


def fold_cost(weight, path, connectivity, mult):
    """the left-folded fp64 cost of an index path, or None where two consecutive cells share no edge"""
    weight = np.asarray(weight, np.float64)
    h, wd = weight.shape
    w = np.where(np.isnan(weight), np.inf, weight).reshape(-1)
    total = np.float64(0.0)
    for a, b in zip(path[:-1], path[1:]):
        dr, dc = abs(b // wd - a // wd), abs(b % wd - a % wd)
        if max(dr, dc) != 1 or (dr + dc == 2 and connectivity != 8) or np.isinf(w[a]) or np.isinf(w[b]):
            return None
        e = (w[a] + w[b]) / 2.0
        if dr + dc == 2:
            e = e * mult
        if e == 0.0:
            return None
        total = total + e
    return float(total)


def world_path(path, width, boundary, resolution):
    """Dijkstra.plan's last lines: integer cell coordinates, scaled and shifted IN PLACE in the integer array they were built in"""
    cells = np.array([[int(p) % width, int(p) // width] for p in path])
    cells[:, 0] = cells[:, 0] * resolution + boundary[0]
    cells[:, 1] = cells[:, 1] * resolution + boundary[2]
    return cells
