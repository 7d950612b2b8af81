"""The grid A* of t2d_grid_astar (include/t2d.h) as a plain-Python specification with an explicit heap.

What it restates: search/a_star.py (AStar.plan_graph :279-404; AStar.plan :23-276 is the same loop) over the graph of
search/graph_utils.py (grid_to_csr), operation by operation in fp64:
  * edge of two neighbouring free cells: (w[a] + w[b]) / 2.0, times diagonal_cost_multiplier for a diagonal; an edge whose weight is
    exactly 0 is NOT an edge (the reference walks graph[i].nonzero());
  * pop the smallest (f, cell); a popped entry whose cell is closed costs one iteration and nothing else; close, test the target;
    relax every neighbour that is not closed: a STRICTLY smaller g[cur] + e sets came_from, g and f = g + scale * h and pushes;
  * while the open set is not empty and i < max_iter.
The order in which a cell's neighbours are relaxed cannot matter: each relaxation touches its own neighbour only, and the heap's
order of (f, cell) is total.  `also` collects what the fixture's counted preconditions need (stale pops, the popped entries).
"""
import heapq
import math

import numpy as np

FOUND, NO_PATH, TRUNCATED, INVALID, MAX_ITER = 0, 1, 2, 3, 5
H_ZERO, H_EUCLIDEAN, H_MANHATTAN, H_OCTILE, H_TABLE = range(5)
KINDS = {"zero": H_ZERO, "euclidean": H_EUCLIDEAN, "manhattan": H_MANHATTAN, "octile": H_OCTILE, "table": H_TABLE}
NEIGHBOURS = ((0, 1), (1, 0), (0, -1), (-1, 0), (1, 1), (1, -1), (-1, 1), (-1, -1))   # (d_row, d_col): orthogonal first


def heuristic(kind, x, y, hx, hy, mult=1.4142135623730951):
    """h of the cell (x, y) = (col, row) against the point (hx, hy): the built-in kinds, one rounding per operation"""
    dx, dy = np.float64(x) - np.float64(hx), np.float64(y) - np.float64(hy)
    if kind == H_ZERO:
        return np.float64(0.0)
    if kind == H_EUCLIDEAN:
        return np.sqrt(dx * dx + dy * dy)
    ax, ay = abs(dx), abs(dy)
    if kind == H_MANHATTAN:
        return ax + ay
    if kind == H_OCTILE:
        hi, lo = (ax, ay) if ax > ay else (ay, ax)
        return hi + (np.float64(mult) - np.float64(1.0)) * lo
    raise ValueError(kind)


def solve(weight, source, target, kind=H_EUCLIDEAN, htarget=None, table=None, scale=1.0, connectivity=4, mult=1.4142135623730951,
          max_iter=100000, max_path=None, cell_size=1.0, origin=(0.0, 0.0), also=None):
    """One row of t2d_grid_astar -> dict(status, path int32 [max_path] (-1 past the end), path_len, path_xy float64 [max_path, 2]
    (NaN past the end), iterations, expanded, g float64 [H*W], closed uint8 [H*W], parent int32 [H*W]).  htarget None: the target
    cell's own (col, row).  also: a dict that receives stale_at (the iterations that popped a closed cell) and popped ((f, cell) in pop order)."""
    weight = np.asarray(weight, np.float64)
    h, wd = weight.shape
    n = h * wd
    max_path = n if max_path is None else max_path
    out = dict(status=INVALID, path=np.full(max_path, -1, np.int32), path_len=0, path_xy=np.full((max_path, 2), np.nan), iterations=0,
               expanded=0, g=np.full(n, np.inf), closed=np.zeros(n, np.uint8), parent=np.full(n, -1, np.int32))
    w = np.where(np.isnan(weight), np.inf, weight).reshape(-1)
    scale = np.float64(scale)
    if n == 0 or not 0 <= source < n or not 0 <= target < n or (w < 0).any() or not (0.0 <= scale < np.inf):
        return out
    if kind == H_TABLE:
        hs = np.asarray(table, np.float64).reshape(-1)[:n]
    else:
        hx, hy = (target % wd, target // wd) if htarget is None else htarget
        if kind != H_ZERO and not (math.isfinite(hx) and math.isfinite(hy)):
            return out
        with np.errstate(all="ignore"):
            hs = np.array([heuristic(kind, v % wd, v // wd, hx, hy, mult) for v in range(n)], np.float64)
    with np.errstate(all="ignore"):
        sh = scale * hs
    if np.isnan(hs).any() or (hs == -np.inf).any() or np.isnan(sh).any() or np.isinf(w[source]) or np.isinf(w[target]):
        return out
    mult = np.float64(mult)
    g, closed, parent = out["g"], out["closed"], out["parent"]
    g[source] = 0.0
    heap = [(np.float64(0.0) + sh[source], source)]
    i = expanded = 0
    popped, stale_at = [], []
    status = None
    with np.errstate(all="ignore"):
        while True:
            if not heap:
                status = NO_PATH
                break
            if i >= max_iter:
                status = MAX_ITER
                break
            f, cur = heapq.heappop(heap)
            popped.append((f, cur))
            if closed[cur]:
                stale_at.append(i)
                i += 1
                continue
            closed[cur] = 1
            expanded += 1
            if cur == target:
                status = FOUND
                break
            r, c = divmod(cur, wd)
            for k, (dr, dc) in enumerate(NEIGHBOURS[:connectivity]):
                rr, cc = r + dr, c + dc
                if not (0 <= rr < h and 0 <= cc < wd):
                    continue
                nb = rr * wd + cc
                if closed[nb]:
                    continue
                e = (w[cur] + w[nb]) / np.float64(2.0)
                if k >= 4:
                    e = e * mult
                if e == 0.0:
                    continue
                t = g[cur] + e
                if t < g[nb]:
                    parent[nb] = cur
                    g[nb] = t
                    heapq.heappush(heap, (t + sh[nb], nb))
            i += 1
    if also is not None:
        also.update(stale_at=stale_at, popped=popped)
    out.update(iterations=i, expanded=expanded)
    if status == FOUND:
        chain, cur = [target], target
        while parent[cur] >= 0 and len(chain) < n:
            cur = int(parent[cur])
            chain.append(cur)
        chain.reverse()
        k = min(len(chain), max_path)
        out["path"][:k] = chain[:k]
        for j in range(k):
            out["path_xy"][j, 0] = np.float64(origin[0]) + np.float64(chain[j] % wd) * np.float64(cell_size)
            out["path_xy"][j, 1] = np.float64(origin[1]) + np.float64(chain[j] // wd) * np.float64(cell_size)
        out["path_len"] = len(chain)
        status = FOUND if len(chain) <= max_path else TRUNCATED
    out["status"] = status
    return out


def wavy(a, b):
    """An arbitrary heuristic_fn, a pure function of the cell a = [x, y] and the point b: neither admissible nor consistent.  The
    fixture records the reference's AStar.plan with it; AStar.plan here evaluates it per cell on the host (the TABLE kind)."""
    return abs(a[0] - b[0]) * 0.75 + abs(a[1] - b[1]) * 1.25 + ((a[0] * 7 + a[1] * 3) % 5) * 0.1
