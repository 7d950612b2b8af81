"""The hybrid A* of t2d_hybrid_astar (include/t2d.h) as a plain-Python specification: the reference's
`HybridAStar.plan` (search/hybrid_a_star.py:58-172) statement by statement, with the grid collision checker its test suite pairs
with it (tests/test_search.py:128-191: create_grid_collision_checker) evaluated over the cells near the segment only, the cost
grid held as DEPTHS (g of a node is the running fp64 sum of `depth` copies of step_size, a strictly increasing function of the
depth: `check_costs` keeps the fp64 grid beside it and asserts every prune decision equal), and cos / sin through `oracle.sincos`,
the C restatement of the device's sincos_det -- so every number here has the device's bits.  tan never runs here or there: the
caller passes delta[s] = tan(steer) / wheelbase * step_size (steer_deltas).

The open set is a heapq of (f, node index) tuples as in the reference.  The second member is unique, so a pop is the minimum of a
total order whatever the heap's layout: the kernel's argmin over an unordered array pops the same sequence."""
import heapq
import math

import numpy as np

FOUND, NO_PATH, MAX_ITER, TRUNCATED, OVERFLOW, INVALID = range(6)
MAX_OPEN = 2048          # open entries (LDS)
MAX_XY_CELLS = 32768     # x_cells * y_cells of the cost grid
MAX_STEER = 16
EMPTY = 65535            # the cost grid's +inf; depths 0 .. 65534
XY_LIMIT, ANGLE_LIMIT = 1e150, 1e9
HEADING_RES = math.pi / 8
HEADING_CELLS = 16
TWO_PI = 2 * math.pi


def _sincos():
    import oracle.oracle as O
    return O.sincos


def steer_deltas(steering_angles, wheelbase, step_size):
    """hybrid_a_star.py:121-122, on the host with libm's tan as there"""
    return [math.tan(s) / wheelbase * step_size for s in steering_angles]


def heuristic(x, y, h, tx, ty, th):
    """_heuristic as written (it goes negative for a heading difference above 2 pi)"""
    dx = x - tx
    dy = y - ty
    dist = math.sqrt(dx * dx + dy * dy)
    d = abs(h - th)
    d = min(d, TWO_PI - d)
    return dist + d * 0.1


def obstacle_mask(grid):
    g = np.asarray(grid, np.float64)
    return np.isnan(g) | (g == np.inf)


def _range(lo, hi, o, cs, n):
    """the cells of one axis whose centre o + k * cs lies in [lo - 1.5 cs, hi + 1.5 cs], rounded outwards, clamped to 0 .. n - 1"""
    fa = (lo - o) / cs - 1.5
    fb = (hi - o) / cs + 1.5
    if fa < 0.0:
        fa = 0.0
    if fa > n:
        fa = float(n)
    if fb < -1.0:
        fb = -1.0
    if fb > n - 1:
        fb = float(n - 1)
    return int(math.floor(fa)), int(math.ceil(fb))


def slab(x1, y1, x2, y2, cx, cy, half):
    """one obstacle of collide_fn, operation by operation: the closed square of half side `half` centred at (cx, cy)"""
    dx = x2 - x1
    dy = y2 - y1
    ox_min = cx - half
    ox_max = cx + half
    oy_min = cy - half
    oy_max = cy + half
    if abs(dx) < 1e-9:
        if not (ox_min <= x1 <= ox_max):
            return False
        tx_min, tx_max = -math.inf, math.inf
    else:
        tx1 = (ox_min - x1) / dx
        tx2 = (ox_max - x1) / dx
        tx_min = min(tx1, tx2)
        tx_max = max(tx1, tx2)
    if abs(dy) < 1e-9:
        if not (oy_min <= y1 <= oy_max):
            return False
        ty_min, ty_max = -math.inf, math.inf
    else:
        ty1 = (oy_min - y1) / dy
        ty2 = (oy_max - y1) / dy
        ty_min = min(ty1, ty2)
        ty_max = max(ty1, ty2)
    return max(tx_min, ty_min, 0.0) <= min(tx_max, ty_max, 1.0)


def collides(obst, x1, y1, x2, y2, cell_size=1.0, origin=(0.0, 0.0), everywhere=False):
    """collide_fn over the obstacle cells near the segment (everywhere=True: over all of them, the reference's loop)"""
    H, W = obst.shape
    if everywhere:
        c0, c1, r0, r1 = 0, W - 1, 0, H - 1
    else:
        c0, c1 = _range(min(x1, x2), max(x1, x2), origin[0], cell_size, W)
        r0, r1 = _range(min(y1, y2), max(y1, y2), origin[1], cell_size, H)
    half = cell_size / 2.0
    for r in range(r0, r1 + 1):
        row = obst[r]
        for c in range(c0, c1 + 1):
            if row[c] and slab(x1, y1, x2, y2, origin[0] + c * cell_size, origin[1] + r * cell_size, half):
                return True
    return False


def _bad(v, lim):
    return not (abs(v) <= lim)


def solve(grid, start, target, boundary, deltas, step_size=1.0, cell_size=1.0, origin=(0.0, 0.0), max_iter=50000, max_nodes=1 << 16,
          max_path=256, hw=None, stride=None, max_open=MAX_OPEN, check_costs=False, trig=None, record=None):
    """One row of t2d_hybrid_astar -> dict(status, path float64 [max_path, 3] (NaN past the end), path_len, iterations (pops),
    nodes, open_peak).  grid: the row's weights [H, W] (or flat with hw = (H, W)); stride: the entries the row has (default H * W).
    record: a list that receives (popped node, kept primitive indices) per expansion."""
    trig = trig or _sincos()
    out = dict(status=INVALID, path=np.full((max_path, 3), np.nan), path_len=0, iterations=0, nodes=0, open_peak=0)
    grid = np.asarray(grid, np.float64)
    H, W = (int(v) for v in (hw if hw is not None else grid.shape))
    stride = grid.size if stride is None else stride
    sx, sy, sh = (float(v) for v in start)
    tx, ty, th = (float(v) for v in target)
    x_min, x_max, y_min, y_max = (float(v) for v in boundary)
    if any(_bad(v, XY_LIMIT) for v in (sx, sy, tx, ty, x_min, x_max, y_min, y_max)) or _bad(sh, ANGLE_LIMIT) or _bad(th, ANGLE_LIMIT) \
            or any(_bad(float(d), ANGLE_LIMIT) for d in deltas):
        return out
    if x_min >= x_max or y_min >= y_max or H < 1 or W < 1 or H * W > stride:
        return out
    xy_res = step_size * 0.5
    qx, qy = (sx - x_min) / xy_res, (sy - y_min) / xy_res
    cxd, cyd = (x_max - x_min) / xy_res, (y_max - y_min) / xy_res
    if math.isinf(qx) or math.isinf(qy):
        return out
    cxd = (float(math.trunc(cxd)) if math.isfinite(cxd) else cxd) + 1.0
    cyd = (float(math.trunc(cyd)) if math.isfinite(cyd) else cyd) + 1.0
    if not (0.0 <= math.trunc(qx) < cxd and 0.0 <= math.trunc(qy) < cyd):
        return out
    if not (cxd * cyd <= MAX_XY_CELLS):
        out["status"] = OVERFLOW
        return out
    x_cells, y_cells = int(cxd), int(cyd)
    obst = obstacle_mask(grid.reshape(-1)[:H * W].reshape(H, W)).tolist()

    def cell_of(x, y, h):
        xi = int((x - x_min) / xy_res)
        yi = int((y - y_min) / xy_res)
        hi = int((h % TWO_PI) / HEADING_RES)
        if hi >= HEADING_CELLS:
            hi = HEADING_CELLS - 1
        return (xi * y_cells + yi) * HEADING_CELLS + hi

    depth_grid = np.full(x_cells * y_cells * HEADING_CELLS, EMPTY, np.uint16)
    cost_grid = np.full(x_cells * y_cells * HEADING_CELLS, np.inf) if check_costs else None
    # a node: x, y, heading, parent, g, depth
    nodes = [(sx, sy, sh, -1, 0.0, 0)]
    open_set = [(0.0 + heuristic(sx, sy, sh, tx, ty, th), 0)]
    depth_grid[cell_of(sx, sy, sh)] = 0
    if check_costs:
        cost_grid[cell_of(sx, sy, sh)] = 0.0
    iterations, peak, status, goal = 0, 1, None, -1
    half = cell_size / 2.0
    n_steer = len(deltas)
    while True:
        if not open_set:
            status = NO_PATH
            break
        if iterations >= max_iter:
            status = MAX_ITER
            break
        _, idx = heapq.heappop(open_set)
        iterations += 1
        x, y, h, parent, g, depth = nodes[idx]
        if abs(x - tx) < xy_res and abs(y - ty) < xy_res and abs(h - th) < HEADING_RES:
            goal = idx
            break
        new_g = g + step_size
        new_depth = depth + 1
        kept = []   # (primitive, x, y, heading, cell)
        for s in range(n_steer):
            delta = float(deltas[s])
            new_h = h + delta
            avg = h + delta / 2
            sn, cs = trig(avg)
            nx = x + cs * step_size
            ny = y + sn * step_size
            if not (x_min <= nx <= x_max and y_min <= ny <= y_max):
                continue
            c0, c1 = _range(min(x, nx), max(x, nx), origin[0], cell_size, W)
            r0, r1 = _range(min(y, ny), max(y, ny), origin[1], cell_size, H)
            hit = False
            for r in range(r0, r1 + 1):
                row = obst[r]
                for c in range(c0, c1 + 1):
                    if row[c] and slab(x, y, nx, ny, origin[0] + c * cell_size, origin[1] + r * cell_size, half):
                        hit = True
                        break
                if hit:
                    break
            if hit:
                continue
            cell = cell_of(nx, ny, new_h)
            # the sequential prune: against the grid as the earlier primitives of this expansion left it
            prune = new_depth >= depth_grid[cell] or any(k[4] == cell for k in kept)
            if check_costs:
                assert prune == (new_g >= cost_grid[cell]), (idx, s)
                if not prune:
                    cost_grid[cell] = new_g
            if prune:
                continue
            kept.append((s, nx, ny, new_h, cell))
        if record is not None:
            record.append((idx, [k[0] for k in kept]))
        if kept and (new_depth >= EMPTY or len(nodes) + len(kept) > max_nodes or len(open_set) + len(kept) > max_open):
            status = OVERFLOW
            break
        for s, nx, ny, new_h, cell in kept:
            depth_grid[cell] = new_depth
            nodes.append((nx, ny, new_h, idx, new_g, new_depth))
            heapq.heappush(open_set, (new_g + heuristic(nx, ny, new_h, tx, ty, th), len(nodes) - 1))
        peak = max(peak, len(open_set))
    out.update(iterations=iterations, nodes=len(nodes), open_peak=peak)
    if goal < 0:
        out["status"] = status
        return out
    length = nodes[goal][5] + 1
    i = goal
    while i != -1:
        d = nodes[i][5]
        if d < max_path:
            out["path"][d] = nodes[i][:3]
        i = nodes[i][3]
    out.update(status=FOUND if length <= max_path else TRUNCATED, path_len=length)
    return out
