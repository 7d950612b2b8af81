"""Grid shortest paths on the device: the reference's `tactics2d.search.Dijkstra` over the graph of
`tactics2d.search.grid_to_csr`, for n weighted obstacle grids in ONE launch of t2d_grid_dijkstra (include/t2d.h).

    field = cost_to_go(weight_grids, sources)                       # float64 [n, H, W] on the device: reward shaping, heuristics
    out = Dijkstra.plan_batch(weight_grids, sources, targets)       # out.field, out.path, out.path_len, out.status: device tensors
    xy = Dijkstra.plan(start, target, boundary, weight_grid, grid_resolution)   # one query with the reference's signature

The device takes the GRID: `grid_to_csr` is not rebuilt, its edge weights are evaluated in flight.  The field equals the
reference's g_score bit for bit and the path is the reference's path (an edge of weight exactly 0 is no edge there and here).

Hybrid A* on the device: the reference's `tactics2d.search.HybridAStar.plan` for n queries in ONE launch of t2d_hybrid_astar
(DESIGN.md 4.22), with the grid collision checker the reference's tests pair with it fixed in the kernel:

    out = HybridAStar.plan_batch(starts, targets, boundaries, weight_grids)     # out.path, out.path_len, out.status, ...: device tensors
    states = HybridAStar.plan(start, target, boundary, weight_grid, grid_collide)   # one query with the reference's signature

The obstacles are the +inf / NaN cells of the SAME weight grids `cost_to_go` takes.  Such a grid comes from the scene a pool holds
on the device -- `ParticipantPool.occupancy_grid` / `sensor.OccupancyGrid`: conservative, obstacles grown by a
clearance, in this layout, with `planner_kwargs()` for cell_size and origin --, from `generator.GridMapGenerator`, or from the caller's
own tensor.  The kernel equals tests/hybrid_astar_ref.py bit
for bit; that specification equals the reference on its recorded fixture (cos / sin are this library's deterministic ones).

The sampling planners on the device: the reference's `RRT.plan`, `RRTStar.plan` and `RRTConnect.plan` for n queries in ONE launch of
t2d_sample_plan, over the same obstacle grids and with the same collision checker:

    out = RRT.plan_batch(starts, targets, boundaries, weight_grids, seeds)      # out.path, out.path_len, out.status, out.xy, ...
    path, tree = RRTStar.plan(start, target, boundary, weight_grid, grid_collide, seed=7)   # the reference's signature and return
    pool.polyline_routes(out.path, out.path_len)                                # the planned paths as the routes traffic follows

The draws come from the build's counter stream, one stream per query keyed by its seed; the kernel equals tests/sample_plan_ref.py
bit for bit, and that makes the reference's decisions when the reference is fed the same draws.

The probabilistic roadmap on the device: the reference's `PRM.plan` for n queries in ONE launch of t2d_prm_plan, over
the same obstacle grids and with the same collision checker and streams of draws; it returns the path AND the roadmap:

    out = PRM.plan_batch(starts, targets, boundaries, weight_grids, seeds, n_samples=254)   # out.path, out.nodes, out.edge_ij, out.dist, ...
    path, (nodes, edges) = PRM.plan(start, target, boundary, weight_grid, grid_collide, seed=7)   # the reference's signature and return

The kernel equals tests/prm_ref.py bit for bit, and that makes the reference's decisions when the reference is fed the same draws.

Grid A* on the device: the reference's `tactics2d.search.AStar` over the same graph, for n queries in ONE launch of t2d_grid_astar
 -- the goal-directed search that stops at the target, with the reference's heap order, closed set, stale pops and
max_iter, a heuristic per launch (zero, euclidean, manhattan, octile, or a table per cell) and its weight:

    out = AStar.plan_batch(weight_grids, sources, targets, heuristic="euclidean", heuristic_scale=1.0)   # out.path, out.path_xy, out.iterations, ...
    xy = AStar.plan(start, target, boundary, weight_grid, euclidean_heuristic, grid_resolution)   # one query with the reference's signature
    pool.polyline_routes(out.path_xy, out.path_len)                             # the planned paths as the routes traffic follows

A* is NOT Dijkstra on these grids: the Euclidean heuristic is inadmissible wherever a cell costs less than 1, so its path can
differ from `Dijkstra.plan`'s and cost more, and its max_iter counts the stale entries its heap pops.  The kernel equals
tests/astar_ref.py bit for bit; that specification equals the reference on its recorded fixture with tolerance 0.

D* (`d_star.py`: `DStar.plan` is D* Lite run once with km = 0 and the reference has no call that replans; its answer is a shortest
path, which `cost_to_go` gives) and MCTS (`mcts.py`: its model is Python callables) remain out of this package.  There is no CPU
fallback.
"""
import math

import numpy as np

from . import _ffi
from . import layout as L
from .interpolator import _is_tensor, _stream_of

SQRT2 = 1.4142135623730951   # grid_to_csr's default diagonal_cost_multiplier
FOUND, NO_PATH, TRUNCATED, INVALID, FIELD_ONLY = L.GRID_FOUND, L.GRID_NO_PATH, L.GRID_TRUNCATED, L.GRID_INVALID, L.GRID_FIELD_ONLY
MAX_CELLS = L.GRID_MAX_CELLS
MAX_ITER = L.GRID_MAX_ITER   # (t2d_grid_astar only)


class GridPaths:
    """What plan_batch returns: device tensors, one row per grid.  field float64 [n, H_max, W_max] (a view of [n, H_max * W_max]:
    grid e is the first hw[e, 0] * hw[e, 1] entries of its flat row, row-major with ITS OWN width; +inf in obstacles and
    unreached cells; the rest is not written), path int32 [n, max_path] (cells row * W + col from source to target, -1 past the
    end), path_len int32 [n] (the FULL length; > max_path: TRUNCATED), status int32 [n] (FOUND, NO_PATH, TRUNCATED, INVALID,
    FIELD_ONLY), sweeps int32 [n] (relaxation rounds), hw int32 [n, 2]."""

    def __init__(self, field, path, path_len, status, sweeps, hw):
        self.field, self.path, self.path_len, self.status, self.sweeps, self.hw = field, path, path_len, status, sweeps, hw

    def flat_field(self):
        """field as float64 [n, H_max * W_max]"""
        return self.field.reshape(self.field.shape[0], -1)


def _i32(x, dev, shape):
    import torch
    t = x.to(dev, torch.int32) if _is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x, np.int32)).to(dev)
    return t.reshape(shape).contiguous()


def _f64(x, dev, shape):
    import torch
    t = x.to(dev, torch.float64) if _is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x, np.float64)).to(dev)
    return t.reshape(shape).contiguous()


# ---- what every batch function takes in the same way ---------------------------------------------------------------------------------
def _grids(weight_grids):
    """weight_grids [n, H_max, W_max] or [H, W], numpy or a CUDA tensor -> (n, h_max, w_max, stride, upload); upload(dev), inside
    the stream context, gives float64 [n, stride] on the device (a contiguous float64 tensor is read in place)"""
    if not _is_tensor(weight_grids):
        weight_grids = np.asarray(weight_grids, np.float64)
    shape = tuple(weight_grids.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3 or shape[1] * shape[2] < 1:
        raise ValueError(f"weight_grids must have shape (n, H, W) or (H, W) with at least one cell, got {tuple(weight_grids.shape)}")
    n, h_max, w_max = shape
    return n, h_max, w_max, h_max * w_max, lambda dev: _f64(weight_grids, dev, (n, h_max * w_max))


def _hw_host(hw, n, h_max, w_max):
    """the host copy of hw, int32 [n, 2] (None: every grid fills its row) -- or None for a device-resident hw, which _hw_dev takes
    as it is"""
    if _is_tensor(hw):
        return None
    return np.tile(np.int32([h_max, w_max]), (n, 1)) if hw is None else np.asarray(hw, np.int32).reshape(n, 2)


def _hw_dev(hw, hw_host, dev, n):
    return _i32(hw if hw_host is None else hw_host, dev, (n, 2))


def _cell_origin(cell_size, origin):
    """-> (cell_size, origin_x, origin_y) as floats"""
    cell_size = float(cell_size)
    if not (1e-150 <= cell_size <= 1e150):
        raise ValueError(f"cell_size must be positive and finite, got {cell_size}")
    if len(origin) != 2 or not all(math.isfinite(float(v)) for v in origin):
        raise ValueError(f"origin must be two finite numbers, got {origin}")
    return cell_size, float(origin[0]), float(origin[1])


def _count(name, value, least=0):
    """int(value), not below `least`"""
    value = int(value)
    if value < least:
        raise ValueError(f"{name} must not be negative, got {value}" if least == 0 else f"{name} must be at least {least}, got {value}")
    return value


def _clamped_iter(max_iter):
    return max(min(int(max_iter), 2 ** 31 - 1), 0)


def _points(what, x, n, cols):
    """starts / targets: [n, cols], or [cols] for one row"""
    if tuple(x.shape if _is_tensor(x) else np.shape(x)) not in ((n, cols), (cols,) if n == 1 else (n, cols)):
        raise ValueError(f"{what} must have shape ({n}, {cols}), got {tuple(np.shape(x))}")
    return x


def _boundaries(boundaries, n):
    """[n, 4], or [4] for all rows"""
    if not _is_tensor(boundaries) and np.ndim(boundaries) == 1:
        return np.tile(np.asarray(boundaries, np.float64).reshape(1, 4), (n, 1))
    return boundaries


def _workspace(need, n, dev):
    """-> (ws, part): the launch's workspace of `need` bytes (allocated on the current stream: reused only behind this launch) and
    part(lo, dtype, *shape): the view [n, *shape] of the bytes from lo of every query's row (a row is a multiple of 256 bytes: every
    part stays aligned); an empty batch has empty parts of the same shapes"""
    import torch
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    rows = ws[:need].view(n, need // n) if n else None

    def part(lo, dtype, *shape):
        if rows is None:
            return torch.empty((0,) + shape, dtype=dtype, device=dev)
        return rows[:, lo:lo + math.prod(shape) * dtype.itemsize].view(dtype).view((n,) + shape)
    return ws, part


def _device_only(who, callback=None, collide_fn=None):
    """the refusals of the one-query calls: a Python callable cannot run in a kernel"""
    if callback is not None:
        raise TypeError(f"{who} runs on the device, where a Python callable cannot be called: callback must be None, got {callback!r}")
    if collide_fn is not None and collide_fn is not grid_collide:
        raise TypeError(f"{who} runs on the device, where a Python callable cannot be called: collide_fn must be None or "
                        "tactics2d_amd.search.grid_collide (the grid collision checker of the reference's tests, which the kernel "
                        f"implements over the weight grid passed as `obstacles`), got {collide_fn!r}")


def _cells(cells, n, hw_host):
    """[n] linear indices from [n] indices or [n, 2] (row, col) pairs (numpy; pairs need the host copy of hw)"""
    c = np.asarray(cells)
    if c.ndim == 2 and c.shape[1] == 2 and c.shape[0] == n:
        if hw_host is None:
            raise ValueError("(row, col) pairs need hw on the host: pass linear cells beside a device-resident hw")
        return c[:, 0].astype(np.int64) * hw_host[:, 1] + c[:, 1]
    return c.reshape(n)


def plan_batch(weight_grids, sources, targets=None, hw=None, connectivity=4, diagonal_cost_multiplier=SQRT2, max_path=None,
               device_id=0, stream=None):
    """t2d_grid_dijkstra: the cost-to-go field and the shortest path of n grids in one launch, asynchronous on `stream`.
    weight_grids [n, H_max, W_max] (or [H, W] for one grid): numpy, or a float64 CUDA tensor (a contiguous one is read in place);
    a cell's traversal cost, +inf or NaN for an obstacle.  hw int [n, 2] (optional): grid e is H x W = hw[e], stored row-major
    in the first H * W entries of its flat row; default: every grid fills its row.  sources / targets: int [n] linear cells
    row * W + col (numpy or CUDA tensors), or numpy [n, 2] (row, col) pairs; targets None or -1: the field only.  max_path: the
    columns of `path` (default: H_max * W_max with targets, 0 without).  Returns GridPaths.  ValueError: another connectivity, a
    multiplier that is negative or not finite, shapes that disagree; GeometryError: H_max * W_max above MAX_CELLS."""
    import torch
    n, h_max, w_max, stride, upload = _grids(weight_grids)
    mult = _edge_rule(connectivity, diagonal_cost_multiplier)
    hw_host = _hw_host(hw, n, h_max, w_max)
    if not _is_tensor(sources):
        sources = _cells(sources, n, hw_host)
    if targets is not None and not _is_tensor(targets):
        targets = _cells(targets, n, hw_host)
    max_path = _count("max_path", (stride if targets is not None else 0) if max_path is None else max_path)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        w, hw_t = upload(dev), _hw_dev(hw, hw_host, dev, n)
        src = _i32(sources, dev, (n,))
        tgt = torch.full((n,), -1, dtype=torch.int32, device=dev) if targets is None else _i32(targets, dev, (n,))
        field = torch.empty((n, stride), dtype=torch.float64, device=dev)
        path = torch.empty((n, max_path), dtype=torch.int32, device=dev)
        path_len, status, sweeps = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        _ffi.check(lib.t2d_grid_dijkstra(device_id, n, w.data_ptr(), hw_t.data_ptr(), src.data_ptr(), tgt.data_ptr(), stride,
                                         connectivity, mult, max_path, field.data_ptr(), path.data_ptr() if max_path else None,
                                         path_len.data_ptr(), status.data_ptr(), sweeps.data_ptr(), st.cuda_stream), None, lib)
    out = GridPaths(field.reshape(n, h_max, w_max), path, path_len, status, sweeps, hw_t)
    out._inputs = (w, src, tgt)   # (kept alive with the result)
    return out


def cost_to_go(weight_grids, sources, hw=None, connectivity=4, diagonal_cost_multiplier=SQRT2, device_id=0, stream=None):
    """The field-only call: float64 [n, H_max, W_max] on the device, the cost of the cheapest path from sources[e] to every cell of
    grid e (+inf in obstacles, unreached cells and every cell of a row plan_batch would mark INVALID).  Arguments as plan_batch."""
    return plan_batch(weight_grids, sources, None, hw, connectivity, diagonal_cost_multiplier, 0, device_id, stream).field


def _edge_rule(connectivity, diagonal_cost_multiplier):
    """-> the multiplier as a float"""
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    mult = float(diagonal_cost_multiplier)
    if not math.isfinite(mult) or mult < 0:
        raise ValueError(f"diagonal_cost_multiplier must be finite and not negative, got {diagonal_cost_multiplier}")
    return mult


def _grid_query(start, target, boundary, weight_grid, grid_resolution):
    """The head Dijkstra.plan (dijkstra.py:24-266) and AStar.plan (a_star.py:23-276) share: the reference's checks of boundary and
    resolution with its messages, start and target rasterised to cells and clamped -> (width, height, grid float64 [H, W],
    start_rasterized, target_rasterized, start_idx, target_idx)"""
    x_min, x_max, y_min, y_max = boundary
    if grid_resolution <= 0:
        raise ValueError(f"grid_resolution must be positive, got {grid_resolution}")
    if x_min >= x_max or y_min >= y_max:
        raise ValueError(f"Invalid boundary: {boundary}. Must satisfy x_min < x_max and y_min < y_max")
    eps = grid_resolution * 1e-9
    if not (x_min - eps <= start[0] < x_max + eps and y_min - eps <= start[1] < y_max + eps):
        raise ValueError(f"start coordinate {start} is outside boundary {boundary}")
    if not (x_min - eps <= target[0] < x_max + eps and y_min - eps <= target[1] < y_max + eps):
        raise ValueError(f"target coordinate {target} is outside boundary {boundary}")
    width = int((x_max - x_min) / grid_resolution)
    height = int((y_max - y_min) / grid_resolution)
    grid = np.asarray(weight_grid, np.float64)
    if grid.ndim != 2:
        raise ValueError(f"weight_grid must be 2D array, got shape {grid.shape}")
    N = grid.size
    if not math.isclose(width * height, N, rel_tol=1e-9):
        raise ValueError(f"width*height={width*height} does not equal to N={N}. "
                         f"Graph dimensions don't match the calculated grid size.")
    if tuple(grid.shape) != (height, width):
        raise ValueError(f"weight_grid has shape {grid.shape}, the boundary and resolution give ({height}, {width})")
    start_rasterized = [(start[0] - x_min) / grid_resolution, (start[1] - y_min) / grid_resolution]
    target_rasterized = [(target[0] - x_min) / grid_resolution, (target[1] - y_min) / grid_resolution]
    start_x = max(0, min(int(round(start_rasterized[0])), width - 1))
    start_y = max(0, min(int(round(start_rasterized[1])), height - 1))
    target_x = max(0, min(int(round(target_rasterized[0])), width - 1))
    target_y = max(0, min(int(round(target_rasterized[1])), height - 1))
    start_idx = start_y * width + start_x
    target_idx = target_y * width + target_x
    if not (0 <= start_idx < N):
        raise ValueError(f"start_idx {start_idx} out of bounds [0, {N})")
    if not (0 <= target_idx < N):
        raise ValueError(f"target_idx {target_idx} out of bounds [0, {N})")
    return width, height, grid, start_rasterized, target_rasterized, start_idx, target_idx


class Dijkstra:
    """Dijkstra (search/dijkstra.py) over a weight grid."""

    plan_batch = staticmethod(plan_batch)

    @staticmethod
    def plan(start, target, boundary, weight_grid, grid_resolution, connectivity=4, diagonal_cost_multiplier=SQRT2, device_id=0):
        """Dijkstra.plan (dijkstra.py:24-266) with the weight grid [H, W] in place of grid_to_csr's graph of it: start / target
        [x, y] in world coordinates, boundary [x_min, x_max, y_min, y_max].  Returns the reference's array: the path's cells as
        x * grid_resolution + x_min, y * grid_resolution + y_min WRITTEN INTO THE INTEGER ARRAY of cell coordinates (so truncated
        towards zero, as there), None when there is no path, [[x, y]] of `start` when start and target fall into one cell.  The
        reference's ValueErrors are raised with its messages; max_iter is not modelled.  Synchronous: one launch, one download."""
        width, _, grid, _, _, start_idx, target_idx = _grid_query(start, target, boundary, weight_grid, grid_resolution)
        N = grid.size
        if start_idx == target_idx:
            return np.array([[start[0], start[1]]])
        out = plan_batch(grid[None], np.int32([start_idx]), np.int32([target_idx]), None, connectivity, diagonal_cost_multiplier, N,
                         device_id)
        if int(out.status[0]) != FOUND:   # (NO_PATH, or INVALID: an obstacle at either end has no edges in the reference's graph)
            return None
        return world_path(out.path[0, :int(out.path_len[0])].cpu().numpy(), width, boundary, grid_resolution)


def world_path(cells, width, boundary, grid_resolution):
    """The last lines of Dijkstra.plan (dijkstra.py:187-199) for a path of linear cell indices: [x, y] cell coordinates as an
    integer array, scaled and shifted IN PLACE -- numpy casts each column back to the array's integer type."""
    path = np.array([[int(c) % width, int(c) // width] for c in cells])
    path[:, 0] = path[:, 0] * grid_resolution + boundary[0]
    path[:, 1] = path[:, 1] * grid_resolution + boundary[2]
    return path


# ---- grid A* -------------------------------------------------------------------------------------------------------------------------
def zero_heuristic(a, b):
    """h = 0 (A* becomes Dijkstra's search with A*'s bookkeeping).  A marker for `heuristic_fn`: T2D_ASTAR_H_ZERO on the device."""
    return 0.0


def euclidean_heuristic(a, b):
    """sqrt(dx * dx + dy * dy), dx = a[0] - b[0], dy = a[1] - b[1]: euclidean_heuristic of the reference's tests/test_search.py.  A
    marker for `heuristic_fn` (T2D_ASTAR_H_EUCLIDEAN on the device) and, called, the same formula on the host."""
    dx, dy = float(a[0]) - float(b[0]), float(a[1]) - float(b[1])
    return math.sqrt(dx * dx + dy * dy)


def manhattan_heuristic(a, b):
    """|dx| + |dy|.  A marker for `heuristic_fn` (T2D_ASTAR_H_MANHATTAN) and the same formula on the host."""
    return abs(float(a[0]) - float(b[0])) + abs(float(a[1]) - float(b[1]))


def octile_heuristic(a, b, diagonal_cost_multiplier=SQRT2):
    """hi + (diagonal_cost_multiplier - 1.0) * lo, hi / lo the larger / smaller of |dx|, |dy|.  A marker for `heuristic_fn`
    (T2D_ASTAR_H_OCTILE, with the launch's multiplier) and the same formula on the host."""
    ax, ay = abs(float(a[0]) - float(b[0])), abs(float(a[1]) - float(b[1]))
    hi, lo = (ax, ay) if ax > ay else (ay, ax)
    return hi + (float(diagonal_cost_multiplier) - 1.0) * lo


ASTAR_KINDS = {"zero": L.ASTAR_H_ZERO, "euclidean": L.ASTAR_H_EUCLIDEAN, "manhattan": L.ASTAR_H_MANHATTAN, "octile": L.ASTAR_H_OCTILE,
               "table": L.ASTAR_H_TABLE}
_ASTAR_MARKERS = ((zero_heuristic, L.ASTAR_H_ZERO), (euclidean_heuristic, L.ASTAR_H_EUCLIDEAN), (manhattan_heuristic, L.ASTAR_H_MANHATTAN),
                  (octile_heuristic, L.ASTAR_H_OCTILE))


def _marker_kind(fn):
    """ASTAR_H_* of a marker, None for any other object (by identity: a callable need not be hashable)"""
    return next((kind for marker, kind in _ASTAR_MARKERS if fn is marker), None)


class AStarPaths:
    """What astar_plan_batch returns: device tensors, one row per query.  path int32 [n, max_path] (cells row * W + col from source
    to target, -1 past the end), path_xy float64 [n, max_path, 2] (origin + (col, row) * cell_size, NaN past the end: what
    polyline_routes takes), path_len int32 [n] (the FULL length; > max_path: TRUNCATED; 0 without a path), status int32 [n] (FOUND,
    NO_PATH, MAX_ITER, TRUNCATED, INVALID), iterations int32 [n] (the reference's i when it returns), expanded int32 [n] (closed
    cells), hw int32 [n, 2]; with want_state the search's state at termination, else None: g float64 [n, H_max * W_max] (tentative
    values of open cells included, +inf where never reached), closed uint8 and parent int32 (came_from, -1: none) of the same
    shape -- grid e is the first hw[e, 0] * hw[e, 1] entries of its flat row, the rest is not written."""

    def __init__(self, path, path_xy, path_len, status, iterations, expanded, hw, g=None, closed=None, parent=None):
        self.path, self.path_xy, self.path_len, self.status, self.iterations, self.expanded = path, path_xy, path_len, status, iterations, expanded
        self.hw, self.g, self.closed, self.parent = hw, g, closed, parent


def astar_plan_batch(weight_grids, sources, targets, heuristic="euclidean", heuristic_targets=None, heuristic_table=None,
                     heuristic_scale=1.0, hw=None, connectivity=4, diagonal_cost_multiplier=SQRT2, max_iter=100000, max_path=None,
                     cell_size=1.0, origin=(0.0, 0.0), want_state=False, device_id=0, stream=None):
    """t2d_grid_astar: n grid A* queries in one launch, asynchronous on `stream`.  weight_grids, hw, sources, targets, connectivity,
    diagonal_cost_multiplier, max_path: as plan_batch takes them (a target is required).  heuristic: "zero", "euclidean",
    "manhattan", "octile", "table", one of the markers (search.euclidean_heuristic, ...) or ASTAR_H_*, one per launch.
    heuristic_targets float64 [n, 2]: the point (hx, hy) in cell units a built-in heuristic measures the cell (x, y) = (col, row)
    against; None: the target cell's own (col, row).  heuristic_table float64 [n, H_max, W_max] (or [n, H_max * W_max]; the rows in
    the grids' layout): h of every cell, with heuristic="table" -- a Python callable evaluated on the host, or a cost_to_go field;
    +inf is legal, NaN and -inf make the row INVALID.  f = g + heuristic_scale * h.  cell_size, origin: path_xy only
    (OccupancyGrid.planner_kwargs() gives them).  want_state: also g, closed and parent.  Returns AStarPaths.  ValueError: an
    unknown heuristic, a table without "table" or "table" without one, another connectivity, a multiplier that is negative or not
    finite, a cell_size that is not positive and finite, shapes that disagree; GeometryError: H_max * W_max above MAX_CELLS."""
    import torch
    n, h_max, w_max, stride, upload = _grids(weight_grids)
    mult = _edge_rule(connectivity, diagonal_cost_multiplier)
    kind = _marker_kind(heuristic) if callable(heuristic) else ASTAR_KINDS.get(heuristic, heuristic)
    if isinstance(kind, bool) or kind not in ASTAR_KINDS.values():
        raise ValueError(f"heuristic must be one of {sorted(ASTAR_KINDS)}, a marker of this module or search.ASTAR_H_*, got {heuristic!r}")
    if (kind == L.ASTAR_H_TABLE) != (heuristic_table is not None):
        raise ValueError('heuristic="table" and heuristic_table go together')
    cell_size, origin_x, origin_y = _cell_origin(cell_size, origin)
    hw_host = _hw_host(hw, n, h_max, w_max)
    if not _is_tensor(sources):
        sources = _cells(sources, n, hw_host)
    if not _is_tensor(targets):
        targets = _cells(targets, n, hw_host)
    max_path = _count("max_path", stride if max_path is None else max_path)
    max_iter = _clamped_iter(max_iter)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        w, hw_t = upload(dev), _hw_dev(hw, hw_host, dev, n)
        src, tgt = _i32(sources, dev, (n,)), _i32(targets, dev, (n,))
        table = _f64(heuristic_table, dev, (n, stride)) if kind == L.ASTAR_H_TABLE else None
        if kind in (L.ASTAR_H_ZERO, L.ASTAR_H_TABLE):
            point = None
        elif heuristic_targets is None:   # the target cell's own (col, row)
            width = hw_t[:, 1].clamp(min=1)
            point = torch.stack((tgt % width, torch.div(tgt, width, rounding_mode="floor")), 1).to(torch.float64).contiguous()
        else:
            point = _f64(heuristic_targets, dev, (n, 2))
        need = int(lib.t2d_grid_astar_workspace_bytes(n, min(stride, MAX_CELLS), connectivity))
        ws, _ = _workspace(need, n, dev)
        path = torch.empty((n, max_path), dtype=torch.int32, device=dev)
        path_xy = torch.empty((n, max_path, 2), dtype=torch.float64, device=dev)
        path_len, status, iterations, expanded = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        g = torch.empty((n, stride), dtype=torch.float64, device=dev) if want_state else None
        closed = torch.empty((n, stride), dtype=torch.uint8, device=dev) if want_state else None
        parent = torch.empty((n, stride), dtype=torch.int32, device=dev) if want_state else None
        ptr = lambda t: t.data_ptr() if t is not None and t.numel() else None
        if n or stride > MAX_CELLS:   # (an empty batch has no memory to point at and nothing to launch; the cap is refused by name)
            _ffi.check(lib.t2d_grid_astar(device_id, n, w.data_ptr(), hw_t.data_ptr(), src.data_ptr(), tgt.data_ptr(), stride, connectivity,
                                          mult, kind, ptr(point), ptr(table), float(heuristic_scale), max_iter, max_path, cell_size,
                                          origin_x, origin_y, ws.data_ptr(), need, ptr(path), path_len.data_ptr(),
                                          ptr(path_xy), status.data_ptr(), iterations.data_ptr(), expanded.data_ptr(), ptr(g), ptr(closed),
                                          ptr(parent), st.cuda_stream), None, lib)
    out = AStarPaths(path, path_xy, path_len, status, iterations, expanded, hw_t, g, closed, parent)
    out._inputs = (w, src, tgt, point, table, ws)   # (kept alive with the result)
    return out


def _astar_one(who, grid, start_idx, target_idx, heuristic_fn, point, per_cell, max_iter, connectivity, mult, device_id):
    """one query for AStar.plan / plan_graph -> (cells of the path or None, cost).  A marker runs its kind on the device against
    `point`; any other callable is evaluated once per cell on the host (per_cell(cell) -> h) and launched as a table."""
    if not callable(heuristic_fn):
        raise TypeError(f"{who}: heuristic_fn must be callable, got {heuristic_fn!r}")
    n = grid.size
    kw = dict(connectivity=connectivity, diagonal_cost_multiplier=mult, max_iter=max_iter, max_path=n, want_state=True, device_id=device_id)
    if _marker_kind(heuristic_fn) is not None:
        out = astar_plan_batch(grid[None], np.int32([start_idx]), np.int32([target_idx]), heuristic_fn, np.float64([point]), **kw)
    else:
        table = np.array([float(per_cell(v)) for v in range(n)], np.float64)
        if np.isnan(table).any() or (table == -np.inf).any():
            raise ValueError(f"{who}: heuristic_fn returned NaN or -inf for cell {int(np.flatnonzero(np.isnan(table) | (table == -np.inf))[0])}")
        out = astar_plan_batch(grid[None], np.int32([start_idx]), np.int32([target_idx]), "table", heuristic_table=table[None], **kw)
    status = int(out.status[0])
    if status == INVALID:
        flat = grid.reshape(-1)
        if all(math.isfinite(flat[i]) for i in (start_idx, target_idx)):   # (an obstacle at either end has no edges in the reference's graph)
            raise ValueError(f"{who}: the weight grid holds a negative weight")
        return None, math.inf
    if status != FOUND:   # (NO_PATH, or MAX_ITER: the reference returns None for both)
        return None, math.inf
    return out.path[0, :int(out.path_len[0])].cpu().numpy(), float(out.g[0, target_idx])


class AStar:
    """AStar (search/a_star.py) over a weight grid."""

    plan_batch = staticmethod(astar_plan_batch)

    @staticmethod
    def plan(start, target, boundary, weight_grid, heuristic_fn, grid_resolution, max_iter=100000, callback=None, connectivity=4,
             diagonal_cost_multiplier=SQRT2, device_id=0):
        """AStar.plan (a_star.py:23-276) with the reference's argument order and the weight grid [H, W] in place of grid_to_csr's
        graph of it: start / target [x, y] in world coordinates, boundary [x_min, x_max, y_min, y_max].  heuristic_fn: one of the
        markers search.euclidean_heuristic, manhattan_heuristic, octile_heuristic, zero_heuristic -- evaluated on the device against
        the UNROUNDED rasterized target, as the reference calls it --, or any callable heuristic_fn([x, y], target_rasterized): it
        is evaluated ONCE PER CELL on the host before the launch, so it must be a pure function of the cell (the reference calls
        it at every relaxation).  callback must be None (TypeError otherwise: a Python callable cannot run in a kernel).  Returns
        the reference's integer array (see world_path), None when there is no path and when max_iter stopped the search, [[x, y]]
        of `start` when start and target fall into one cell.  The reference's ValueErrors are raised with its messages.
        Synchronous: one launch, one download."""
        _device_only("AStar.plan", callback)
        width, _, grid, _, target_rasterized, start_idx, target_idx = _grid_query(start, target, boundary, weight_grid, grid_resolution)
        if start_idx == target_idx:
            return np.array([[start[0], start[1]]])
        cells, _ = _astar_one("AStar.plan", grid, start_idx, target_idx, heuristic_fn, target_rasterized,
                              lambda v: heuristic_fn([v % width, v // width], target_rasterized), max_iter, connectivity,
                              diagonal_cost_multiplier, device_id)
        return None if cells is None else world_path(cells, width, boundary, grid_resolution)

    @staticmethod
    def plan_graph(start_idx, target_idx, weight_grid, heuristic_fn, max_iter=100000, connectivity=4, diagonal_cost_multiplier=SQRT2,
                   device_id=0):
        """AStar.plan_graph (a_star.py:279-404) over the weight grid [H, W] in place of its graph: cells row * W + col.  heuristic_fn:
        a marker (measured against the target cell's (col, row)) or any callable heuristic_fn(cell, target_cell), evaluated once
        per cell on the host: a pure function of the cell.  Returns (index_path, cost) -- ([start_idx], 0.0) for one cell,
        ([], inf) when the search fails or max_iter stops it.  The reference's ValueErrors for indices out of bounds."""
        grid = np.asarray(weight_grid, np.float64)
        if grid.ndim != 2:
            raise ValueError(f"weight_grid must be 2D array, got shape {grid.shape}")
        n_nodes, width = grid.size, grid.shape[1]
        if not (0 <= start_idx < n_nodes):
            raise ValueError(f"start_idx {start_idx} out of bounds [0, {n_nodes})")
        if not (0 <= target_idx < n_nodes):
            raise ValueError(f"target_idx {target_idx} out of bounds [0, {n_nodes})")
        if start_idx == target_idx:
            return [start_idx], 0.0
        cells, cost = _astar_one("AStar.plan_graph", grid, int(start_idx), int(target_idx), heuristic_fn,
                                 [float(target_idx % width), float(target_idx // width)], lambda v: heuristic_fn(v, target_idx), max_iter,
                                 connectivity, diagonal_cost_multiplier, device_id)
        return ([], math.inf) if cells is None else ([int(c) for c in cells], cost)


# ---- hybrid A* ---------------------------------------------------------------------------------------------------------------------
HYBRID_FOUND, HYBRID_NO_PATH, HYBRID_MAX_ITER = L.HYBRID_FOUND, L.HYBRID_NO_PATH, L.HYBRID_MAX_ITER
HYBRID_TRUNCATED, HYBRID_OVERFLOW, HYBRID_INVALID = L.HYBRID_TRUNCATED, L.HYBRID_OVERFLOW, L.HYBRID_INVALID


def grid_collide(p1, p2, obstacles):
    """The collision function HybridAStar.plan runs on the device, as a marker to pass for `collide_fn` -- and, called, the same test
    on the host: does the segment p1 -> p2 touch the closed unit square of an obstacle cell (+inf or NaN) of the weight grid
    `obstacles`, the cell (row, col) being centred at (x, y) = (col, row)?  It is create_grid_collision_checker of the reference's
    tests/test_search.py over the grid instead of a list of centres."""
    grid = np.asarray(obstacles, np.float64)
    x1, y1 = float(p1[0]), float(p1[1])
    x2, y2 = float(p2[0]), float(p2[1])
    dx, dy = x2 - x1, y2 - y1
    for row, col in zip(*np.nonzero(np.isnan(grid) | (grid == np.inf))):
        ox_min, ox_max, oy_min, oy_max = col - 0.5, col + 0.5, row - 0.5, row + 0.5
        if abs(dx) < 1e-9:
            if not (ox_min <= x1 <= ox_max):
                continue
            tx_min, tx_max = -math.inf, math.inf
        else:
            tx1, tx2 = (ox_min - x1) / dx, (ox_max - x1) / dx
            tx_min, tx_max = min(tx1, tx2), max(tx1, tx2)
        if abs(dy) < 1e-9:
            if not (oy_min <= y1 <= oy_max):
                continue
            ty_min, ty_max = -math.inf, math.inf
        else:
            ty1, ty2 = (oy_min - y1) / dy, (oy_max - y1) / dy
            ty_min, ty_max = min(ty1, ty2), max(ty1, ty2)
        if max(tx_min, ty_min, 0.0) <= min(tx_max, ty_max, 1.0):
            return True
    return False


class HybridPaths:
    """What HybridAStar.plan_batch returns: device tensors, one row per query.  path float64 [n, max_path, 3] (x, y, heading from
    start to goal, NaN past the end; headings are not reduced to [0, 2 pi)), path_len int32 [n] (the FULL length; > max_path:
    HYBRID_TRUNCATED; 0 without a path), status int32 [n] (HYBRID_FOUND, _NO_PATH, _MAX_ITER, _TRUNCATED, _OVERFLOW, _INVALID),
    iterations int32 [n] (pops), nodes int32 [n]."""

    def __init__(self, path, path_len, status, iterations, nodes):
        self.path, self.path_len, self.status, self.iterations, self.nodes = path, path_len, status, iterations, nodes


def steer_deltas(steering_angles, wheelbase, step_size):
    """delta_heading of each motion primitive (hybrid_a_star.py:121-122), on the host with libm's tan as the reference has it"""
    return [math.tan(float(s)) / wheelbase * step_size for s in steering_angles]


def hybrid_plan_batch(starts, targets, boundaries, weight_grids, hw=None, step_size=1.0, max_iter=50000, steering_angles=(-0.5, 0, 0.5),
                      wheelbase=2.5, cell_size=1.0, origin=(0.0, 0.0), max_path=256, max_nodes=65536, device_id=0, stream=None):
    """t2d_hybrid_astar: n hybrid A* queries in one launch, asynchronous on `stream`.  starts / targets [n, 3] (x, y, heading),
    boundaries [n, 4] (x_min, x_max, y_min, y_max) or [4] for all rows, weight_grids [n, H_max, W_max] (or [H, W]) with hw as
    plan_batch takes them: numpy, or float64 CUDA tensors (contiguous ones are read in place).  A cell that is +inf or NaN is an
    obstacle: a closed square of side cell_size centred at origin + (col, row) * cell_size.  max_path: the rows of `path`;
    max_nodes: the nodes one query may append (40 bytes each in the launch's workspace, beside 1 MiB of cost grid per query).
    Returns HybridPaths.  ValueError: no or more than 16 steering angles, a step_size or cell_size that is not positive and
    finite, a wheelbase of 0, shapes that disagree."""
    import torch
    n, h_max, w_max, stride, upload = _grids(weight_grids)
    step_size, wheelbase = float(step_size), float(wheelbase)
    if not (1e-150 <= step_size <= 1e150):
        raise ValueError(f"step_size must be positive and finite, got {step_size}")
    cell_size, origin_x, origin_y = _cell_origin(cell_size, origin)
    if wheelbase == 0 or wheelbase != wheelbase:
        raise ValueError(f"wheelbase must not be 0, got {wheelbase}")
    steering_angles = list(steering_angles)
    if not 1 <= len(steering_angles) <= L.HYBRID_MAX_STEER:
        raise ValueError(f"1 .. {L.HYBRID_MAX_STEER} steering angles, got {len(steering_angles)}")
    max_path, max_nodes, max_iter = _count("max_path", max_path), _count("max_nodes", max_nodes, 1), _clamped_iter(max_iter)
    deltas = steer_deltas(steering_angles, wheelbase, step_size)
    starts, targets, boundaries = _points("starts", starts, n, 3), _points("targets", targets, n, 3), _boundaries(boundaries, n)
    hw_host = _hw_host(hw, n, h_max, w_max)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        w, hw_t = upload(dev), _hw_dev(hw, hw_host, dev, n)
        s_t, t_t, b_t = _f64(starts, dev, (n, 3)), _f64(targets, dev, (n, 3)), _f64(boundaries, dev, (n, 4))
        d_t = _f64(np.float64(deltas), dev, (len(deltas),))
        need = int(lib.t2d_hybrid_astar_workspace_bytes(n, max_nodes))
        ws, _ = _workspace(need, n, dev)
        path = torch.empty((n, max_path, 3), dtype=torch.float64, device=dev)
        path_len, status, iterations, nodes = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        _ffi.check(lib.t2d_hybrid_astar(device_id, n, w.data_ptr(), hw_t.data_ptr(), stride, s_t.data_ptr(), t_t.data_ptr(), b_t.data_ptr(),
                                        d_t.data_ptr(), len(deltas), step_size, cell_size, origin_x, origin_y, max_iter,
                                        max_nodes, max_path, ws.data_ptr(), need, path.data_ptr() if max_path else None,
                                        path_len.data_ptr(), status.data_ptr(), iterations.data_ptr(), nodes.data_ptr(), st.cuda_stream),
                   None, lib)
    out = HybridPaths(path, path_len, status, iterations, nodes)
    out._inputs = (w, hw_t, s_t, t_t, b_t, d_t)   # (kept alive with the result)
    return out


class HybridAStar:
    """HybridAStar (search/hybrid_a_star.py) over a weight grid, with the grid collision checker of the reference's tests."""

    plan_batch = staticmethod(hybrid_plan_batch)

    @staticmethod
    def plan(start, target, boundary, obstacles, collide_fn=None, step_size=1.0, max_iter=50000, steering_angles=(-0.5, 0, 0.5),
             velocity=1.0, wheelbase=2.5, device_id=0):
        """HybridAStar.plan (hybrid_a_star.py:27-157) with the reference's argument order and defaults.  `obstacles` is the weight
        grid [H, W] (+inf or NaN: an obstacle cell, a unit square centred at (col, row)); `collide_fn` must be None or
        `search.grid_collide`, the checker the device runs -- a Python callable cannot run in a kernel, so any other raises
        TypeError.  `velocity` is unused, as in the reference.  Returns the reference's list of [x, y, heading] from start to
        target, [] when there is no path and when max_iter stopped the search.  RuntimeError when the search outgrew the device's
        caps (HYBRID_OVERFLOW): that is not "no path".  ValueError for a row the device calls INVALID.  Synchronous."""
        _device_only("HybridAStar.plan", collide_fn=collide_fn)
        grid = np.asarray(obstacles, np.float64)
        if grid.ndim != 2:
            raise ValueError(f"obstacles must be a 2D weight grid, got shape {grid.shape}")
        max_path = 256
        while True:
            out = hybrid_plan_batch(np.float64([list(start)[:3]]), np.float64([list(target)[:3]]), np.float64([list(boundary)]), grid[None],
                                    None, step_size, max_iter, steering_angles, wheelbase, max_path=max_path, max_nodes=1 << 18,
                                    device_id=device_id)
            status, length = int(out.status[0]), int(out.path_len[0])
            if status != HYBRID_TRUNCATED:
                break
            max_path = length   # (a path longer than the first buffer: once more with its length)
        if status == HYBRID_OVERFLOW:
            raise RuntimeError(f"hybrid A* outgrew the device's caps after {int(out.iterations[0])} pops and {int(out.nodes[0])} nodes "
                               f"(at most {1 << 18} nodes, {L.HYBRID_MAX_OPEN} open entries, {L.HYBRID_MAX_XY_CELLS} x-y cells): "
                               "the search was not finished, which is not the same as no path")
        if status == HYBRID_INVALID:
            raise ValueError(f"start {list(start)}, target {list(target)} or boundary {list(boundary)} is not finite, the boundary is "
                             "empty, or the start lies outside the boundary's cost grid")
        if status != HYBRID_FOUND:
            return []
        return [[float(v) for v in row] for row in out.path[0, :length].cpu().numpy()]


# ---- sampling planners: RRT, RRT*, RRT-Connect -------------------------------------------------------------------------------------
SAMPLE_RRT, SAMPLE_RRT_STAR, SAMPLE_RRT_CONNECT = L.SAMPLE_RRT, L.SAMPLE_RRT_STAR, L.SAMPLE_RRT_CONNECT
SAMPLE_FOUND, SAMPLE_MAX_ITER, SAMPLE_TRUNCATED = L.SAMPLE_FOUND, L.SAMPLE_MAX_ITER, L.SAMPLE_TRUNCATED
SAMPLE_OVERFLOW, SAMPLE_INVALID = L.SAMPLE_OVERFLOW, L.SAMPLE_INVALID
SAMPLE_KINDS = {"rrt": L.SAMPLE_RRT, "rrt_star": L.SAMPLE_RRT_STAR, "rrt_connect": L.SAMPLE_RRT_CONNECT}
SAMPLE_PLAN_MAX_NODES = 1 << 20   # where RRT.plan and its siblings stop doubling max_nodes (28 MiB of workspace)
_MASK64 = (1 << 64) - 1
_GAMMA = 0x9E3779B97F4A7C15


def stream_mix(z):
    """splitmix64's finaliser (t2d_rng.h: stream_mix)"""
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _MASK64
    return z ^ (z >> 31)


def row_seeds(seed, n):
    """The seeds sample_plan_batch derives from ONE integer: row i gets stream_mix(seed + (i + 1) * 0x9E3779B97F4A7C15), output
    i + 1 of the splitmix64 stream whose state is `seed` (mod 2^64).  uint64 [n]."""
    seed = int(seed) & _MASK64
    return np.array([stream_mix((seed + (i + 1) * _GAMMA) & _MASK64) for i in range(n)], np.uint64)


def _seeds(seeds, n):
    """seeds as sample_plan_batch takes them -> upload(dev): the n 64-bit keys on the device"""
    import torch
    if _is_tensor(seeds):
        if seeds.dtype not in (torch.int64, torch.uint64) or tuple(seeds.shape) != (n,):
            raise ValueError(f"seeds as a tensor must be int64 or uint64 [{n}]")
        return lambda dev: seeds.to(dev).contiguous()
    if np.ndim(seeds) == 0:
        seeds = row_seeds(int(seeds), n)
    seeds = np.ascontiguousarray(seeds).astype(np.uint64).reshape(-1)
    if seeds.shape != (n,):
        raise ValueError(f"seeds must be one integer or hold one per row ({n}), got {seeds.shape}")
    return lambda dev: torch.as_tensor(seeds.view(np.int64)).to(dev)


class SamplePaths:
    """What sample_plan_batch returns: device tensors, one row per query.  path float64 [n, max_path, 2] (NaN past the end),
    path_len int32 [n] (the FULL length; > max_path: cut), status int32 [n] (SAMPLE_FOUND, _MAX_ITER, _TRUNCATED, _OVERFLOW,
    _INVALID), iterations int32 [n], nodes int32 [n, 2] (tree a, tree b), and views of the trees in the launch's workspace:
    xy float64 [n, max_nodes, 2], parent int32 [n, max_nodes], cost float64 [n, max_nodes] (None unless RRT*).  Tree a's node i is
    entry i, RRT-Connect's tree b's node j is entry max_nodes - 1 - j; entries past the node counts are not written."""

    def __init__(self, kind, path, path_len, status, iterations, nodes, xy, parent, cost):
        self.kind, self.path, self.path_len, self.status, self.iterations, self.nodes = kind, path, path_len, status, iterations, nodes
        self.xy, self.parent, self.cost = xy, parent, cost

    def tree(self, row, which="a"):
        """(xy float64 [k, 2], parent int32 [k], cost float64 [k] or None) of one row's tree on the host; which "b": RRT-Connect's
        tree from the target, its nodes in the order they were appended"""
        k = int(self.nodes[row, 1 if which == "b" else 0])
        take = (lambda t: t[row].flip(0)[:k]) if which == "b" else (lambda t: t[row, :k])
        return (take(self.xy).cpu().numpy(), take(self.parent).cpu().numpy(),
                None if self.cost is None else take(self.cost).cpu().numpy())


def sample_plan_batch(kind, starts, targets, boundaries, weight_grids, seeds, hw=None, extension_step=1.0, max_iter=100000, radius=3.0,
                      cell_size=1.0, origin=(0.0, 0.0), max_path=256, max_nodes=4096, device_id=0, stream=None):
    """t2d_sample_plan: n RRT / RRT* / RRT-Connect queries in one launch, asynchronous on `stream`.  kind "rrt" / "rrt_star" /
    "rrt_connect" or SAMPLE_*; starts / targets [n, 2], boundaries [n, 4] (x_min, x_max, y_min, y_max) or [4] for all rows,
    weight_grids [n, H_max, W_max] (or [H, W]) with hw, cell_size and origin as hybrid_plan_batch takes them: numpy, or CUDA tensors.
    seeds: uint64 [n] (numpy, or an int64 / uint64 CUDA tensor whose bits are taken), one stream of draws per row -- or ONE integer,
    from which row i gets row_seeds(seeds, n)[i].  Equal seeds in two rows with equal inputs give equal rows.  max_nodes: the nodes
    one query may append, both trees of RRT-Connect together (28 bytes each in the launch's workspace).  radius: RRT*'s.  Returns
    SamplePaths.  ValueError: an unknown kind, an extension_step or cell_size that is not positive and finite, a negative or NaN
    radius, shapes that disagree."""
    import torch
    kind = SAMPLE_KINDS.get(kind, kind)
    if kind not in SAMPLE_KINDS.values() or isinstance(kind, bool):
        raise ValueError(f"kind must be one of {sorted(SAMPLE_KINDS)} or search.SAMPLE_*, got {kind!r}")
    n, h_max, w_max, stride, upload = _grids(weight_grids)
    extension_step, radius = float(extension_step), float(radius)
    if not (1e-150 <= extension_step <= 1e150):
        raise ValueError(f"extension_step must be positive and finite, got {extension_step}")
    cell_size, origin_x, origin_y = _cell_origin(cell_size, origin)
    if not radius >= 0:
        raise ValueError(f"radius must not be negative or NaN, got {radius}")
    max_path, max_nodes, max_iter = _count("max_path", max_path), _count("max_nodes", max_nodes, 1), _clamped_iter(max_iter)
    starts, targets, boundaries = _points("starts", starts, n, 2), _points("targets", targets, n, 2), _boundaries(boundaries, n)
    upload_seeds = _seeds(seeds, n)
    hw_host = _hw_host(hw, n, h_max, w_max)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        w, hw_t, seed_t = upload(dev), _hw_dev(hw, hw_host, dev, n), upload_seeds(dev)
        s_t, t_t, b_t = _f64(starts, dev, (n, 2)), _f64(targets, dev, (n, 2)), _f64(boundaries, dev, (n, 4))
        need = int(lib.t2d_sample_plan_workspace_bytes(n, max_nodes))
        ws, part = _workspace(need, n, dev)
        path = torch.empty((n, max_path, 2), dtype=torch.float64, device=dev)
        path_len, status, iterations = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(3))
        nodes = torch.empty((n, 2), dtype=torch.int32, device=dev)
        _ffi.check(lib.t2d_sample_plan(device_id, n, kind, w.data_ptr(), hw_t.data_ptr(), stride, s_t.data_ptr(), t_t.data_ptr(),
                                       b_t.data_ptr(), seed_t.data_ptr(), extension_step, radius, cell_size, origin_x,
                                       origin_y, max_iter, max_nodes, max_path, ws.data_ptr(), need,
                                       path.data_ptr() if max_path else None, path_len.data_ptr(), status.data_ptr(),
                                       iterations.data_ptr(), nodes.data_ptr(), st.cuda_stream), None, lib)
        xy = part(0, torch.float64, max_nodes, 2)
        cost = part(16 * max_nodes, torch.float64, max_nodes) if kind == SAMPLE_RRT_STAR else None
        parent = part(24 * max_nodes, torch.int32, max_nodes)
    out = SamplePaths(kind, path, path_len, status, iterations, nodes, xy, parent, cost)
    out._inputs = (w, hw_t, s_t, t_t, b_t, seed_t, ws)   # (kept alive with the result)
    return out


def _sample_plan(kind, who, start, target, boundary, obstacles, collide_fn, extension_step, max_iter, radius, callback, seed, device_id):
    """RRT.plan / RRTStar.plan / RRTConnect.plan: one query, synchronous, in the reference's lists"""
    _device_only(f"{who}.plan", callback, collide_fn)
    grid = np.asarray(obstacles, np.float64)
    if grid.ndim != 2:
        raise ValueError(f"obstacles must be a 2D weight grid, got shape {grid.shape}")
    if len(start) < 2 or len(target) < 2 or len(boundary) != 4:
        raise ValueError("start and target must be [x, y], boundary [x_min, x_max, y_min, y_max]")
    if seed is None:
        seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))   # (ONE draw of numpy's global stream: np.random.seed(k) repeats it)
    seed = int(seed) & _MASK64
    max_path, max_nodes = 256, 4096
    while True:
        out = sample_plan_batch(kind, np.float64([list(start)[:2]]), np.float64([list(target)[:2]]), np.float64([list(boundary)]),
                                grid[None], np.array([seed], np.uint64), None, extension_step, max_iter, radius, max_path=max_path,
                                max_nodes=max_nodes, device_id=device_id)
        status, length = int(out.status[0]), int(out.path_len[0])
        if status == SAMPLE_OVERFLOW and max_nodes < SAMPLE_PLAN_MAX_NODES:
            max_nodes *= 2   # (the same seed: the same search with more room)
        elif length > max_path and status in (SAMPLE_TRUNCATED, SAMPLE_MAX_ITER):
            max_path = length   # (a path longer than the first buffer: once more with its length)
        else:
            break
    if status == SAMPLE_OVERFLOW:
        raise RuntimeError(f"{who} outgrew the device's caps after {int(out.iterations[0])} iterations: more than {SAMPLE_PLAN_MAX_NODES} "
                           "nodes; the search was not finished, which is not the same as no path")
    if status == SAMPLE_INVALID:
        raise ValueError(f"start {list(start)}, target {list(target)} or boundary {list(boundary)} is not finite")
    path = [[float(v) for v in p] for p in out.path[0, :length].cpu().numpy()]

    def as_list(which):
        xy, parent, cost = out.tree(0, which)
        return [(float(x), float(y), None if p < 0 else int(p)) + (() if cost is None else (float(cost[i]),))
                for i, ((x, y), p) in enumerate(zip(xy, parent))]
    if kind == SAMPLE_RRT_CONNECT:
        return path, (as_list("a"), as_list("b"))
    return path, as_list("a")


class RRT:
    """RRT (search/rrt.py) over a weight grid, with the grid collision checker of the reference's tests."""

    @staticmethod
    def plan_batch(starts, targets, boundaries, weight_grids, seeds, **kw):
        """sample_plan_batch("rrt", ...)"""
        return sample_plan_batch(SAMPLE_RRT, starts, targets, boundaries, weight_grids, seeds, **kw)

    @staticmethod
    def plan(start, target, boundary, obstacles, collide_fn=None, extension_step=1.0, max_iter=100000, callback=None, seed=None,
             device_id=0):
        """RRT.plan (rrt.py:28-164) with the reference's argument order and defaults.  `obstacles` is the weight grid [H, W] (+inf or
        NaN: an obstacle cell, a unit square centred at (col, row)); `collide_fn` must be None or `search.grid_collide`; `callback`
        must be None (TypeError otherwise: a Python callable cannot run in a kernel).  seed: the 64-bit key of the query's stream
        of draws; None takes ONE draw of numpy's global stream for it, so np.random.seed(k) makes the call reproducible as it does
        the reference's.  Returns the reference's (path, tree): a list of [x, y] from the start and a list of (x, y, parent or
        None).  AS THE REFERENCE DOES, a search that max_iter stopped returns the walk from the start to the last node appended,
        not [].  A tree that outgrows 4096 nodes is searched again with twice the room, up to SAMPLE_PLAN_MAX_NODES, then
        RuntimeError; a path longer than 256 points once more with its length.  ValueError for a row the device calls INVALID.
        Synchronous."""
        return _sample_plan(SAMPLE_RRT, "RRT", start, target, boundary, obstacles, collide_fn, extension_step, max_iter, 3.0, callback,
                            seed, device_id)


class RRTStar:
    """RRTStar (search/rrt_star.py) over a weight grid, with the grid collision checker of the reference's tests."""

    @staticmethod
    def plan_batch(starts, targets, boundaries, weight_grids, seeds, **kw):
        """sample_plan_batch("rrt_star", ...)"""
        return sample_plan_batch(SAMPLE_RRT_STAR, starts, targets, boundaries, weight_grids, seeds, **kw)

    @staticmethod
    def plan(start, target, boundary, obstacles, collide_fn=None, extension_step=1.0, max_iter=100000, radius=3.0, callback=None,
             seed=None, device_id=0):
        """RRTStar.plan (rrt_star.py:39-201): as RRT.plan, with the rewiring `radius`; the tree's nodes are (x, y, parent or None,
        cost).  A rewired node's descendants keep their stale costs, as there."""
        return _sample_plan(SAMPLE_RRT_STAR, "RRTStar", start, target, boundary, obstacles, collide_fn, extension_step, max_iter, radius,
                            callback, seed, device_id)


class RRTConnect:
    """RRTConnect (search/rrt_connect.py) over a weight grid, with the grid collision checker of the reference's tests."""

    @staticmethod
    def plan_batch(starts, targets, boundaries, weight_grids, seeds, **kw):
        """sample_plan_batch("rrt_connect", ...)"""
        return sample_plan_batch(SAMPLE_RRT_CONNECT, starts, targets, boundaries, weight_grids, seeds, **kw)

    @staticmethod
    def plan(start, target, boundary, obstacles, collide_fn=None, extension_step=1.0, max_iter=100000, callback=None, seed=None,
             device_id=0):
        """RRTConnect.plan (rrt_connect.py:28-206): as RRT.plan; returns (path, (tree_a, tree_b)), the path [] when max_iter stopped
        the search."""
        return _sample_plan(SAMPLE_RRT_CONNECT, "RRTConnect", start, target, boundary, obstacles, collide_fn, extension_step, max_iter,
                            3.0, callback, seed, device_id)


# ---- probabilistic roadmaps ----------------------------------------------------------------------------------------------------------
PRM_FOUND, PRM_NO_PATH, PRM_TRUNCATED, PRM_OVERFLOW, PRM_INVALID = L.PRM_FOUND, L.PRM_NO_PATH, L.PRM_TRUNCATED, L.PRM_OVERFLOW, L.PRM_INVALID
PRM_MAX_NODES, PRM_MAX_K = L.PRM_MAX_NODES, L.PRM_MAX_K
PRM_PLAN_MAX_DEGREE = PRM_MAX_NODES   # where PRM.plan stops doubling max_degree: no node has more neighbours than there are nodes


class PRMPaths:
    """What prm_plan_batch returns: device tensors, one row per query.  path float64 [n, max_path, 2] (from the start to the target,
    NaN past the end), path_len int32 [n] (the FULL length; > max_path: PRM_TRUNCATED; 0 without a path), status int32 [n] (PRM_FOUND,
    _NO_PATH, _TRUNCATED, _OVERFLOW, _INVALID), n_edges int32 [n], sweeps int32 [n] (relaxation rounds), and views of the roadmaps in
    the launch's workspace: nodes float64 [n, n_nodes, 2] (node 0 the start, node 1 the target), edge_ij int32 [n, max_edges, 2] and
    edge_cost float64 [n, max_edges] (the first n_edges[e] entries of row e are written), dist float64 [n, n_nodes] (the cost from the
    start to every node, +inf where a node is not connected).  An INVALID row has no roadmap, an OVERFLOW row its nodes only."""

    def __init__(self, path, path_len, status, n_edges, sweeps, nodes, edge_ij, edge_cost, dist):
        self.path, self.path_len, self.status, self.n_edges, self.sweeps = path, path_len, status, n_edges, sweeps
        self.nodes, self.edge_ij, self.edge_cost, self.dist = nodes, edge_ij, edge_cost, dist

    def roadmap(self, row):
        """(nodes, edges) of one row on the host, as PRM.plan returns them: a list of [x, y] and a list of (i, j, cost)"""
        m = int(self.n_edges[row])
        nodes = [] if int(self.status[row]) == PRM_INVALID else [[float(x), float(y)] for x, y in self.nodes[row].cpu().numpy()]
        ij, cost = self.edge_ij[row, :m].cpu().numpy(), self.edge_cost[row, :m].cpu().numpy()
        return nodes, [(int(i), int(j), float(c)) for (i, j), c in zip(ij, cost)]


def prm_plan_batch(starts, targets, boundaries, weight_grids, seeds, hw=None, n_samples=1000, k_nearest=10, connection_radius=None,
                   max_degree=32, cell_size=1.0, origin=(0.0, 0.0), max_path=256, device_id=0, stream=None):
    """t2d_prm_plan: n probabilistic-roadmap queries in one launch, asynchronous on `stream`.  starts / targets [n, 2], boundaries
    [n, 4] (x_min, x_max, y_min, y_max) or [4] for all rows, weight_grids [n, H_max, W_max] (or [H, W]) with hw, cell_size and origin,
    and seeds (uint64 [n], an int64 / uint64 CUDA tensor, or ONE integer: row_seeds) as sample_plan_batch takes them.  Every query
    has n_samples + 2 nodes (at most PRM_MAX_NODES).  connection_radius None: each node is joined to its k_nearest nearest (at most
    PRM_MAX_K); a radius: to every node within it, and a node with more than max_degree of them makes its row PRM_OVERFLOW.  Returns
    PRMPaths.  ValueError: n_samples below 1 or above PRM_MAX_NODES - 2, k_nearest outside 1 .. PRM_MAX_K, a radius that is not
    positive and finite, max_degree below 1, a cell_size that is not positive and finite, shapes that disagree."""
    import torch
    n, h_max, w_max, stride, upload = _grids(weight_grids)
    n_samples, k_nearest, max_degree = int(n_samples), int(k_nearest), int(max_degree)
    if n_samples < 1:
        raise ValueError(f"n_samples must be positive, got {n_samples}")
    if n_samples + 2 > PRM_MAX_NODES:
        raise ValueError(f"n_samples + 2 nodes must not exceed PRM_MAX_NODES = {PRM_MAX_NODES}, got n_samples = {n_samples}")
    by_radius = connection_radius is not None
    if by_radius:
        connection_radius = float(connection_radius)
        if not (0 < connection_radius <= 1e150):
            raise ValueError(f"connection_radius must be positive, got {connection_radius}")
        if max_degree < 1:
            raise ValueError(f"max_degree must be at least 1, got {max_degree}")
    elif not 1 <= k_nearest <= PRM_MAX_K:
        raise ValueError(f"k_nearest must be in 1 .. {PRM_MAX_K}, got {k_nearest}")
    cell_size, origin_x, origin_y = _cell_origin(cell_size, origin)
    max_path = _count("max_path", max_path)
    starts, targets, boundaries = _points("starts", starts, n, 2), _points("targets", targets, n, 2), _boundaries(boundaries, n)
    upload_seeds = _seeds(seeds, n)
    hw_host = _hw_host(hw, n, h_max, w_max)
    n_nodes = n_samples + 2
    k = max_degree if by_radius else k_nearest
    max_edges = n_nodes * min(k, n_nodes - 1)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        w, hw_t, seed_t = upload(dev), _hw_dev(hw, hw_host, dev, n), upload_seeds(dev)
        s_t, t_t, b_t = _f64(starts, dev, (n, 2)), _f64(targets, dev, (n, 2)), _f64(boundaries, dev, (n, 4))
        need = int(lib.t2d_prm_plan_workspace_bytes(n, n_samples, k))
        ws, part = _workspace(need, n, dev)
        path = torch.empty((n, max_path, 2), dtype=torch.float64, device=dev)
        path_len, status, n_edges, sweeps = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
        if n:   # (an empty batch has no memory to point at and nothing to launch)
            _ffi.check(lib.t2d_prm_plan(device_id, n, w.data_ptr(), hw_t.data_ptr(), stride, s_t.data_ptr(), t_t.data_ptr(), b_t.data_ptr(),
                                        seed_t.data_ptr(), n_samples, k_nearest if not by_radius else 1,
                                        connection_radius if by_radius else 0.0, max_degree if by_radius else 1, cell_size, origin_x,
                                        origin_y, max_path, ws.data_ptr(), need, path.data_ptr() if max_path else None,
                                        path_len.data_ptr(), status.data_ptr(), n_edges.data_ptr(), sweeps.data_ptr(), st.cuda_stream),
                       None, lib)
        nodes, dist = part(0, torch.float64, n_nodes, 2), part(16 * n_nodes, torch.float64, n_nodes)
        edge_cost = part(24 * n_nodes, torch.float64, max_edges)
        edge_ij = part(24 * n_nodes + 8 * max_edges, torch.int32, max_edges, 2)
    out = PRMPaths(path, path_len, status, n_edges, sweeps, nodes, edge_ij, edge_cost, dist)
    out._inputs = (w, hw_t, s_t, t_t, b_t, seed_t, ws)   # (kept alive with the result)
    return out


class PRM:
    """PRM (search/prm.py) over a weight grid, with the grid collision checker of the reference's tests."""

    plan_batch = staticmethod(prm_plan_batch)

    @staticmethod
    def plan(start, target, boundary, obstacles, collide_fn=None, n_samples=1000, k_nearest=10, connection_radius=None, max_iter=100000,
             callback=None, seed=None, device_id=0):
        """PRM.plan (prm.py:52-344) with the reference's argument order, defaults and ValueError messages.  `obstacles` is the weight
        grid [H, W] (+inf or NaN: an obstacle cell, a unit square centred at (col, row)); `collide_fn` must be None or
        `search.grid_collide`; `callback` must be None (TypeError otherwise: a Python callable cannot run in a kernel).  seed: the
        64-bit key of the query's stream of draws; None takes ONE draw of numpy's global stream for it.  Returns the reference's
        (path, (nodes, edges)): a list of [x, y] from the start to the target ([] without a path), a list of [x, y] and a list of
        (i, j, cost).  A path longer than 256 points runs once more with its length; in radius mode a node with more than 32
        neighbours doubles the room up to PRM_MAX_NODES, then RuntimeError.  max_iter: the reference's search pops at most
        2 * n_edges + 1 entries, so a max_iter at or above that cannot bind; below it ValueError -- a binding max_iter is not
        modelled.  Synchronous."""
        _device_only("PRM.plan", callback, collide_fn)
        grid = np.asarray(obstacles, np.float64)
        if grid.ndim != 2:
            raise ValueError(f"obstacles must be a 2D weight grid, got shape {grid.shape}")
        if len(start) < 2 or len(target) < 2 or len(boundary) != 4:
            raise ValueError("start and target must be [x, y], boundary [x_min, x_max, y_min, y_max]")
        boundary_arr = np.asarray(boundary)
        x_min, x_max, y_min, y_max = boundary_arr
        if x_min >= x_max or y_min >= y_max:
            raise ValueError(f"Invalid boundary: {boundary_arr}. Must satisfy x_min < x_max and y_min < y_max")
        eps = 1e-9
        for who, point in (("start", start), ("target", target)):
            if not (x_min - eps <= point[0] <= x_max + eps):
                raise ValueError(f"{who} x-coordinate {point[0]} is outside boundary x-range [{x_min}, {x_max}]")
            if not (y_min - eps <= point[1] <= y_max + eps):
                raise ValueError(f"{who} y-coordinate {point[1]} is outside boundary y-range [{y_min}, {y_max}]")
        if n_samples <= 0:
            raise ValueError(f"n_samples must be positive, got {n_samples}")
        if k_nearest <= 0:
            raise ValueError(f"k_nearest must be positive, got {k_nearest}")
        if connection_radius is not None and connection_radius <= 0:
            raise ValueError(f"connection_radius must be positive, got {connection_radius}")
        if max_iter <= 0:
            raise ValueError(f"max_iter must be positive, got {max_iter}")
        if seed is None:
            seed = int(np.random.randint(0, 2 ** 63 - 1, dtype=np.int64))   # (ONE draw of numpy's global stream: np.random.seed(k) repeats it)
        seed = int(seed) & _MASK64
        max_path, max_degree = 256, 32
        while True:
            out = prm_plan_batch(np.float64([list(start)[:2]]), np.float64([list(target)[:2]]), np.float64([list(boundary)]), grid[None],
                                 np.array([seed], np.uint64), None, n_samples, k_nearest, connection_radius, max_degree, max_path=max_path,
                                 device_id=device_id)
            status, length = int(out.status[0]), int(out.path_len[0])
            if status == PRM_OVERFLOW and max_degree < PRM_PLAN_MAX_DEGREE:
                max_degree *= 2   # (the same seed: the same roadmap with more room)
            elif status == PRM_TRUNCATED:
                max_path = length   # (a path longer than the first buffer: once more with its length)
            else:
                break
        if status == PRM_OVERFLOW:
            raise RuntimeError(f"PRM outgrew the device's caps: a node has more than {max_degree} neighbours within {connection_radius}; "
                               "the roadmap was not finished, which is not the same as no path")
        if status == PRM_INVALID:
            raise ValueError(f"start {list(start)}, target {list(target)} or boundary {list(boundary)} is not finite, or the grid is empty")
        nodes, edges = out.roadmap(0)
        if max_iter < 2 * len(edges) + 1:
            raise ValueError(f"max_iter = {max_iter} is below 2 * n_edges + 1 = {2 * len(edges) + 1}, the most the reference's search can "
                             "pop on this roadmap: a binding max_iter is not modelled")
        path = [[float(v) for v in p] for p in out.path[0, :length].cpu().numpy()] if status == PRM_FOUND else []
        return path, (nodes, edges)
