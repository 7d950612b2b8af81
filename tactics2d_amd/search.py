"""Grid shortest paths on the device: the reference's `tactics2d.search.Dijkstra` over the graph of
`tactics2d.search.grid_to_csr`, for n weighted obstacle grids in ONE launch of t2d_grid_dijkstra (include/t2d.h).

    field = cost_to_go(weight_grids, sources)                       # float64 [n, H, W] on the device: reward shaping, heuristics
    out = Dijkstra.plan_batch(weight_grids, sources, targets)       # out.field, out.path, out.path_len, out.status: device tensors
    xy = Dijkstra.plan(start, target, boundary, weight_grid, grid_resolution)   # one query with the reference's signature

The device takes the GRID: `grid_to_csr` is not rebuilt, its edge weights are evaluated in flight.  The field equals the
reference's g_score bit for bit and the path is the reference's path (an edge of weight exactly 0 is no edge there and here).
A* (`a_star.py`), D*, the sampling planners and hybrid A* are not part of this package.  There is no CPU fallback.
"""
import math

import numpy as np

from . import _ffi
from . import layout as L
from .interpolator import _is_tensor, _stream_of

SQRT2 = 1.4142135623730951   # grid_to_csr's default diagonal_cost_multiplier
FOUND, NO_PATH, TRUNCATED, INVALID, FIELD_ONLY = L.GRID_FOUND, L.GRID_NO_PATH, L.GRID_TRUNCATED, L.GRID_INVALID, L.GRID_FIELD_ONLY
MAX_CELLS = L.GRID_MAX_CELLS


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
    if not _is_tensor(weight_grids):
        weight_grids = np.asarray(weight_grids, np.float64)
    shape = tuple(weight_grids.shape)
    if len(shape) == 2:
        shape = (1,) + shape
    if len(shape) != 3:
        raise ValueError(f"weight_grids must have shape (n, H, W) or (H, W), got {tuple(weight_grids.shape)}")
    if connectivity not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity}")
    mult = float(diagonal_cost_multiplier)
    if not math.isfinite(mult) or mult < 0:
        raise ValueError(f"diagonal_cost_multiplier must be finite and not negative, got {diagonal_cost_multiplier}")
    n, h_max, w_max = shape
    stride = h_max * w_max
    if stride < 1:
        raise ValueError(f"weight_grids must have at least one cell, got shape {shape}")
    hw_host = None if _is_tensor(hw) else (np.tile(np.int32([h_max, w_max]), (n, 1)) if hw is None else np.asarray(hw, np.int32).reshape(n, 2))
    if not _is_tensor(sources):
        sources = _cells(sources, n, hw_host)
    if targets is not None and not _is_tensor(targets):
        targets = _cells(targets, n, hw_host)
    max_path = (stride if targets is not None else 0) if max_path is None else int(max_path)
    if max_path < 0:
        raise ValueError(f"max_path must not be negative, got {max_path}")
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        if _is_tensor(weight_grids):
            w = weight_grids.to(dev, torch.float64).reshape(n, stride).contiguous()
        else:
            w = torch.as_tensor(np.ascontiguousarray(weight_grids, np.float64).reshape(n, stride)).to(dev)
        hw_t = _i32(hw_host if hw_host is not None else hw, dev, (n, 2))
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
        start_x = int(round((start[0] - x_min) / grid_resolution))
        start_y = int(round((start[1] - y_min) / grid_resolution))
        target_x = int(round((target[0] - x_min) / grid_resolution))
        target_y = int(round((target[1] - y_min) / grid_resolution))
        start_x = max(0, min(start_x, width - 1))
        start_y = max(0, min(start_y, height - 1))
        target_x = max(0, min(target_x, width - 1))
        target_y = max(0, min(target_y, height - 1))
        start_idx = start_y * width + start_x
        target_idx = target_y * width + target_x
        if not (0 <= start_idx < N):
            raise ValueError(f"start_idx {start_idx} out of bounds [0, {N})")
        if not (0 <= target_idx < N):
            raise ValueError(f"target_idx {target_idx} out of bounds [0, {N})")
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
