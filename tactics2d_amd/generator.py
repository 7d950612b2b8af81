"""Batched mirror of `tactics2d.map.generator.ParkingLotGenerator` (scope row f4): the rejection
sampler of map/generator/generate_parking_lot.py:239-444 run for many scenes at once on the device.

    gen = ParkingLotGenerator(vehicle_size=(4.284, 1.81), type_proportion=0.5)
    scenes = gen.generate(n_env=4096, seed=7)          # one HIP launch, one lane per scene
    scenes.scene().load(pool)                          # static geometry, target, boundary, start pose

The reference's `generate(map_)` fills a Map with obstacle Areas and returns (start_state, target_area,
target_heading) for ONE scene from numpy's global random stream; here scene e of a batch draws from the
counter stream (seed, first_env + e) -- the same scenes whatever the batch split or the number of ranks.
Parity with the reference is UNPINNED (see include/t2d.h: t2d_generate_parking); the kernel is pinned bit
for bit to its CPU restatement (oracle t2do_generate_parking).  There is no CPU fallback in this module.
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi
from . import layout as L
from .participant import VEHICLE_TEMPLATE, vehicle_model
from .scenarios import Scene

MAX_QUADS = 12
BAY, UNVERIFIED, START_UNVERIFIED, NONCONVEX, OVERFLOW, START_FLIPPED, TARGET_FLIPPED = 1, 2, 4, 8, 16, 32, 64


@dataclass
class ParkingScenes:
    """What `generate` returns for a batch (host arrays).  `start` / `target_heading` keep the reference's
    un-wrapped headings (+pi when the start pose was flipped, generate_parking_lot.py:409-419)."""
    quads: np.ndarray           # (n, 12, 4, 2) f32 obstacle quads in Map.areas order
    quad_id: np.ndarray         # (n, 12) reference ids, -1 = unused
    n_quads: np.ndarray         # (n,)
    start: np.ndarray           # (n, 3) f64 x, y, heading
    target: np.ndarray          # (n, 4, 2) f32
    target_heading: np.ndarray  # (n,) f64
    boundary: np.ndarray        # (n, 4) f32 xmin, xmax, ymin, ymax
    info: np.ndarray            # (n,) u32 flag bits | obstacle attempts << 8 | start attempts << 16
    vehicle_size: tuple

    @property
    def n_env(self):
        return len(self.n_quads)

    @property
    def mode(self):
        return np.where(self.info & BAY, "bay", "parallel")

    def static_csr(self):
        """(env_poly_offsets, poly_vert_offsets, verts_xy) for t2d_set_static_geometry."""
        n = self.n_quads.astype(np.int64)
        eo = np.concatenate([[0], np.cumsum(n)]).astype(np.int32)
        keep = np.arange(MAX_QUADS)[None, :] < n[:, None]
        xy = self.quads[keep].reshape(-1, 2)
        vo = (4 * np.arange(int(eo[-1]) + 1)).astype(np.int32)
        return eo, vo, np.ascontiguousarray(xy, np.float32)

    def scene(self, agent="medium_car", max_step=20000):
        """A one-ego-per-env Scene with the ParkingEnv agent (envs/parking.py:318-327: SingleTrackKinematics,
        speed +-0.5, accel +-2, steer +-0.524) at the generated start poses."""
        bad = self.info & (UNVERIFIED | START_UNVERIFIED | NONCONVEX | OVERFLOW)
        if bad.any():
            raise _ffi.GeometryError(f"{int((bad != 0).sum())} generated scenes are flagged (info bits "
                                     f"{int(np.bitwise_or.reduce(bad)):#x}); regenerate them with another seed")
        ego = vehicle_model(agent, "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0),
                            steer_range=(-0.524, 0.524))
        Ln, W = VEHICLE_TEMPLATE[agent][:2]
        rows = ego.param_row(L.SHAPE_OBB, Ln, W)[None]
        n = self.n_env
        return Scene("parking_generated", n, 1, rows, [agent + ":parking"], np.float32(self.start[:, 0]),
                     np.float32(self.start[:, 1]), np.float32(self.start[:, 2]), np.zeros(n, np.float32),
                     np.zeros(n, np.uint8), np.ones(n, np.uint8), static=self.static_csr(),
                     boundary=np.ascontiguousarray(self.boundary, np.float32),
                     status=dict(max_step=max_step, check_dynamic=0, check_off_lane=0, check_arrival=1,
                                 check_no_action=1, no_action_max_step=100, shaped_reward=1),
                     target=np.ascontiguousarray(self.target, np.float32),
                     target_heading=np.float32(self.target_heading))


class ParkingLotGenerator:
    """`ParkingLotGenerator(vehicle_size=(5.3, 2.5), type_proportion=0.5)` (generate_parking_lot.py:42-58):
    an invalid vehicle size falls back to the default, the proportion is clipped to [0, 1]."""
    _vehicle_size = (5.3, 2.5)

    def __init__(self, vehicle_size=(5.3, 2.5), type_proportion=0.5, device=0):
        if vehicle_size[0] < vehicle_size[1] or vehicle_size[0] <= 0 or vehicle_size[1] <= 0:
            self.vehicle_size = self._vehicle_size
        else:
            self.vehicle_size = (float(vehicle_size[0]), float(vehicle_size[1]))
        self.type_proportion = float(np.clip(type_proportion, 0, 1))
        self.device = int(device)

    def generate(self, n_env, seed, first_env=0):
        n_env = int(n_env)
        out = ParkingScenes(np.zeros((n_env, MAX_QUADS, 4, 2), np.float32), np.zeros((n_env, MAX_QUADS), np.int32),
                            np.zeros(n_env, np.int32), np.zeros((n_env, 3)), np.zeros((n_env, 4, 2), np.float32),
                            np.zeros(n_env), np.zeros((n_env, 4), np.float32), np.zeros(n_env, np.uint32),
                            self.vehicle_size)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        _ffi.check(_ffi.lib().t2d_generate_parking(
            self.device, int(seed) & (2**64 - 1), int(first_env), n_env, self.type_proportion, self.vehicle_size[0],
            self.vehicle_size[1], ptr(out.quads), ptr(out.quad_id), ptr(out.n_quads), ptr(out.start), ptr(out.target),
            ptr(out.target_heading), ptr(out.boundary), ptr(out.info)))
        return out


# ------------------------------------------------------------------------------------------------------- racing tracks
@dataclass
class RacingTrack:
    """One generated track.  tiles float64 [n_tile, 4, 2]: tile i's ring in the order of Lane.geometry (left side, then the
    right side reversed: left[i], left[i + 1], right[i + 1], right[i]); tile i's successor is (i + 1) % n_tile.
    start_line float64 [2, 2] = tile 0's ends, end_line = its starts, center_line float64 [m, 2]; start_point the
    customs["start_state"] location; n_checkpoint the number of turns."""
    tiles: np.ndarray
    start_line: np.ndarray
    end_line: np.ndarray
    center_line: np.ndarray
    start_point: np.ndarray
    n_checkpoint: int

    @property
    def n_tile(self):
        return len(self.tiles)

    def start_pose(self, length=VEHICLE_TEMPLATE["medium_car"][0]):
        """_reset_agent (envs/racing.py:314-326): (x, y, heading) of the car, its nose on the start line"""
        vec = self.start_line[1] - self.start_line[0]
        heading = np.arctan2(vec[0], -vec[1])
        loc = np.mean(self.start_line, axis=0)
        loc -= length / 2 / np.linalg.norm(vec) * np.array([-vec[1], vec[0]])
        return float(loc[0]), float(loc[1]), float(heading)


def _circle_radius(p1, p2, p3):
    """radius of the circle through three points, by the perpendicular bisectors (geometry/cpp_geometry/src/circle.cpp:3-33)"""
    a = p1[0] - p2[0]; b = p1[1] - p2[1]; c = p1[0] - p3[0]; d = p1[1] - p3[1]
    e = (p1[0] * p1[0] - p2[0] * p2[0] + p1[1] * p1[1] - p2[1] * p2[1]) / 2.0
    f = (p1[0] * p1[0] - p3[0] * p3[0] + p1[1] * p1[1] - p3[1] * p3[1]) / 2.0
    denom = a * d - b * c
    if abs(denom) < 1e-10:
        raise RuntimeError("Cannot define a unique circle: points are collinear")
    cx = (e * d - b * f) / denom
    cy = (a * f - e * c) / denom
    dx = p1[0] - cx; dy = p1[1] - cy
    return np.sqrt(dx * dx + dy * dy)


def _bezier2(p0, p1, p2, n):
    """n points of the order-2 Bezier curve, Bernstein form, accumulated control point by control point
    (interpolator/cpp_interpolator/src/bezier.cpp): float64 [n, 2]"""
    t = np.arange(n) * (1.0 / (n - 1))
    u = 1.0 - t
    w0 = 1.0 * (u * u) * 1.0
    w1 = 2.0 * u * t
    w2 = 1.0 * 1.0 * (t * t)
    out = np.zeros((n, 2))
    for w, p in ((w0, p0), (w1, p1), (w2, p2)):
        out[:, 0] += w * p[0]
        out[:, 1] += w * p[1]
    return out


class _Polyline:
    """LineString.length / interpolate of the reference's shapely calls: segment lengths sqrt(dx dx + dy dy) summed in order;
    the point at distance d lies on the first segment whose end is beyond d, at p0 + frac (p1 - p0) with
    frac = (d - length before) / segment length; d <= 0 gives the first point, d beyond the end the last."""

    def __init__(self, pts):
        self.p = np.asarray(pts, np.float64)
        d = np.diff(self.p, axis=0)
        self.seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1])
        total, before = 0.0, []
        for s in self.seg.tolist():          # (a running sum in segment order, not a pairwise one)
            before.append(total)
            total += s
        self.before, self.length = before, total
        self._k = 0

    def interpolate(self, dist):
        if dist <= 0.0:
            return self.p[0].copy()
        k = self._k if self.before[self._k] <= dist else 0      # (distances are asked for in increasing order)
        while k < len(self.seg):
            if self.before[k] + self.seg[k] > dist:
                self._k = k
                frac = (dist - self.before[k]) / self.seg[k]
                p0, p1 = self.p[k], self.p[k + 1]
                return np.array([p0[0] + frac * (p1[0] - p0[0]), p0[1] + frac * (p1[1] - p0[1])])
            k += 1
        return self.p[-1].copy()


class RacingTrackGenerator:
    """Host-side restatement of `tactics2d.map.generator.RacingTrackGenerator` (map/generator/generate_racing_track.py):
    checkpoints on a circle of radius 800 m with their rejection loop, the three-point circle, order-2 Bezier turns of 50
    points, the start point, the centre line and the tiles of `_get_tiles`.  It consumes numpy's GLOBAL random stream draw
    for draw, as the reference does: `np.random.seed(s)` before `generate()` gives the track the reference generates after the
    same seed (tests/golden/racing_tracks.npz).  Set-up code: there is no kernel here."""

    _n_checkpoint = (10, 20)
    _track_width = 5
    _track_rad = 800
    _curve_rad = (50, 150)
    _tile_length = 10

    def __init__(self, bezier_order=2, bezier_interpolation=50, max_tiles=L.MAX_TRACK_TILES):
        if bezier_order != 2:
            raise NotImplementedError("only the order-2 curves RacingEnv uses are restated")
        self._bezier_interpolation = int(bezier_interpolation)
        self.max_tiles = int(max_tiles)

    def _get_checkpoints(self, rnd=np.random):
        n = rnd.randint(*self._n_checkpoint)
        noise = rnd.uniform(0, 2 * np.pi / n, n)
        alpha = 2 * np.pi * np.arange(n) / n + noise
        rad = rnd.uniform(self._track_rad / 5, self._track_rad, n)
        cp = np.array([rad * np.cos(alpha), rad * np.sin(alpha)])
        control, success = [], False
        for _ in range(100):
            control, glued = [], 0
            for i in range(n):
                nxt = 0 if i + 1 == n else i + 1
                pt1, pt2, pt3 = cp[:, i - 1], cp[:, i], cp[:, nxt]
                t1 = rnd.uniform(low=1 / 4, high=1 / 2)
                t2 = rnd.uniform(low=1 / 4, high=1 / 2)
                a = (1 - t1) * pt2 + t1 * pt1
                b = (1 - t2) * pt2 + t2 * pt3
                radius = _circle_radius(a, pt2, b)
                if radius < self._curve_rad[0] or radius > self._curve_rad[1]:
                    # too sharp: push the next checkpoint away from this one's radius and on; too wide: the other way
                    sign = 1.0 if radius < self._curve_rad[0] else -1.0
                    step = rnd.uniform(0.0, 10.0)
                    rad[nxt] += sign * step if rad[i] > rad[nxt] else -sign * step
                    alpha[nxt] += sign * rnd.uniform(0.0, 0.05)
                    cp[:, nxt] = [rad[nxt] * np.cos(alpha[nxt]), rad[nxt] * np.sin(alpha[nxt])]
                else:
                    glued += 1
                    control.append([a, b])
            if glued == n:
                success = True
                break
        success = success and all(alpha == sorted(alpha))
        return cp, control, success

    def _get_start_point(self, n, control):
        # (the reference measures each straight by np.linalg.norm of the 2 x 2 array of its two end points -- the Frobenius
        # norm of their coordinates, not their distance; kept, since the choice of the start straight follows from it)
        lens = [np.linalg.norm([control[i][0], control[i - 1][1]]) for i in range(n)]
        order = sorted(range(n), key=lambda i: lens[i], reverse=True)
        start_id = None
        for i in range(3):
            start_id = order[i]
            if lens[start_id] < 200:
                break
        line = _Polyline([control[start_id][0], control[start_id - 1][1]])
        return line.interpolate(lens[start_id] / 3), start_id

    def _get_center_line(self, start_point, start_id, cp, control):
        pts = [start_point[None]]
        for i in range(cp.shape[1]):
            k = start_id - i - 1
            pts.append(_bezier2(control[k][1], cp[:, k], control[k][0], self._bezier_interpolation))
        pts.append(start_point[None])
        return np.concatenate(pts)

    def _get_tiles(self, n_tile, line):
        c = np.array([line.interpolate(self._tile_length * i) for i in range(n_tile)])
        prev = np.roll(c, 1, axis=0)
        xd, yd = c[:, 0] - prev[:, 0], c[:, 1] - prev[:, 1]
        k = np.array([self._track_width / 2 / np.linalg.norm([a, b]) for a, b in zip(xd.tolist(), yd.tolist())])
        left = np.stack([c[:, 0] - k * yd, c[:, 1] + k * xd], 1)
        right = np.stack([c[:, 0] + k * yd, c[:, 1] - k * xd], 1)
        ln, rn = np.roll(left, -1, axis=0), np.roll(right, -1, axis=0)
        return np.stack([left, ln, rn, right], 1)

    def generate(self, rng=None):
        """One track -> RacingTrack (fp64, the reference's coordinates).  rng: the draw source, an object with numpy's
        `randint(low, high)` and `uniform(low, high, size=None)`; None is numpy's global random stream."""
        rnd = np.random if rng is None else rng
        success = False
        while not success:
            cp, control, success = self._get_checkpoints(rnd)
        n = cp.shape[1]
        start_point, start_id = self._get_start_point(n, control)
        center = self._get_center_line(start_point, start_id, cp, control)
        line = _Polyline(center)
        n_tile = int(np.ceil(line.length / self._tile_length))
        if n_tile > self.max_tiles:
            raise ValueError(f"the generated track has {n_tile} tiles, more than the {self.max_tiles} a track may hold "
                             "(T2D_MAX_TRACK_TILES)")
        tiles = self._get_tiles(n_tile, line)
        return RacingTrack(tiles, np.array([tiles[0, 1], tiles[0, 2]]), np.array([tiles[0, 0], tiles[0, 3]]), center,
                           start_point, n)

    def generate_batch(self, n_tracks, seed, first_track=0, device=0):
        """n_tracks tracks from the DEVICE generator (t2d_generate_tracks, one launch): track t of the batch is the track of the
        counter stream (seed, first_track + t) -- the same track whatever the batch split -- already shifted to the centre of
        its bounding box and rounded to fp32, as VecRacingEnv installs it.  The random stream is the build's own (include/
        t2d.h), not numpy's: these are not the tracks `generate()` makes.  -> TrackBatch (host arrays)."""
        import torch
        n = int(n_tracks)
        if n < 0 or int(first_track) < 0:
            raise ValueError("n_tracks and first_track must be >= 0")
        if self.max_tiles != L.MAX_TRACK_TILES:
            raise ValueError("the device generator writes tracks of capacity T2D_MAX_TRACK_TILES")
        dev = f"cuda:{int(device)}"
        z = lambda shape, dt: torch.zeros(shape, dtype=dt, device=dev)
        tiles, n_tile, n_cp, attempt = z((n, self.max_tiles, 4, 2), torch.float32), z(n, torch.int32), z(n, torch.int32), z(n, torch.int32)
        pose, line, bound, flags = z((n, 3), torch.float64), z((n, 2, 2), torch.float32), z((n, 4), torch.float32), z(n, torch.int32)
        _ffi.check(_ffi.lib().t2d_generate_tracks(int(device), n, int(seed) & (2**64 - 1), int(first_track),
                                                  VEHICLE_TEMPLATE["medium_car"][0], tiles.data_ptr(), n_tile.data_ptr(),
                                                  n_cp.data_ptr(), attempt.data_ptr(), pose.data_ptr(), line.data_ptr(),
                                                  bound.data_ptr(), flags.data_ptr(), torch.cuda.current_stream(dev).cuda_stream))
        torch.cuda.current_stream(dev).synchronize()
        nt = n_tile.cpu().numpy()
        fl = flags.cpu().numpy().view(np.uint32)
        keep = np.where(fl == 0, nt, 0)
        host = [tiles[t, :int(keep[t])].cpu().numpy() for t in range(n)]
        return TrackBatch(host, nt, n_cp.cpu().numpy(), attempt.cpu().numpy(), pose.cpu().numpy(), line.cpu().numpy(),
                          bound.cpu().numpy(), fl)


TRACK_CAPPED, TRACK_OVERFLOW = 1, 2     # T2D_TRACKGEN_CAPPED / T2D_TRACKGEN_OVERFLOW


@dataclass
class TrackBatch:
    """What `RacingTrackGenerator.generate_batch` returns.  A flagged track (flags != 0) has no tiles."""
    tiles: list                 # n arrays float32 [n_tile, 4, 2]
    n_tile: np.ndarray          # (n,) int32
    n_checkpoint: np.ndarray    # (n,) int32
    attempt: np.ndarray         # (n,) int32 index of the accepted attempt, -1 when the cap was hit
    start_pose: np.ndarray      # (n, 3) f64 x, y, heading in [0, 2 pi)
    start_line: np.ndarray      # (n, 2, 2) f32
    boundary: np.ndarray        # (n, 4) f32 xmin, xmax, ymin, ymax
    flags: np.ndarray           # (n,) uint32 TRACK_CAPPED | TRACK_OVERFLOW


class GridMapGenerator:
    """Host restatement of map/generator/generate_grid_map.py: GridMapGenerator -- a random cost grid with obstacles (+inf), a
    start and a goal cell, drawn from NUMPY'S GLOBAL STREAM draw for draw (random_seed reseeds it in the constructor, as the
    reference does): the same seed gives the reference's grid, start and goal bit for bit.  Not a hot path; the grids go to the
    device through tactics2d_amd.search."""

    def __init__(self, size, min_cost=0, max_cost=5, obstacle_proportion=0.1, random_seed=None):
        self.size = size
        self.min_cost = min_cost
        self.max_cost = max_cost
        self.obstacle_proportion = obstacle_proportion
        if random_seed is not None:
            np.random.seed(random_seed)

    def generate(self):
        """(grid float64 [H, W], start (row, col), goal (row, col)); start and goal are free cells and differ"""
        h, w = self.size
        grid = np.random.randint(self.min_cost, self.max_cost + 1, size=self.size).astype(float)
        obstacles = np.random.choice(h * w, int(h * w * self.obstacle_proportion), replace=False)
        grid[obstacles // w, obstacles % w] = np.inf
        while True:
            start = (np.random.randint(0, h), np.random.randint(0, w))
            if grid[start] != np.inf:
                break
        while True:
            goal = (np.random.randint(0, h), np.random.randint(0, w))
            if grid[goal] != np.inf and goal != start:
                break
        return grid, start, goal

    def generate_batch(self, n):
        """n consecutive generate() calls, stacked: grids float64 [n, H, W], starts int32 [n, 2], goals int32 [n, 2] (row, col)"""
        out = [self.generate() for _ in range(int(n))]
        h, w = self.size
        return (np.stack([g for g, _, _ in out]) if out else np.zeros((0, h, w)),
                np.asarray([s for _, s, _ in out], np.int32).reshape(-1, 2), np.asarray([t for _, _, t in out], np.int32).reshape(-1, 2))
