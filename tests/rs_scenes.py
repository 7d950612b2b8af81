"""Inputs shared by tests/test_rs.py and tests/test_gpu_rs.py (TEST INFRASTRUCTURE): the fixture unpacked, and the seeded planner
scenes -- egos, targets and synthetic scans -- with the specification's plan for each, computed once per session."""
import functools

import numpy as np

import helpers as H
import rs_ref as R

# a medium_car (participant_template.py): length, width, wheel_base, rear_overhang; max_steer 0.524 (vehicle.py:111)
CAR = dict(length=4.284, width=1.799, wheel_base=2.637, rear_overhang=0.767, steer_hi=0.524)
LIDAR_RANGE = 20.0
PARAMS = R.params_from_vehicle(lidar_range=LIDAR_RANGE, **CAR)
KINDS = ("open", "ring", "wall", "box")
SEED = 7


@functools.lru_cache(None)
def fixture():
    """reeds_shepp.npz with the packed parts unpacked: valid bool [N, 48], seg [N, 48, 5], length [N, 48] (+inf for None)"""
    g = H.load_npz("reeds_shepp.npz")
    n = len(g["valid"])
    valid = ((g["valid"][:, None] >> np.arange(48, dtype=np.uint64)) & np.uint64(1)).astype(bool)
    length = np.full((n, 48), np.inf)
    length[valid] = g["length"]
    seg = np.zeros((n, 48, 5))
    per = np.broadcast_to(g["n_seg"], (n, 48))[valid]
    rows = np.repeat(np.arange(len(per)), per)
    cols = np.concatenate([np.arange(k) for k in per])
    flat = np.zeros((len(per), 5))
    flat[rows, cols] = g["seg"]
    seg[valid] = flat
    g.update(valid_mask=g["valid"], valid=valid, seg=seg, length=length, start=g["start"].astype(np.float64),
             goal=g["goal"].astype(np.float64), radius_of=g["radius"][g["query_radius"]])
    return g


def _ray_cast(n_beams, segments):
    """distance from the origin along beam k (angle k * 2 pi / n_beams) to the nearest of `segments` [[x1, y1, x2, y2]]; +inf none"""
    th = R.beam_angles(n_beams)
    c, s = np.cos(th)[:, None], np.sin(th)[:, None]
    seg = np.asarray(segments, float)
    px, py, dx, dy = seg[:, 0], seg[:, 1], seg[:, 2] - seg[:, 0], seg[:, 3] - seg[:, 1]
    det = dx[None] * s - dy[None] * c
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (dx[None] * py[None] - dy[None] * px[None]) / det     # along the beam
        u = (c * py[None] - s * px[None]) / det                   # along the segment
    t = np.where((det != 0) & (t > 0) & (u >= 0) & (u <= 1), t, np.inf)
    return t.min(1)


@functools.lru_cache(None)
def planner_case(n_env, n_beams, seed=SEED):
    """egos and targets with the goal 3 - 18 m away, and one synthetic scan per env (kind = env % 4): an open field, a ring at a
    seeded radius, a wall across the shortest candidate's path, a closed box around the ego"""
    rng = np.random.default_rng(seed)
    p = PARAMS
    ego = np.empty((n_env, 3), np.float32)
    ego[:, :2] = rng.uniform(-30, 30, (n_env, 2))
    ego[:, 2] = rng.uniform(-np.pi, np.pi, n_env)
    dist, bearing = rng.uniform(3, 18, n_env), rng.uniform(-np.pi, np.pi, n_env)
    th = rng.uniform(-np.pi, np.pi, n_env)
    centre = ego[:, :2].astype(float) + dist[:, None] * np.stack([np.cos(bearing), np.sin(bearing)], 1)
    car = np.array([[2.65, -1.25], [2.65, 1.25], [-2.65, 1.25], [-2.65, -1.25]])
    rot = np.stack([np.stack([np.cos(th), -np.sin(th)], 1), np.stack([np.sin(th), np.cos(th)], 1)], 1)   # [n, 2, 2]
    target = (np.einsum("nij,kj->nki", rot, car) + centre[:, None]).astype(np.float32)
    ring_r, box_h = rng.uniform(4, 12, n_env), rng.uniform(3.2, 4.5, n_env)
    scan = np.full((n_env, n_beams), np.inf, np.float32)
    ang = R.beam_angles(n_beams)
    for e in range(n_env):
        kind = KINDS[e % 4]
        if kind == "ring":
            scan[e] = ring_r[e]
        elif kind == "box":
            scan[e] = box_h[e] / np.maximum(np.abs(np.cos(ang)), np.abs(np.sin(ang)))
        elif kind == "wall":
            free = R.plan(p, LIDAR_RANGE, ego[e], target[e], th[e], scan[e])
            if free.status != R.FOUND:
                continue
            poses = R.sample_path(p, free.slot, free.distance / p.radius)
            x, y, yaw = poses[len(poses) // 2]
            nx, ny = -np.sin(yaw), np.cos(yaw)
            wall = [x - 2.5 * nx - p.center_shift, y - 2.5 * ny, x + 2.5 * nx - p.center_shift, y + 2.5 * ny]
            scan[e] = _ray_cast(n_beams, [wall])
    return dict(params=p, ego=ego, target=target, target_heading=th, scan=scan, kind=np.arange(n_env) % 4)


@functools.lru_cache(None)
def spec_plans(n_env, n_beams, seed=SEED, sample_step=None):
    """[(Plan, robust)] of the specification for planner_case(n_env, n_beams, seed); sample_step: another one than the tutorial's"""
    c = planner_case(n_env, n_beams, seed)
    p = c["params"] if sample_step is None else c["params"]._replace(sample_step=sample_step)
    return [R.plan_with_margin(p, LIDAR_RANGE, c["ego"][e], c["target"][e], c["target_heading"][e], c["scan"][e])
            for e in range(n_env)]


def categories(plans):
    """counts of what the issue wants to see in the spec's answers: FOUND first-ranked, FOUND later, NONE_FREE, FAR"""
    st = np.array([p.status for p, _ in plans])
    nv = np.array([p.n_visited for p, _ in plans])
    return dict(found_first=int(((st == R.FOUND) & (nv == 1)).sum()), found_later=int(((st == R.FOUND) & (nv > 1)).sum()),
                none_free=int((st == R.NONE_FREE).sum()), far=int((st == R.FAR).sum()))
