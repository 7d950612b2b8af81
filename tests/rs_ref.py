"""The specification of the Reeds-Shepp primitive and of the parking planner, in numpy (TEST INFRASTRUCTURE).

What it restates, and from where:
  * the 48 candidate curves: ReedsShepp.get_all_path and the five family methods of tactics2d/interpolator/reeds_shepp.py
    (:158-527), ReedsSheppPath.__init__ (:19-44) -- vectorised over the queries, with a slot table of its own (FAMILIES) that
    tests/test_rs.py holds against the fixture tests/golden/reeds_shepp.npz (made by running the reference);
  * the planner: docs/tutorial/train_parking_demo.ipynb cell 9 -- RSPlanner.__init__ (:7-21), init_vehicle_base (:23-44),
    get_rs_path (:52-121), construct_obstacles (:155-193), is_traj_valid (:195-267);
  * the build's own rules: sampling (`sample_path`), the pose cap, the goal box in the chain's frame, fp64
    arithmetic on the fp32 scan, NaN -> UNCHECKED.
`Params` has the fields of t2d_rs_params (include/t2d.h) in the same order.  plan() also reports the sorted candidate lengths;
plan_with_margin() says whether the decision is the same with every scan value moved by +1e-6 m and by -1e-6 m.
"""
import collections

import numpy as np

PI, PIO2 = np.pi, np.pi / 2
NO_TARGET, FAR, FOUND, NONE_FREE, UNCHECKED = range(5)
MAX_POSES = 1024
SCAN_SHIFT = 1e-6

Params = collections.namedtuple("Params", "radius center_shift half_length half_width distance_tolerance threshold_distance "
                                          "sample_step length_ratio edge_tolerance")

# (formula, LRL sign triple or None, first image, letters of image 0, columns of the matrix as (source, factor) with source
#  0 t, 1 u, 2 v, 3 the constant row): four slots each -- image k, k + 1 (time flip: the matrix negated), k + 2 (reflection: L
# and R swapped), k + 3 (both)
H = PIO2
FAMILIES = (
    ("LSL", None, 0, "LSL", ((0, 1), (1, 1), (2, 1))),
    ("LSR", None, 0, "LSR", ((0, 1), (1, 1), (2, 1))),
    ("LRL", (1, -1, 1), 0, "LRL", ((0, 1), (1, -1), (2, 1))),
    ("LRL", (1, -1, -1), 0, "LRL", ((0, 1), (1, -1), (2, -1))),
    ("LRL", (-1, -1, 1), 0, "LRL", ((0, -1), (1, -1), (2, 1))),
    ("LRLR_A", None, 0, "LRLR", ((0, 1), (1, 1), (1, -1), (2, -1))),
    ("LRLR_B", None, 0, "LRLR", ((0, 1), (1, -1), (1, -1), (2, 1))),
    ("LRSL", None, 0, "LRSL", ((0, 1), (3, -H), (1, -1), (2, -1))),
    ("LRSL", None, 4, "LSRL", ((2, -1), (1, -1), (3, -H), (0, 1))),
    ("LRSR", None, 0, "LRSR", ((0, 1), (3, -H), (1, -1), (2, -1))),
    ("LRSR", None, 4, "RSRL", ((2, -1), (1, -1), (3, -H), (0, 1))),
    ("LRSLR", None, 0, "LRSLR", ((0, 1), (3, -H), (1, 1), (3, -H), (2, 1))),
)
CURVE_OF = {"LSL": 0, "LSR": 0, "LRL": 1, "LRLR_A": 2, "LRLR_B": 2, "LRSL": 3, "LRSR": 3, "LRSLR": 4}
SWAP = {"L": "R", "R": "L", "S": "S"}
STEER = {"L": 1, "R": -1, "S": 0}


def slot_table():
    out = []
    for formula, signs, first, word, cols in FAMILIES:
        for k in range(4):
            w = "".join(SWAP[c] for c in word) if k & 2 else word
            f = -1.0 if k & 1 else 1.0
            out.append(dict(formula=formula, signs=signs, image=first + k, word=w, cols=tuple((s, f * c) for s, c in cols),
                            curve_type=CURVE_OF[formula]))
    return out


SLOTS = slot_table()
WORDS = [s["word"] for s in SLOTS]
N_SEG = np.array([len(w) for w in WORDS])
LETTERS = np.zeros((48, 5), np.int8)
SIGNS = np.zeros((48, 5), np.int8)
for _k, _s in enumerate(SLOTS):
    LETTERS[_k, :N_SEG[_k]] = [STEER[c] for c in _s["word"]]
    SIGNS[_k, :N_SEG[_k]] = [np.sign(c) for _, c in _s["cols"]]


def mod_pi(theta):   # _M :164-173
    phi = np.mod(theta, 2 * PI)
    phi = np.where(phi > PI, phi - 2 * PI, phi)
    return np.where(phi < -PI, phi + 2 * PI, phi)


def polar(x, y):   # _R :158-162
    return np.sqrt(x * x + y * y), np.arctan2(y, x)


def tau_omega(u, v, xi, eta, phi):   # :175-187
    delta = mod_pi(u - v)
    A = np.sin(u) - np.sin(delta)
    B = np.cos(u) - np.cos(delta) - 1
    t1 = np.arctan2(eta * A - xi * B, xi * A + eta * B)
    t2 = 2 * (np.cos(delta) - np.cos(v) - np.cos(u)) + 3
    tau = np.where(t2 < 0, mod_pi(t1 + PI), mod_pi(t1))
    return tau, mod_pi(tau - u + v - phi)


def formula(name, signs, x, y, phi):
    """(ok, t, u, v) of one base formula for arrays of goals; ok False where the reference returns None"""
    s, c = np.sin(phi), np.cos(phi)
    with np.errstate(invalid="ignore", divide="ignore"):
        if name == "LSL":   # :208-219
            u, t = polar(x - s, y - 1 + c)
            v = mod_pi(phi - t)
            return ~(t < 0) & ~(v < 0), t, u, v
        if name == "LSR":   # :221-236
            u1, t1 = polar(x + s, y - 1 - c)
            ok = ~(u1 * u1 < 4)
            u = np.sqrt(np.where(ok, u1 * u1 - 4, 0.0))
            t = mod_pi(t1 + np.arctan2(2.0, u))
            v = mod_pi(t - phi)
            return ok & ~((t < 0) | (v < 0)), t, u, v
        if name == "LRL":   # :260-278
            u1, theta = polar(x - s, y - 1 + c)
            ok = ~(u1 > 4)
            A = PI - np.arcsin(np.where(ok, u1 / 4, 0.0))
            t = mod_pi(theta + A)
            u = mod_pi(2 * A)
            v = mod_pi(phi - t + u)
            return ok & ~((t * signs[0] < 0) | (u * signs[1] < 0) | (v * signs[2] < 0)), t, u, v
        if name == "LRLR_A":   # :315-330
            xi, eta = x + s, y - 1 - c
            rho = (2 + np.sqrt(xi * xi + eta * eta)) / 4
            ok = ~((rho > 1) | (rho < 0))
            u = np.arccos(np.where(ok, rho, 1.0))
            t, v = tau_omega(u, -u, xi, eta, phi)
            return ok & ~((t < 0) | (v > 0)), t, u, v
        if name == "LRLR_B":   # :332-350
            xi, eta = x + s, y - 1 - c
            rho = (20 - xi * xi - eta * eta) / 16
            ok = ~((rho > 1) | (rho < 0))
            u = -np.arccos(np.where(ok, rho, 1.0))
            ok &= ~(u < -PIO2)
            t, v = tau_omega(u, u, xi, eta, phi)
            return ok & ~((t < 0) | (v < 0)), t, u, v
        if name == "LRSL":   # :377-394
            rho, theta = polar(x - s, y - 1 + c)
            ok = ~(rho < 2)
            r = np.sqrt(np.where(ok, rho * rho - 4, 0.0))
            u = 2 - r
            t = mod_pi(theta + np.arctan2(r, -2.0))
            v = mod_pi(phi - PIO2 - t)
            return ok & ~((t < 0) | (u > 0) | (v > 0)), t, u, v
        if name == "LRSR":   # :396-412
            xi, eta = x + s, y - 1 - c
            rho, t = polar(-eta, xi)
            ok = ~(rho < 2)
            u = 2 - rho
            v = mod_pi(t + PIO2 - phi)
            return ok & ~((t < 0) | (u > 0) | (v > 0)), t, u, v
        # LRSLR :452-472
        xi, eta = x + s, y - 1 - c
        rho, theta = polar(xi, eta)
        ok = ~(rho < 2)
        t = mod_pi(theta - np.arccos(np.where(ok, -2 / np.where(ok, rho, 2.0), 0.0)))
        ok &= ~(t <= 0)
        u = 4 - (xi + 2 * np.cos(t)) / np.sin(t)
        v = mod_pi(t - phi)
        return ok & ~((u > 0) | (v < 0)), t, u, v


def image(k, x, y, phi):   # the `inputs` lists: _backward :195-198 first, then _reflect :192-193, _time_flip :189-190
    if k & 4:
        x, y = x * np.cos(phi) + y * np.sin(phi), x * np.sin(phi) - y * np.cos(phi)
    if k & 2:
        y, phi = -y, -phi
    if k & 1:
        x, phi = -x, -phi
    return x, y, phi


def candidates(x, y, phi):
    """valid [n, 48], signed segments [n, 48, 5] (signs * segments of ReedsSheppPath :35-42, units of the radius, zero padded),
    total [n, 48] = np.abs(segments).sum()"""
    x, y, phi = (np.atleast_1d(np.asarray(v, float)) for v in (x, y, phi))
    n = x.size
    valid = np.zeros((n, 48), bool)
    seg = np.zeros((n, 48, 5))
    total = np.zeros((n, 48))
    for k, sl in enumerate(SLOTS):
        ok, t, u, v = formula(sl["formula"], sl["signs"], *image(sl["image"], x, y, phi))
        ok = ok & np.isfinite(x) & np.isfinite(y) & np.isfinite(phi)
        src = (t, u, v, np.ones(n))
        tot = np.zeros(n)
        for i, (s, c) in enumerate(sl["cols"]):
            m = np.abs(src[s] * c)
            tot = tot + m
            seg[:, k, i] = np.where(ok, np.sign(c) * m, 0.0)
        valid[:, k] = ok
        total[:, k] = np.where(ok, tot, 0.0)
    return valid, seg, total


def normalise(start, goal, radius):   # get_all_path :513-517
    start, goal = np.atleast_2d(start).astype(float), np.atleast_2d(goal).astype(float)
    radius = np.reshape(radius, -1)
    dx, dy = (goal[:, 0] - start[:, 0]) / radius, (goal[:, 1] - start[:, 1]) / radius
    c, s = np.cos(start[:, 2]), np.sin(start[:, 2])
    return dx * c + dy * s, -dx * s + dy * c, goal[:, 2] - start[:, 2]


def all_paths(start, goal, radius):
    """valid [n, 48], signed segments [n, 48, 5], length [n, 48] in metres (+inf where None)"""
    valid, seg, total = candidates(*normalise(start, goal, radius))
    return valid, seg, np.where(valid, total * np.reshape(radius, (-1, 1)), np.inf)


def shortest_slots(length):
    """per query: get_path's slot (:549-556, the LAST of equal shortest lengths) and the lowest-index shortest (RSPlanner's heap)"""
    length = np.atleast_2d(length)
    best = length.min(1)
    hit = length == best[:, None]
    last = 47 - np.argmax(hit[:, ::-1], 1)
    first = np.argmax(hit, 1)
    none = ~np.isfinite(best)
    return np.where(none, -1, last), np.where(none, -1, first)


def advance(x, y, yaw, steer, d, r):
    """one piece of a word from the pose (x, y, yaw): steer +1 L / -1 R / 0 S, d the signed distance, r the radius"""
    if steer == 0:
        return x + d * np.cos(yaw), y + d * np.sin(yaw), yaw + 0 * d
    yaw1 = yaw + steer * d / r
    return x + steer * r * (np.sin(yaw1) - np.sin(yaw)), y + steer * r * (np.cos(yaw) - np.cos(yaw1)), yaw1


def integrate(slot, seg, r=1.0):
    """end pose of the word of `slot` with the signed segments seg[..., 5] (units of r) from the origin"""
    x = y = yaw = np.zeros(np.shape(seg)[:-1])
    for i in range(N_SEG[slot]):
        x, y, yaw = advance(x, y, yaw, int(LETTERS[slot, i]), seg[..., i] * r, r)
    return x, y, yaw


# ---- the planner ------------------------------------------------------------------------------------------------------------------
def params_from_vehicle(length, width, wheel_base, rear_overhang, steer_hi, steer_ratio=0.98, lidar_range=20.0):
    """RSPlanner.__init__ :7-21"""
    return Params(wheel_base / np.tan(steer_hi * steer_ratio), 0.5 * length - rear_overhang, 0.5 * length, 0.5 * width, 0.05,
                  lidar_range - 5.0, 0.1, 2.0, 1e-4)


def beam_angles(n):
    return np.arange(n) * np.pi / n * 2   # :164


def vehicle_base(n_beams, half_length, half_width):
    """init_vehicle_base :23-44: from the box centre along each beam to the box outline"""
    th = beam_angles(n_beams)
    with np.errstate(divide="ignore"):
        return np.minimum(half_length / np.abs(np.cos(th)), half_width / np.abs(np.sin(th)))


def box_corners(p):
    x0, x1, w = p.center_shift + p.half_length, p.center_shift - p.half_length, p.half_width
    return np.array([[x0, -w], [x0, w], [x1, w], [x1, -w]])


def chain(p, scan, lidar_range, base):
    """construct_obstacles :160-178 up to the edges: x1, y1, x2, y2 [n_beams]; all fp64 on the fp32 values"""
    v = np.clip(np.asarray(scan, np.float32).astype(np.float64), 0.0, lidar_range)
    d = np.maximum(base, v - p.distance_tolerance)
    th = beam_angles(len(v))
    x1, y1 = np.cos(th) * d + p.center_shift, np.sin(th) * d
    return x1, y1, np.roll(x1, -1), np.roll(y1, -1)


def collide_map(p, poses, edges):
    """is_traj_valid :195-260: bool [poses, 4, E].  The verdict of a (box edge, obstacle edge) pair is evaluated only where the
    pose's box and the edge overlap in both coordinate ranges (widened by the tolerance): elsewhere an intersection point
    cannot lie inside both edges' ranges, so the verdict is False either way."""
    x1, y1, x2, y2 = edges
    tol = p.edge_tolerance
    poses = np.atleast_2d(poses)
    cs, sn = np.cos(poses[:, 2])[:, None], np.sin(poses[:, 2])[:, None]
    car = box_corners(p)
    vx = cs * car[:, 0] - sn * car[:, 1] + poses[:, 0, None]   # [P, 4]
    vy = sn * car[:, 0] + cs * car[:, 1] + poses[:, 1, None]
    out = np.zeros((len(poses), 4, len(x1)), bool)
    exlo, exhi, eylo, eyhi = np.minimum(x1, x2) - tol, np.maximum(x1, x2) + tol, np.minimum(y1, y2) - tol, np.maximum(y1, y2) + tol
    near = ~((exlo[None] > vx.max(1)[:, None] + tol) | (vx.min(1)[:, None] - tol > exhi[None]) |
             (eylo[None] > vy.max(1)[:, None] + tol) | (vy.min(1)[:, None] - tol > eyhi[None]))
    pi_, ei = np.nonzero(near)
    if pi_.size == 0:
        return out
    d, e, f = (y2 - y1)[ei], (x1 - x2)[ei], (y1 * x2 - x1 * y2)[ei]
    for b in range(4):
        vx1, vy1, vx2, vy2 = vx[pi_, b], vy[pi_, b], vx[pi_, (b + 1) & 3], vy[pi_, (b + 1) & 3]
        a_, b_, c_ = vy2 - vy1, vx1 - vx2, vy1 * vx2 - vx1 * vy2
        det = a_ * e - b_ * d
        par = det == 0
        det = np.where(par, 1.0, det)
        rx, ry = (b_ * f - c_ * e) / det, (c_ * d - a_ * f) / det
        hit = ~(rx > exhi[ei]) & ~(rx < exlo[ei]) & ~(ry > eyhi[ei]) & ~(ry < eylo[ei])
        hit &= ~(rx > np.maximum(vx1, vx2) + tol) & ~(rx < np.minimum(vx1, vx2) - tol)
        hit &= ~(ry > np.maximum(vy1, vy2) + tol) & ~(ry < np.minimum(vy1, vy2) - tol)
        out[pi_, b, ei] = hit & ~par
    return out


def sample_path(p, slot, seg):
    """BUILD-DEFINED sampling: per segment the poses at arc length k * sample_step, k = 0 .. ceil(len / sample_step), the last
    one clipped to the segment's end.  Returns [P, 3] in the rear-axle frame of the start."""
    x = y = yaw = 0.0
    poses = []
    for i in range(N_SEG[slot]):
        d = seg[i] * p.radius
        n = int(np.ceil(abs(d) / p.sample_step)) + 1
        arc = np.minimum(np.arange(n) * p.sample_step, abs(d)) * (-1.0 if d < 0 else 1.0)
        px, py, pyaw = advance(x, y, yaw, int(LETTERS[slot, i]), arc, p.radius)
        poses.append(np.stack([px, py, pyaw], 1))
        x, y, yaw = advance(x, y, yaw, int(LETTERS[slot, i]), d, p.radius)
    return np.concatenate(poses)


def n_poses(p, slot, seg):
    return sum(int(np.ceil(abs(seg[i] * p.radius) / p.sample_step)) + 1 for i in range(N_SEG[slot]))


# candidates: (signed segments [48, 5] in units of the radius, length [48] in metres, +inf for None) of the env, or None
Plan = collections.namedtuple("Plan", "status slot n_seg n_visited steer distance length shortest sorted_lengths candidates")


def _plan(status, slot=-1, n_visited=0, seg=None, length=np.nan, shortest=np.nan, sorted_lengths=(), radius=1.0, with_path=False,
          cand=None):
    steer, dist, n_seg = np.zeros(5, np.int32), np.zeros(5), 0
    if with_path:
        n_seg = int(N_SEG[slot])
        steer[:n_seg] = LETTERS[slot, :n_seg]
        dist[:n_seg] = seg[:n_seg] * radius
    return Plan(status, slot, n_seg, n_visited, steer, dist, length, shortest, np.asarray(sorted_lengths, float), cand)


def plan(p, lidar_range, ego, target_xy, target_heading, scan, base=None, active=True):
    """get_rs_path :52-121 for one env.  ego = (x, y, heading), target_xy [4, 2]; scan [n_beams] fp32 in the ego's frame."""
    ego = np.asarray(ego, float)
    dest = np.mean(np.asarray(target_xy, float).reshape(4, 2), axis=0)
    th = float(target_heading)
    if not (active and np.isfinite(ego).all() and np.isfinite(dest).all() and np.isfinite(th)):
        return _plan(NO_TARGET)
    dest = dest - p.center_shift * np.array([np.cos(th), np.sin(th)])
    e = ego[:2] - p.center_shift * np.array([np.cos(ego[2]), np.sin(ego[2])])
    rel = np.sqrt((dest[0] - e[0]) ** 2 + (dest[1] - e[1]) ** 2)
    if rel > p.threshold_distance:
        return _plan(FAR)
    ang = np.arctan2(dest[1] - e[1], dest[0] - e[0]) - ego[2]
    gx, gy, gyaw = rel * np.cos(ang), rel * np.sin(ang), th - ego[2]
    valid, seg, total = candidates(gx / p.radius, gy / p.radius, gyaw)
    valid, seg, length = valid[0], seg[0], np.where(valid[0], total[0] * p.radius, np.inf)
    mk = lambda *a, **k: _plan(*a, cand=(seg, length), **k)
    order = sorted((length[s], s) for s in range(48) if valid[s])
    lens = [l for l, _ in order]
    if not order:
        return mk(NONE_FREE)
    scan = np.asarray(scan, np.float32)
    if np.isnan(scan).any():
        return mk(UNCHECKED, shortest=lens[0], sorted_lengths=lens)
    if base is None:
        base = vehicle_base(len(scan), p.half_length, p.half_width)
    edges = chain(p, scan, lidar_range, base)
    keep = ~collide_map(p, [[gx, gy, gyaw]], edges).any((0, 1))   # :180-191, the goal in the chain's frame
    edges = tuple(v[keep] for v in edges)
    visited = 0
    for l, s in order:
        if l > p.length_ratio * lens[0]:
            break
        visited += 1
        if n_poses(p, s, seg[s]) > MAX_POSES:
            return mk(UNCHECKED, s, visited, seg[s], l, lens[0], lens, p.radius, True)
        if not collide_map(p, sample_path(p, s, seg[s]), edges).any():
            return mk(FOUND, s, visited, seg[s], l, lens[0], lens, p.radius, True)
    return mk(NONE_FREE, -1, visited, shortest=lens[0], sorted_lengths=lens)


def plan_with_margin(p, lidar_range, ego, target_xy, target_heading, scan, base=None, active=True):
    """(plan, robust): robust = status and slot are the same with every finite scan value moved by +-SCAN_SHIFT"""
    scan = np.asarray(scan, np.float32)
    main = plan(p, lidar_range, ego, target_xy, target_heading, scan, base, active)
    robust = True
    if main.status in (FOUND, NONE_FREE, UNCHECKED) and not np.isnan(scan).any():
        if base is None:
            base = vehicle_base(len(scan), p.half_length, p.half_width)
        for sh in (SCAN_SHIFT, -SCAN_SHIFT):
            # the shift is applied to the clipped fp64 distances: an fp32 scan value cannot carry 1e-6 m at 20 m
            q = p._replace(distance_tolerance=p.distance_tolerance - sh)
            other = plan(q, lidar_range, ego, target_xy, target_heading, scan, base, active)
            robust &= other.status == main.status and other.slot == main.slot
    return main, robust
