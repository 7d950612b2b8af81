"""Reference restatement of the off-route detector (test infrastructure; the definition is include/t2d.h, "Off-route
detection", and DESIGN.md 4.12).

Two statements of `OffRoute.update` (traffic/event_detection/off_route.py:24-34: route.distance(location) > threshold):

  * fp64, in the kernel's operation order.  Every numpy operation below -- on fp64 scalars in `seg_d2`, elementwise on fp64
    arrays in `evaluate` -- is ONE IEEE rounding (numpy never contracts a product and a sum), so the results are comparable
    with the kernel's (built with -ffp-contract=off) bit for bit.
  * exact, on fractions.Fraction: the squared distance exactly, the verdict `d2 > threshold^2` without a square root.

Coordinates and thresholds are fp32 values (what the pool and the C ABI hold), widened exactly.
"""
from fractions import Fraction

import numpy as np

F64 = np.float64


# ---------------------------------------------------------------------------------------------------- fp64, scalar
def seg_d2(ax, ay, bx, by, px, py):
    """squared distance of P to the segment A -> B; all arguments np.float64 scalars"""
    ux = bx - ax; uy = by - ay; wx = px - ax; wy = py - ay
    L2 = ux * ux + uy * uy
    t = wx * ux + wy * uy
    if t <= 0.0:
        return wx * wx + wy * wy
    if t >= L2:
        vx = px - bx; vy = py - by
        return vx * vx + vy * vy
    c = wx * uy - wy * ux
    return (c * c) / L2


def distance(route, px, py, thr):
    """(distance float32, off bool, index of the nearest segment) of one point against one polyline (fp32 (n, 2), n >= 2):
    the minimum over the segments in vertex order, strict `<` (the first minimum wins)"""
    r = np.asarray(route, np.float32).astype(F64)
    px, py = F64(np.float32(px)), F64(np.float32(py))
    d2min, seg = F64(np.inf), -1
    with np.errstate(all="ignore"):
        for k in range(len(r) - 1):
            d2 = seg_d2(r[k, 0], r[k, 1], r[k + 1, 0], r[k + 1, 1], px, py)
            if d2 < d2min:
                d2min, seg = d2, k
        d = np.sqrt(d2min)
        return np.float32(d), bool(d > F64(np.float32(thr))), seg


# ---------------------------------------------------------------------------------------------------- fp64, vectorised
def evaluate(VX, VY, nvert, x, y, thr, active):
    """Every participant at once.  VX, VY: float32 [N, S] padded route vertices of participant i (nvert[i] of them in use;
    nvert < 2 = no route); x, y, thr float32 [N]; active [N].  Returns (distance float32 [N], off uint8 [N], nearest segment
    int [N]) with the build-defined rows (no route, inactive, non-finite x or y): off = 0, distance = NaN, segment = -1."""
    VX, VY = np.asarray(VX, np.float32).astype(F64), np.asarray(VY, np.float32).astype(F64)
    x32, y32 = np.asarray(x, np.float32), np.asarray(y, np.float32)
    px, py = x32.astype(F64), y32.astype(F64)
    nvert = np.asarray(nvert)
    N, S = VX.shape
    d2min, seg = np.full(N, np.inf), np.full(N, -1)
    with np.errstate(all="ignore"):
        for k in range(S - 1):
            ax, ay, bx, by = VX[:, k], VY[:, k], VX[:, k + 1], VY[:, k + 1]
            ux = bx - ax; uy = by - ay; wx = px - ax; wy = py - ay
            L2 = ux * ux + uy * uy
            t = wx * ux + wy * uy
            vx = px - bx; vy = py - by
            c = wx * uy - wy * ux
            d2 = np.where(t <= 0.0, wx * wx + wy * wy, np.where(t >= L2, vx * vx + vy * vy, (c * c) / L2))
            better = (k + 1 < nvert) & (d2 < d2min)
            d2min = np.where(better, d2, d2min)
            seg = np.where(better, k, seg)
        d = np.sqrt(d2min)
        live = (np.asarray(active) != 0) & (nvert >= 2) & np.isfinite(x32) & np.isfinite(y32)
        off = live & (d > np.asarray(thr, np.float32).astype(F64))
        dist = np.where(live, d, np.nan).astype(np.float32)
    return dist, off.astype(np.uint8), np.where(live, seg, -1)


def pad_routes(routes, index):
    """routes: list of fp32 (n, 2) polylines; index int [N] (-1 = none) -> VX, VY [N, S], nvert [N]"""
    index = np.asarray(index)
    S = max([len(r) for r in routes] + [2])
    RX, RY = np.zeros((len(routes) + 1, S), np.float32), np.zeros((len(routes) + 1, S), np.float32)
    n = np.zeros(len(routes) + 1, int)
    for k, r in enumerate(routes):
        r = np.asarray(r, np.float32).reshape(-1, 2)
        RX[k, :len(r)], RY[k, :len(r)], n[k] = r[:, 0], r[:, 1], len(r)
    sel = np.where(index < 0, len(routes), index)
    return RX[sel], RY[sel], n[sel]


def evaluate_sets(route_sets, set_of_env, route_of, A, x, y, thr, active):
    """set routes: route_sets [[polyline, ...] per set], set_of_env [E], route_of [N] (index inside the env's set, -1 none)"""
    flat, base = [], []
    for routes in route_sets:
        base.append(len(flat)); flat += list(routes)
    route_of = np.asarray(route_of)
    env = np.arange(len(route_of)) // A
    index = np.where(route_of < 0, -1, np.asarray(base)[np.asarray(set_of_env)[env]] + route_of)
    return evaluate(*pad_routes(flat, index), x, y, thr, active)


def evaluate_traces(trace_xy, first_slot, last_slot, src_env, route_of, A, x, y, thr, active):
    """trace routes: trace_xy float32 [n_slots, N_src, 2] (the recorded x, y), windows [N_src], src_env [E], route_of [N]
    (source agent index, -1 none): the route of participant i is slots first..last of source participant
    src_env[env(i)] * A + route_of[i]; fewer than two slots = no route"""
    route_of = np.asarray(route_of)
    N = len(route_of)
    env = np.arange(N) // A
    j = np.asarray(src_env)[env] * A + np.maximum(route_of, 0)
    first, last = np.asarray(first_slot)[j], np.asarray(last_slot)[j]
    nvert = np.where(route_of < 0, 0, np.maximum(last - first + 1, 0))
    S = max(int(nvert.max()), 2)
    slot = np.minimum(first[:, None] + np.arange(S)[None, :], trace_xy.shape[0] - 1)   # (padding repeats in-range slots)
    V = trace_xy[slot, j[:, None]]
    return evaluate(V[..., 0], V[..., 1], nvert, x, y, thr, active)


# ---------------------------------------------------------------------------------------------------- exact
def _fr(v):
    return Fraction(float(np.float32(v)))


def exact_d2(route, px, py):
    """(exact squared distance, index of the first nearest segment) on Fractions"""
    r = np.asarray(route, np.float32)
    P = (_fr(px), _fr(py))
    best, seg = None, -1
    for k in range(len(r) - 1):
        A, B = (_fr(r[k, 0]), _fr(r[k, 1])), (_fr(r[k + 1, 0]), _fr(r[k + 1, 1]))
        ux, uy, wx, wy = B[0] - A[0], B[1] - A[1], P[0] - A[0], P[1] - A[1]
        L2, t = ux * ux + uy * uy, wx * ux + wy * uy
        if t <= 0:
            d2 = wx * wx + wy * wy
        elif t >= L2:
            d2 = (P[0] - B[0]) ** 2 + (P[1] - B[1]) ** 2
        else:
            d2 = (wx * uy - wy * ux) ** 2 / L2
        if best is None or d2 < best:
            best, seg = d2, k
    return best, seg


def exact_off(d2, thr):
    """distance > threshold without a square root (a negative threshold: every distance is beyond it)"""
    t = _fr(thr)
    return True if t < 0 else d2 > t * t


# ---------------------------------------------------------------------------------------------------- cases
def kats():
    """Known answers where every operation is exact (axis-aligned segments, small dyadic numbers): (name, route, (px, py),
    threshold, off, distance, nearest segment)."""
    f = np.float32
    up = lambda v: float(np.nextafter(f(v), f(np.inf)))
    L = [(0, 0), (8, 0), (8, 4)]
    return [
        ("at the threshold: not off", L, (4, 2), 2.0, False, 2.0, 0),
        ("one fp32 ulp further: off", L, (4, up(2.0)), 2.0, True, up(2.0), 0),
        ("one fp32 ulp less threshold: off", L, (4, 2), float(np.nextafter(f(2.0), f(0))), True, 2.0, 0),
        ("foot before the first vertex", L, (-3, 4), 4.5, True, 5.0, 0),
        ("foot beyond the last vertex", L, (11, 8), 5.0, False, 5.0, 1),
        ("vertex hit", L, (8, 0), 0.0, False, 0.0, 0),
        ("on a segment", L, (8, 3), 0.0, False, 0.0, 1),
        ("zero-length first segment", [(1, 1), (1, 1), (5, 1)], (1, 4), 2.5, True, 3.0, 0),
        ("zero-length middle segment", [(0, 0), (4, 0), (4, 0), (4, 4)], (6, 0), 2.0, False, 2.0, 0),
        ("the first of two equal minima", [(0, 0), (4, 0), (4, 4), (0, 4)], (2, 2), 1.0, True, 2.0, 0),
        ("equal minima, the later one listed first", [(0, 4), (4, 4), (4, 0), (0, 0)], (2, 2), 3.0, False, 2.0, 0),
        ("negative threshold: off at distance 0", L, (8, 0), -1.0, True, 0.0, 0),
        ("nearest segment is the last", [(0, 0), (0, 8), (8, 8), (8, 0)], (6, 1), 1.5, True, 2.0, 2),
    ]


def random_cases(n=20000, seed=7):
    """The issue's recipe: 2-12 vertices; first vertex U(-200, 200)^2; steps of U(1, 30) m along a heading that starts
    U(0, 2 pi) and random-walks with sigma 0.4 rad per vertex; vertices rounded to fp32; 10 % of the routes with >= 3
    vertices get vertex 1 := vertex 0; threshold U(0.5, 5) as fp32; the point = a uniform point of a uniformly chosen
    segment + N(0, threshold) per axis, as fp32.  Yields (route float32 (n, 2), px, py, thr)."""
    rng = np.random.default_rng(seed)
    for _ in range(n):
        nv = int(rng.integers(2, 13))
        v = np.zeros((nv, 2))
        v[0] = rng.uniform(-200, 200, 2)
        h = rng.uniform(0, 2 * np.pi)
        for k in range(1, nv):
            step = rng.uniform(1, 30)
            v[k] = v[k - 1] + step * np.array([np.cos(h), np.sin(h)])
            h += rng.normal(0, 0.4)
        v = v.astype(np.float32)
        if nv >= 3 and rng.uniform() < 0.1:
            v[1] = v[0]
        thr = np.float32(rng.uniform(0.5, 5))
        k = int(rng.integers(0, nv - 1))
        s = rng.uniform()
        p = (v[k].astype(F64) * (1 - s) + v[k + 1].astype(F64) * s + rng.normal(0, float(thr), 2)).astype(np.float32)
        yield v, p[0], p[1], thr


# what OffRoute.reset must refuse with TypeError (the golden file records the names; both sides build the values here)
UNCOERCIBLE = {"none": None, "scalar": 5, "string": "abc", "single_point": [(1.0, 2.0)], "empty": [], "flat_numbers": [1.0, 2.0, 3.0]}
