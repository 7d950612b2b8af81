"""The numpy specification of the Dubins paths (tactics2d/interpolator/dubins.py) and of the sampled curve lines of a Dubins or
Reeds-Shepp word (DubinsPath.get_curve_line dubins.py:28-104, ReedsSheppPath.get_curve_line reeds_shepp.py:46-139, Circle.get_arc
geometry/circle.py:106-139), in the project's own words: what t2d_dubins_paths, t2d_curve_lines and t2d_curve_routes (include/t2d.h)
are held against, and what tests/golden/dubins_curves.npz -- made by running the reference's own classes -- pins.

Operation order follows the reference's expressions (numpy evaluates left to right); the device evaluates the same operations
with the library's own sincos / atan2 / mod 2 pi, so values agree to a few ulp and integers (validity, counts) agree except on
the reference's own thresholds -- which `stable_mask` / `stable_count` find by perturbation, as the fixture script does."""
import numpy as np

PI, TWO_PI, PIO2 = np.pi, 2 * np.pi, np.pi / 2
WORDS = ("LRL", "RLR", "LSL", "RSL", "RSR", "LSR")      # get_all_path :264-271
STEER = {"L": 1, "R": -1, "S": 0}
LETTERS = np.array([[STEER[c] for c in w] for w in WORDS], np.int8)
DUBINS, RS = 0, 1                                       # the sampling rules (T2D_CURVE_DUBINS / T2D_CURVE_RS)
DEFAULT_STEP = {DUBINS: 0.1, RS: 0.01}


# ---- Dubins.get_all_path / get_path --------------------------------------------------------------------------------------------
def normalise(start, goal, radius):   # :259-262
    start, goal = np.atleast_2d(start).astype(float), np.atleast_2d(goal).astype(float)
    dx, dy = goal[:, 0] - start[:, 0], goal[:, 1] - start[:, 1]
    theta = np.arctan2(dy, dx)
    d = np.sqrt(dx * dx + dy * dy) / radius
    return np.mod(start[:, 2] - theta, TWO_PI), np.mod(goal[:, 2] - theta, TWO_PI), d


def words(alpha, beta, d, lrl="reference"):
    """valid [n, 6], (t, p, q) [n, 6, 3] (zero where None) of the six words for arrays of normalised queries.  lrl: "reference" =
    _LRL as written (:216-231), "standard" = the family's sign of its tmp term (build-defined)."""
    a, b = np.asarray(alpha, float), np.asarray(beta, float)
    sa, ca, sb, cb, cab = np.sin(a), np.cos(a), np.sin(b), np.cos(b), np.cos(a - b)
    n = len(a)
    valid, seg = np.zeros((n, 6), bool), np.zeros((n, 6, 3))
    with np.errstate(invalid="ignore"):
        # LRL :216-231
        disc = (6 - d ** 2 + 2 * cab + 2 * d * (-sa + sb)) / 8
        ok = ~(np.abs(disc) > 1)
        p = np.mod(TWO_PI - np.arccos(np.clip(disc, -1, 1)), TWO_PI)
        tmp = np.arctan2(ca - cb, d + sa - sb)
        t = np.mod(-a + tmp + p / 2, TWO_PI) if lrl == "reference" else np.mod(-a - tmp + p / 2, TWO_PI)
        q = np.mod(b - a - t + p, TWO_PI)
        valid[:, 0], seg[:, 0] = ok, np.stack([t, p, q], 1)
        # RLR :200-214
        disc = (6 - d ** 2 + 2 * cab + 2 * d * (sa - sb)) / 8
        ok = ~(np.abs(disc) > 1)
        tmp = np.arctan2(ca - cb, d - sa + sb)
        p = np.mod(TWO_PI - np.arccos(np.clip(disc, -1, 1)), TWO_PI)
        t = np.mod(a - tmp + p / 2, TWO_PI)
        q = np.mod(a - b - t + p, TWO_PI)
        valid[:, 1], seg[:, 1] = ok, np.stack([t, p, q], 1)
        # LSL :165-179
        disc = 2 + d ** 2 - 2 * cab + 2 * d * (sa - sb)
        ok = ~(disc < 0)
        tmp = np.arctan2(-ca + cb, d + sa - sb)
        valid[:, 2], seg[:, 2] = ok, np.stack([np.mod(-(a - tmp), TWO_PI), np.sqrt(np.abs(disc)), np.mod(b - tmp, TWO_PI)], 1)
        # RSL :146-163
        disc = -2 + d ** 2 + 2 * cab - 2 * d * (sa + sb)
        ok = ~(disc < 0)
        p = np.sqrt(np.abs(disc))
        tmp = np.arctan2(ca + cb, d - sa - sb) - np.arctan2(2, p)
        valid[:, 3], seg[:, 3] = ok, np.stack([np.mod(a - tmp, TWO_PI), p, np.mod(b - tmp, TWO_PI)], 1)
        # RSR :130-144
        disc = 2 + d ** 2 - 2 * cab + 2 * d * (-sa + sb)
        ok = ~(disc < 0)
        tmp = np.arctan2(ca - cb, d - sa + sb)
        valid[:, 4], seg[:, 4] = ok, np.stack([np.mod(a - tmp, TWO_PI), np.sqrt(np.abs(disc)), np.mod(-(b - tmp), TWO_PI)], 1)
        # LSR :181-198
        disc = -2 + d ** 2 + 2 * cab + 2 * d * (sa + sb)
        ok = ~(disc < 0)
        p = np.sqrt(np.abs(disc))
        tmp = -np.arctan2(ca + cb, d + sa + sb) + np.arctan2(2, p)
        valid[:, 5], seg[:, 5] = ok, np.stack([np.mod(-a + tmp, TWO_PI), p, np.mod(-b + tmp, TWO_PI)], 1)
    finite = np.isfinite(a) & np.isfinite(b) & np.isfinite(d)       # build-defined: a query that is not finite has no path
    valid &= finite[:, None]
    seg[~valid] = 0.0
    return valid, seg


def all_paths(start, goal, radius, lrl="reference"):
    """valid [n, 6], segments [n, 6, 3] in units of the radius, length [n, 6] in metres (+inf where None)"""
    valid, seg = words(*normalise(start, goal, radius), lrl)
    total = (np.abs(seg[..., 0]) + np.abs(seg[..., 1])) + np.abs(seg[..., 2])
    return valid, seg, np.where(valid, total * radius, np.inf)


def mask_of(valid):
    return (np.atleast_2d(valid) << np.arange(6)).sum(1).astype(np.uint8)


def shortest_slots(length):
    """per query: get_path's slot (:297-302, the LAST of equal shortest lengths) and the lowest-index shortest; -1: no path"""
    length = np.atleast_2d(length)
    last, first = np.full(len(length), -1, np.int32), np.full(len(length), -1, np.int32)
    for i, row in enumerate(length):
        best = np.inf
        for s, v in enumerate(row):
            if v == np.inf:
                continue
            if first[i] < 0 or v < best:
                first[i] = s
            if not v > best:
                last[i], best = s, v
    return last, first


def stable_mask(start, goal, radius, lrl="reference", shift=1e-9):
    """bool [n]: the validity mask is the same for the goal shifted by +-shift in x, in y and in heading"""
    start, goal = np.atleast_2d(start).astype(float), np.atleast_2d(goal).astype(float)
    base = mask_of(all_paths(start, goal, radius, lrl)[0])
    ok = np.ones(len(base), bool)
    for axis in range(3):
        for dlt in (shift, -shift):
            g = goal.copy()
            g[:, axis] += dlt
            ok &= mask_of(all_paths(start, g, radius, lrl)[0]) == base
    return ok


# ---- get_curve_line -------------------------------------------------------------------------------------------------------------
def centre_of(point, heading, radius, letter):
    """get_circle_by_tangent_vector: the centre lies a radius to the left (L) or to the right (R) of the heading"""
    a = heading + PIO2 if letter > 0 else heading - PIO2
    return point + radius * np.array([np.cos(a), np.sin(a)])


def _linspace(a, b, n):
    """np.linspace's own arithmetic: a + k * ((b - a) / (n - 1)), the last value b"""
    if n == 1:
        return np.array([a], float)
    out = a + np.arange(n) * ((b - a) / (n - 1))
    out[-1] = b
    return out


def segment_line(point, heading, radius, step, rule, letter, seg):
    """One segment: (points [c, 2], yaw [c], end point, end heading).  seg: the signed length in units of the radius."""
    point = np.asarray(point, float)
    a, fwd = abs(seg), (-1.0 if seg < 0 and rule == RS else 1.0)   # (DubinsPath takes abs(segment) everywhere, :94-98)
    if a < 1e-15:
        return point[None].copy(), np.array([heading]), point.copy(), heading
    if letter == 0:   # get_straight_line
        end = point + np.array([np.cos(heading), np.sin(heading)]) * radius * a * fwd
        dx, dy = end[0] - point[0], end[1] - point[1]
        n = max(2 if rule == RS else 1, int(np.ceil(np.sqrt(dx * dx + dy * dy) / step)))
        return np.stack([_linspace(point[0], end[0], n), _linspace(point[1], end[1], n)], 1), np.full(n, heading), end, heading
    left = letter > 0
    cw = (left and fwd < 0) or (not left and fwd > 0) if rule == RS else not left
    centre = centre_of(point, heading, radius, letter)
    a0 = heading - PIO2 if left else heading + PIO2
    delta = -step / radius if cw else step / radius
    stop = a0 - a if cw else a0 + a
    n = max(0, int(np.ceil((stop - a0) / delta)))                     # np.arange's length
    ang = a0 + np.arange(n) * ((a0 + delta) - a0)                     # np.arange's fill
    pts = centre + np.stack([np.cos(ang), np.sin(ang)], 1) * radius
    h_end = heading - a if cw else heading + a
    end = centre + np.array([np.cos(stop), np.sin(stop)]) * radius
    if rule == RS and n < 2:
        return np.stack([point, end]), np.array([heading, h_end]), end, h_end
    if n == 0:
        return point[None].copy(), np.array([heading]), end, h_end
    return pts, _linspace(heading, h_end, n), end, h_end


def curve_line(seg, letters, start, radius, step, rule):
    """The curve of one word: xy [c, 2], yaw [c], end [3], per-segment counts.  seg / letters: the first n_seg = len(seg) entries.
    Build-defined: no segments, or a start or segment that is not finite: an empty curve (end = NaN)."""
    seg, start = np.asarray(seg, float), np.asarray(start, float)
    if len(seg) == 0 or not (np.isfinite(seg).all() and np.isfinite(start).all()):
        return np.zeros((0, 2)), np.zeros(0), np.full(3, np.nan), []
    point, heading = start[:2].copy(), float(start[2])
    xy, yaw, counts = [], [], []
    for s, l in zip(seg, letters):
        p, y, point, heading = segment_line(point, heading, radius, step, rule, int(l), float(s))
        xy.append(p)
        yaw.append(y)
        counts.append(len(p))
    return np.concatenate(xy), np.concatenate(yaw), np.array([point[0], point[1], heading]), counts


def stable_count(seg, letters, start, radius, step, rule, scale=1e-9):
    """the point count is the same with every segment scaled by 1 + scale and by 1 - scale"""
    base = curve_line(seg, letters, start, radius, step, rule)[3]
    return all(curve_line(np.asarray(seg, float) * f, letters, start, radius, step, rule)[3] == base for f in (1 + scale, 1 - scale))


def integrate(seg, letters, start, radius):
    """The end pose of driving the word from `start`: exact arcs and straights (no sampling)."""
    x, y, h = (float(v) for v in start)
    for s, l in zip(seg, letters):
        d = float(s) * radius
        if l == 0:
            x, y = x + d * np.cos(h), y + d * np.sin(h)
        else:
            h1 = h + l * d / radius
            x, y = x + l * radius * (np.sin(h1) - np.sin(h)), y + l * radius * (np.cos(h) - np.cos(h1))
            h = h1
    return np.array([x, y, h])


def route_vertices(xy, end, cap, before):
    """t2d_curve_routes' rule for one env: `before` float32 [cap, 2] is what the route held.  No points: unchanged.  Otherwise
    vertex k < count is point k rounded to fp32, vertex k >= count the curve's end point; more points than vertices: the first cap."""
    if len(xy) == 0:
        return np.asarray(before, np.float32).copy()
    out = np.repeat(np.asarray(end[:2], np.float64)[None], cap, 0)
    k = min(cap, len(xy))
    out[:k] = xy[:k]
    return out.astype(np.float32)


def pack_words(seg, letters, n_seg):
    """the 48-byte word records of t2d_curve_lines as float64 [n, 6]: f64 seg[5], i8 letter[5], i8 n_seg, 2 bytes of padding"""
    seg = np.atleast_2d(seg)
    n = len(seg)
    out = np.zeros((n, 6))
    out[:, :seg.shape[1]] = seg
    raw = out.view(np.int8).reshape(n, 48)
    raw[:, 40:40 + np.shape(letters)[1]] = letters
    raw[:, 45] = n_seg
    return out
