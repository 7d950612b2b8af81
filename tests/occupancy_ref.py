"""The occupancy grid of t2d_occupancy_grid (include/t2d.h) as a numpy fp64 specification, operation by operation
what tactics2d_amd/csrc/t2d_occupancy.hip does -- TEST INFRASTRUCTURE, never imported by the product.  cos / sin come through
`oracle.sincos`, the C restatement of the device's sincos_det, so every number here has the device's bits.

The rule (build-defined; the reference has no counterpart): cell (row, col) is the closed square of half side cell_size / 2 centred at
(origin_x + col * cell_size, origin_y + row * cell_size); it is occupied iff the Euclidean distance between it and some listed
obstacle, as a closed filled set, is <= inflate.  `exact_occupied` / `exact_distance2` are that rule in rational arithmetic.

Every element becomes n fp64 vertices (a ring as it is, a participant's box as four corners, a disc as ONE vertex whose radius joins
the threshold) with a guard g = GUARD * max(|its coordinates|, the window's magnitude): rounding can only ADD cells.  BAND bounds
how far beyond `inflate` an added cell can lie, for coordinates up to MAGNITUDE (the derivation is DESIGN.md 4.24)."""
from fractions import Fraction

import numpy as np

OK, INVALID = 0, 1
SHAPE_OBB, SHAPE_CIRCLE = 0, 1
GUARD = 2.0 ** -44
MAGNITUDE = 1024.0            # |coordinate| of the scenes of tests/occupancy_scenes.py stays below this
BAND = 4 * GUARD * MAGNITUDE  # m: a cell the specification marks has exact distance <= inflate + BAND (2^-32 m)


def _sincos():
    import oracle.oracle as O
    return O.sincos


def window_magnitude(H, W, cell_size, origin, inflate):
    """t2d_api.hip: t2d_occupancy_grid's `mwin`, the same operations"""
    ox, oy, cs = float(origin[0]), float(origin[1]), float(cell_size)
    fx = ox + float(W - 1) * cs
    fy = oy + float(H - 1) * cs
    return (max(max(abs(ox), abs(fx)), max(abs(oy), abs(fy))) + cs) + float(inflate)


def box_corners(x, y, heading, length, width):
    """the four corners of a participant's box as the kernel builds them: (x, y, heading) fp32 values, one rounding per operation"""
    s, c = _sincos()(float(np.float32(heading)))
    x, y = float(np.float32(x)), float(np.float32(y))
    hl, hw = 0.5 * float(length), 0.5 * float(width)
    out = []
    for lx, ly in ((hl, -hw), (hl, hw), (-hl, hw), (-hl, -hw)):
        out.append((x + (lx * c - ly * s), y + (lx * s + ly * c)))
    return np.array(out, np.float64)


def elements(rings=(), participants=(), include_participants=False, exclude_slot=-1):
    """The listing of one env -> (list of (vertices float64 [n, 2], radius), invalid).  rings: iterables of fp32 vertices (fewer than
    3: ignored); participants: (x, y, heading, shape, length, width, active) in slot order."""
    out, invalid = [], False
    for r in rings:
        v = np.asarray(r, np.float32).reshape(-1, 2).astype(np.float64)
        if len(v) >= 3:
            out.append((v, 0.0))
    if include_participants:
        for slot, (x, y, h, shape, length, width, active) in enumerate(participants):
            if not active or slot == exclude_slot:
                continue
            if not np.all(np.isfinite(np.float32([x, y, h]))):
                invalid = True
                continue
            if int(shape) == SHAPE_CIRCLE:
                out.append((np.array([[float(np.float32(x)), float(np.float32(y))]]), max(0.5 * float(width), 0.0)))
            else:
                out.append((box_corners(x, y, h, length, width), 0.0))
    return out, invalid


def thresholds(v, rad, mwin, inflate):
    """g, rg2, g2 of one element (phase 1 of the kernel)"""
    mag = max(float(mwin), float(rad)) if len(v) == 1 else float(mwin)
    for x, y in v:
        mag = max(mag, max(abs(float(x)), abs(float(y))))
    g = mag * GUARD
    rg = (float(inflate) + float(rad)) + g
    return g, rg * rg, g * g


def cell_axes(H, W, cell_size, origin):
    cs = float(cell_size)
    return float(origin[0]) + np.arange(W, dtype=np.float64) * cs, float(origin[1]) + np.arange(H, dtype=np.float64) * cs


def element_hits(v, rad, H, W, cell_size, origin, inflate, mwin):
    """bool [H, W]: the cells one element occupies -- cell_hit of the kernel, over all cells at once"""
    cxs, cys = cell_axes(H, W, cell_size, origin)
    half = 0.5 * float(cell_size)
    cx, cy = np.meshgrid(cxs, cys)
    x0, x1, y0, y1 = cx - half, cx + half, cy - half, cy + half
    g, rg2, g2 = thresholds(v, rad, mwin, inflate)
    n = len(v)
    hit = np.zeros((H, W), bool)
    anypos, anyneg, anyzero = (np.zeros((H, W), bool) for _ in range(3))
    with np.errstate(over="ignore", invalid="ignore"):
        for k in range(n):
            ax, ay = float(v[k][0]), float(v[k][1])
            dxv = np.maximum(np.maximum(x0 - ax, ax - x1), 0.0)
            dyv = np.maximum(np.maximum(y0 - ay, ay - y1), 0.0)
            hit |= dxv * dxv + dyv * dyv <= rg2
            if n < 3:
                continue
            bx, by = float(v[(k + 1) % n][0]), float(v[(k + 1) % n][1])
            dx, dy = bx - ax, by - ay
            L2 = dx * dx + dy * dy
            lim = rg2 * L2
            ex, ey = (x0 - ax, x1 - ax), (y0 - ay, y1 - ay)
            mn, mx = np.full((H, W), np.inf), np.full((H, W), -np.inf)
            for c in range(4):
                px, py = ex[c & 1], ey[c >> 1]
                t = px * dx + py * dy
                cr = px * dy - py * dx
                hit |= (t > 0.0) & (t < L2) & (cr * cr <= lim)
                mn, mx = np.minimum(mn, cr), np.maximum(mx, cr)
            gl = g2 * L2
            lo_ok = (mn <= 0.0) | (mn * mn <= gl)
            hi_ok = (mx >= 0.0) | (mx * mx <= gl)
            xov = (x0 - max(ax, bx) <= g) & (min(ax, bx) - x1 <= g)
            yov = (y0 - max(ay, by) <= g) & (min(ay, by) - y1 <= g)
            hit |= lo_ok & hi_ok & xov & yov
            crc = (cx - ax) * dy - (cy - ay) * dx
            anypos |= crc > 0.0
            anyneg |= crc < 0.0
            if L2 != 0.0:
                anyzero |= ~(crc > 0.0) & ~(crc < 0.0)
    if n >= 3:
        hit |= ~anyzero & (anypos != anyneg)
    return hit


def occupancy(H, W, cell_size, origin, inflate, rings=(), participants=(), include_participants=False, exclude_slot=-1):
    """(mask uint8 [H, W], status) of one env"""
    els, invalid = elements(rings, participants, include_participants, exclude_slot)
    if invalid:
        return np.ones((H, W), np.uint8), INVALID
    mwin = window_magnitude(H, W, cell_size, origin, inflate)
    occ = np.zeros((H, W), bool)
    for v, rad in els:
        occ |= element_hits(v, rad, H, W, cell_size, origin, inflate, mwin)
    return occ.astype(np.uint8), OK


def weights(mask, free_weight=1.0):
    return np.where(np.asarray(mask) != 0, np.inf, float(free_weight))


# ---- the rule in exact rational arithmetic ------------------------------------------------------------------------------------
def _F(x):
    return Fraction(float(x))


def _pt_seg_d2(px, py, ax, ay, bx, by):
    dx, dy = bx - ax, by - ay
    L2 = dx * dx + dy * dy
    ex, ey = px - ax, py - ay
    if L2 == 0:
        return ex * ex + ey * ey
    t = ex * dx + ey * dy
    if t <= 0:
        return ex * ex + ey * ey
    if t >= L2:
        return (px - bx) ** 2 + (py - by) ** 2
    cr = ex * dy - ey * dx
    return cr * cr / L2


def _pt_box_d2(px, py, x0, x1, y0, y1):
    dx = max(x0 - px, px - x1, 0)
    dy = max(y0 - py, py - y1, 0)
    return dx * dx + dy * dy


def _seg_box_d2(ax, ay, bx, by, x0, x1, y0, y1):
    """squared distance of a closed segment and a closed axis-aligned box, exact"""
    corners = ((x0, y0), (x1, y0), (x1, y1), (x0, y1))
    # they meet: an end point inside, or the segment crosses one of the box's edges
    if _pt_box_d2(ax, ay, x0, x1, y0, y1) == 0 or _pt_box_d2(bx, by, x0, x1, y0, y1) == 0:
        return Fraction(0)
    dx, dy = bx - ax, by - ay
    cr = [(cx - ax) * dy - (cy - ay) * dx for cx, cy in corners]
    if min(cr) <= 0 <= max(cr) and max(ax, bx) >= x0 and min(ax, bx) <= x1 and max(ay, by) >= y0 and min(ay, by) <= y1:
        return Fraction(0)   # (the separating-axis test of a segment and a box: its three axes)
    d2 = min(_pt_box_d2(ax, ay, x0, x1, y0, y1), _pt_box_d2(bx, by, x0, x1, y0, y1))
    for cx, cy in corners:
        d2 = min(d2, _pt_seg_d2(cx, cy, ax, ay, bx, by))
    return d2


def _inside_convex(px, py, v):
    """the closed convex ring v (either orientation) contains the point"""
    pos = neg = False
    n = len(v)
    for k in range(n):
        ax, ay = v[k]
        bx, by = v[(k + 1) % n]
        cr = (px - ax) * (by - ay) - (py - ay) * (bx - ax)
        pos |= cr > 0
        neg |= cr < 0
    return not (pos and neg)


def exact_distance2(v, cx, cy, half):
    """squared distance (a Fraction) of the closed convex ring / the point v and the closed square of half side `half` at (cx, cy)"""
    x0, x1, y0, y1 = cx - half, cx + half, cy - half, cy + half
    n = len(v)
    if n == 1:
        return _pt_box_d2(v[0][0], v[0][1], x0, x1, y0, y1)
    if _inside_convex(cx, cy, v):
        return Fraction(0)
    return min(_seg_box_d2(v[k][0], v[k][1], v[(k + 1) % n][0], v[(k + 1) % n][1], x0, x1, y0, y1) for k in range(n))


def exact_cells(H, W, cell_size, origin, els):
    """Fraction [H][W]: min over the elements of (distance - radius), squared where positive, as (d2, rad) pairs is awkward -- so this
    returns, per cell, the list of (d2, rad) of every element: the caller compares d2 with (inflate + rad)^2"""
    cs, ox, oy = _F(cell_size), _F(origin[0]), _F(origin[1])
    half = cs / 2
    fv = [([(_F(x), _F(y)) for x, y in v], _F(rad)) for v, rad in els]
    return [[[(exact_distance2(v, ox + c * cs, oy + r * cs, half), rad) for v, rad in fv] for c in range(W)] for r in range(H)]


def exact_within(pairs, limit):
    """some element of the cell's (d2, rad) list lies within distance `limit` (a Fraction): d <= limit + rad"""
    return any(d2 <= (limit + rad) ** 2 for d2, rad in pairs)
