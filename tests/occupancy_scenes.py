"""Scenes for the occupancy grid (t2d_occupancy_grid), shared by tests/test_occupancy_ref.py (the specification
against exact rational arithmetic) and tests/test_gpu_occupancy.py (the kernel against the specification) -- TEST INFRASTRUCTURE.

A scene is a dict: H, W, cell_size, origin, inflate, rings (lists of fp32 vertices), participants ((x, y, heading, shape, length,
width, active) per slot), include_participants, exclude_slot.  Contact scenes add `cell` (row, col) and `occupied`: what the exact
rule says of that cell."""
import numpy as np

SHAPE_OBB, SHAPE_CIRCLE = 0, 1
CELL_SIZES = (0.25, 0.5, 1.0)
INFLATES = (0.0, 0.3, 1.0)


def scene(H, W, cell_size, origin, inflate, rings=(), participants=(), include_participants=False, exclude_slot=-1, **extra):
    return dict(H=H, W=W, cell_size=float(cell_size), origin=(float(origin[0]), float(origin[1])), inflate=float(inflate),
                rings=[np.asarray(r, np.float32).reshape(-1, 2) for r in rings], participants=list(participants),
                include_participants=bool(include_participants), exclude_slot=int(exclude_slot), **extra)


def spec_kwargs(sc):
    """the arguments of occupancy_ref.occupancy"""
    return {k: sc[k] for k in ("H", "W", "cell_size", "origin", "inflate", "rings", "participants", "include_participants", "exclude_slot")}


def convex_ring(rng, centre, size, n=None):
    """a convex ring of 3..8 fp32 vertices: points of an ellipse at separated angles, either orientation"""
    n = int(rng.integers(3, 9)) if n is None else n
    gaps = 0.35 + rng.random(n)
    ang = np.cumsum(gaps / gaps.sum() * 2 * np.pi) + rng.random() * 2 * np.pi
    a, b, rot = size * (0.5 + rng.random()), size * (0.5 + rng.random()), rng.random() * np.pi
    px, py = a * np.cos(ang), b * np.sin(ang)
    v = np.stack([centre[0] + px * np.cos(rot) - py * np.sin(rot), centre[1] + px * np.sin(rot) + py * np.cos(rot)], axis=1)
    if rng.random() < 0.5:
        v = v[::-1]
    return np.ascontiguousarray(v, np.float32)


def random_scene(seed, H=11, W=13, n_rings=3, n_boxes=2, n_discs=1, cell_size=None, inflate=None):
    """rings, oriented boxes and discs at random poses about a window placed anywhere within +-200 m"""
    rng = np.random.default_rng(seed)
    cs = float(CELL_SIZES[seed % 3]) if cell_size is None else cell_size
    infl = float(INFLATES[(seed // 3) % 3]) if inflate is None else inflate
    origin = (float(np.float32(rng.uniform(-200, 200 - W * cs))), float(rng.uniform(-200, 200 - H * cs)))
    span = np.array([W * cs, H * cs])
    place = lambda: np.array(origin) + rng.uniform(-0.3, 1.3, 2) * span
    rings = [convex_ring(rng, place(), rng.uniform(0.05, 0.25) * span.max()) for _ in range(n_rings)]
    parts = [(0.0, 0.0, 0.0, SHAPE_OBB, 4.0, 2.0, 1)]   # slot 0: the ego, at the window's centre below
    parts[0] = (origin[0] + 0.5 * span[0], origin[1] + 0.5 * span[1], rng.uniform(-np.pi, np.pi), SHAPE_OBB, 4.0, 2.0, 1)
    for _ in range(n_boxes):
        c = place()
        parts.append((c[0], c[1], rng.uniform(-7, 7), SHAPE_OBB, rng.uniform(0.1, 0.4) * span.max(), rng.uniform(0.05, 0.2) * span.max(), 1))
    for _ in range(n_discs):
        c = place()
        parts.append((c[0], c[1], rng.uniform(-3, 3), SHAPE_CIRCLE, 0.6, rng.uniform(0.05, 0.3) * span.max(), 1))
    parts = [tuple(float(np.float32(v)) if i < 3 else v for i, v in enumerate(p)) for p in parts]
    return scene(H, W, cs, origin, infl, rings, parts, include_participants=True, exclude_slot=0)


def random_scenes():
    """every cell size x every inflate, twice"""
    return [random_scene(seed) for seed in range(18)]


# ---- contact scenes: dyadic coordinates (multiples of 2^-8 below 2^10), every product of the specification exact --------------
CS, ORIGIN = 0.5, (3.25, -2.5)
CELL = (2, 3)   # (row, col) the contact is made with; its faces:
X0, X1 = ORIGIN[0] + CELL[1] * CS - CS / 2, ORIGIN[0] + CELL[1] * CS + CS / 2
Y0, Y1 = ORIGIN[1] + CELL[0] * CS - CS / 2, ORIGIN[1] + CELL[0] * CS + CS / 2
Q = 1.0 / 16


def _up(x):
    """one fp32 ulp further from zero along +x"""
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


def contact_scenes():
    out = []

    def add(name, rings, inflate, occupied):
        out.append(scene(5, 7, CS, ORIGIN, inflate, rings, cell=CELL, occupied=occupied, name=name))

    for shift, tag, occ in ((lambda x: x, "", True), (_up, " + 1 ulp", False)):
        # a ring edge lying exactly on the cell's right edge
        xe = shift(X1)
        add("edge on a cell edge" + tag, [[(xe, Y0 - 1), (xe + 2, Y0 - 1), (xe + 2, Y1 + 1), (xe, Y1 + 1)]], 0.0, occ)
        # a vertex exactly on the cell's upper right corner
        add("vertex on a cell corner" + tag, [[(shift(X1), Y1), (X1 + 1, Y1 + 0.5), (X1 + 0.5, Y1 + 1)]], 0.0, occ)
        # a ring exactly inflate = 1/4 from the right face (an edge longer than the cell, parallel to the face) ...
        xe = shift(X1 + 0.25)
        add("inflate from a cell face" + tag, [[(xe, Y0 - 1), (xe + 2, Y0 - 1), (xe + 2, Y1 + 1), (xe, Y1 + 1)]], 0.25, occ)
        # ... and exactly inflate = 5 q from the upper right corner: the 3-4-5 offset makes the distance rational
        add("inflate from a cell corner" + tag, [[(shift(X1 + 3 * Q), Y1 + 4 * Q), (X1 + 3 * Q + 1, Y1 + 4 * Q + 0.5), (X1 + 3 * Q + 0.5, Y1 + 4 * Q + 1)]],
            5 * Q, occ)
        # an oblique edge at exactly inflate from the corner: the edge through (3 q, 4 q) + corner with direction (4, -3)
        px, py = X1 + 3 * Q, Y1 + 4 * Q
        add("oblique edge inflate from a cell corner" + tag,
            [[(shift(px - 4 * Q), py + 3 * Q), (shift(px + 4 * Q), py - 3 * Q), (shift(px + 4 * Q + 1), py - 3 * Q + 1)]], 5 * Q, occ)
    cx, cy = X0 + CS / 2, Y0 + CS / 2
    add("a ring strictly inside one cell", [[(cx - Q, cy - Q), (cx + Q, cy - Q), (cx, cy + Q)]], 0.0, True)
    add("a cell strictly inside a ring", [[(X0 - 0.75, Y0 - 0.75), (X1 + 0.75, Y0 - 0.75), (X1 + 0.75, Y1 + 0.75), (X0 - 0.75, Y1 + 0.75)]], 0.0, True)
    add("a cell strictly inside a clockwise ring", [[(X0 - 0.75, Y1 + 0.75), (X1 + 0.75, Y1 + 0.75), (X1 + 0.75, Y0 - 0.75), (X0 - 0.75, Y0 - 0.75)]], 0.0, True)
    # a sliver crossing the cell with no vertex inside it and no corner of the cell inside the sliver
    add("a sliver through a cell", [[(X0 - 1, cy - Q), (X1 + 1, cy - Q / 2), (X1 + 1, cy + Q / 2)]], 0.0, True)
    return out
