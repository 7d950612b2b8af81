"""Contact-dense scenes for the real event kernels (tests/test_gpu_geom_scenes.py), built from fp32 POSES whose candidate pairs sit
in the undecided band of the certifying filters -- what random scenes at tens of metres reach with negligible probability.

Everything lives within |x|, |y| <= 4 m, where an fp32 ulp (<= 2.4e-7 m) is below the band of rect_pair_filter (1e-6 / (2 L) =
2e-6 m for the 0.25-m boxes here), sizes and positions are dyadic so that `contact` is exact, and headings are 0 (the only fp32
heading whose sine and cosine are exact) or general.  An env is a grid of cells; a cell holds one motif and nothing of a neighbouring
cell reaches it, so that every verdict is the motif's own.

    pair_scene(O, n_env, A, kind)   two participants per cell, no map: the pair stage.  kind "saturated": nearly every pair in
                                    contact; "mixed": most pairs clearly apart or deep in each other, a third in contact -- waves
                                    that hold decided and undecided lanes together
    map_scene(n_env, A)             one participant per cell against its own static polygon (3 .. 8 vertices), the outline of the
                                    lane union, or the boundary rectangle
    iou_scene(n_env, A)             egos on, beside and identical to their target areas, at zero speed
Scenes are the dicts of helpers.random_scene (helpers.gpu_collide / oracle_collide take them) plus "motif": the name of every
participant's motif, and for pair scenes "pairs": [k, 2] participant indices of the box pairs with "contact": bool [k].
"""
import numpy as np

PITCH = 0.75
U = 1.0 / 64
# type rows (shape columns as helpers.shape_rows): boxes <= 0.25 m, discs of radius 5/64 and 1/16
BOXES = [(0.25, 0.125), (0.125, 0.25), (0.25, 0.25), (0.125, 0.125), (0.125, 0.0625)]
DISCS = [5 * U * 2, 0.125]
T_DISC5, T_DISC4 = len(BOXES), len(BOXES) + 1
_cache = {}


def rows():
    out = []
    for (L_, W_) in BOXES:
        r = np.zeros(24); r[0] = 0; r[1] = 1.2; r[2] = 1.3; r[3] = 2.5; r[17] = 5; r[18] = 0; r[19] = L_; r[20] = W_
        out.append(r)
    for W_ in DISCS:
        r = np.zeros(24); r[0] = 2; r[17] = 5; r[18] = 1; r[19] = W_; r[20] = W_
        out.append(r)
    return np.array(out)


def _cells(n, pitch):
    g = int(np.ceil(np.sqrt(n)))
    k = np.arange(n)
    return g, ((k % g) - (g - 1) / 2) * pitch, ((k // g) - (g - 1) / 2) * pitch


def _ulps(v, k):
    """the fp32 value k ulps from v"""
    v = np.float32(v)
    for _ in range(abs(int(k))):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf))
    return v


def _scene(n_env, A, x, y, h, tid, active, motif, **kw):
    sc = dict(rows=rows(), n_env=n_env, A=A, x=np.float32(x).reshape(-1), y=np.float32(y).reshape(-1), heading=np.float32(h).reshape(-1),
              type_id=np.uint8(tid).reshape(-1), active=np.uint8(active).reshape(-1), static=None, lanes=None, boundary=None,
              boundary_valid=None, motif=np.array(motif, dtype=object).reshape(-1))
    sc.update(kw)
    assert np.abs(sc["x"]).max() <= 4.0 and np.abs(sc["y"]).max() <= 4.0
    return sc


# --------------------------------------------------------------------------------------------------------------- the pair stage
def pair_scene(O, n_env, A, kind, seed=0):
    key = ("pair", n_env, A, kind, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng([seed, n_env, A, kind == "mixed"])
    R = rows()
    npair = A // 2
    g, cx, cy = _cells(npair, PITCH)
    N = n_env * A
    x = np.zeros((n_env, A), np.float32); y = np.zeros((n_env, A), np.float32); h = np.zeros((n_env, A), np.float32)
    tid = np.zeros((n_env, A), np.uint8); active = np.ones((n_env, A), np.uint8)
    motif = np.full((n_env, A), "", dtype=object)
    if A % 2:
        active[:, -1] = 0
    contact_kinds = ["edge", "swept", "corner", "corner_swept", "general_in", "general_out", "disc_disc", "disc_side", "disc_corner"]
    p_contact = np.array([0.2, 0.2, 0.1, 0.06, 0.12, 0.12, 0.06, 0.07, 0.07])
    decided_kinds = ["apart", "deep", "apart_general", "deep_general"]
    general = []            # (env, pair) of the motifs bisected below
    for e in range(n_env):
        for p in range(npair):
            i, j = 2 * p, 2 * p + 1
            if kind == "saturated" or rng.random() < 0.3:
                m = contact_kinds[rng.choice(len(contact_kinds), p=p_contact)]
            else:
                m = decided_kinds[rng.integers(0, 4)]
            motif[e, i] = motif[e, j] = m
            ta, tb = rng.integers(0, 3, 2)                               # boxes of 0.25 / 0.125 m
            if "general" in m:
                ta, tb = rng.integers(3, 5, 2)                           # (0.125 m and less: b stays inside the cell wherever it turns)
            (La, Wa), (Lb, Wb) = BOXES[ta], BOXES[tb]
            tid[e, i], tid[e, j] = ta, tb
            X, Y = cx[p], cy[p]
            vert = rng.random() < 0.5                                    # stacked in y instead of side by side in x
            half_a, half_b = (Wa / 2, Wb / 2) if vert else (La / 2, Lb / 2)
            slide = rng.integers(-3, 4) * U                              # along the shared side
            if m in ("edge", "swept", "apart", "deep"):
                k = {"edge": 0, "swept": int(rng.integers(-8, 9)), "apart": 0, "deep": 0}[m]
                extra = {"apart": rng.integers(4, 7) * U, "deep": -rng.integers(2, 6) * U}.get(m, 0.0)
                a0, b0 = -half_a, half_b + extra                         # a's far side of the contact line at 0, b's near side at 0
                if vert:
                    x[e, i], y[e, i] = X, Y + a0; x[e, j], y[e, j] = X + slide, _ulps(Y + b0, k)
                else:
                    x[e, i], y[e, i] = X + a0, Y; x[e, j], y[e, j] = _ulps(X + b0, k), Y + slide
            elif m in ("corner", "corner_swept"):
                k = 0 if m == "corner" else int(rng.integers(-8, 9))
                x[e, i], y[e, i] = X - La / 2, Y - Wa / 2
                x[e, j], y[e, j] = _ulps(X + Lb / 2, k), _ulps(Y + Wb / 2, k if rng.random() < 0.5 else 0)
            elif m in ("general_in", "general_out", "apart_general", "deep_general"):
                x[e, i], y[e, i] = X, Y
                h[e, i], h[e, j] = rng.uniform(0, 2 * np.pi, 2)
                general.append((e, p, rng.uniform(0, 2 * np.pi)))
            else:
                tid[e, j] = T_DISC5
                if m == "disc_disc":                                     # 3-4-5: dx^2 + dy^2 == (r + r)^2 exactly
                    tid[e, i] = T_DISC5
                    x[e, i], y[e, i] = X - 3 * U, Y - 4 * U; x[e, j], y[e, j] = X + 3 * U, Y + 4 * U
                elif m == "disc_side":                                   # tangent to the box's front side
                    x[e, i], y[e, i] = X - La / 2, Y; x[e, j], y[e, j] = X + 5 * U, Y + slide * (abs(slide) <= Wa / 2)
                else:                                                    # 3-4-5 from the box's front-left corner
                    x[e, i], y[e, i] = X - La / 2, Y - Wa / 2; x[e, j], y[e, j] = X + 3 * U, Y + 4 * U
                k = int(rng.integers(-2, 3))                             # a couple of ulps either way, half of them exact
                if rng.random() < 0.5:
                    x[e, j] = _ulps(x[e, j], k)
    # general angles: b slid from a along a direction, bisected until two neighbouring fp32 poses bracket contact
    if general:
        ge = np.array([q[0] for q in general]); gp = np.array([q[1] for q in general]); t = np.array([q[2] for q in general])
        ia, ib = 2 * gp, 2 * gp + 1
        dims = np.array(BOXES)
        La, Wa = dims[tid[ge, ia]].T; Lb, Wb = dims[tid[ge, ib]].T
        xa, ya, ha, hb = x[ge, ia], y[ge, ia], h[ge, ia], h[ge, ib]

        def pose(xs, ys, hs, Ls, Ws):
            return np.stack([O.pose_obb(xs[q], ys[q], hs[q], Ls[q], Ws[q], trig=0).reshape(8) for q in range(len(xs))])
        PA = pose(xa, ya, ha, La, Wa)

        def at(s):
            return np.float32(np.float64(xa) + s * np.cos(t)), np.float32(np.float64(ya) + s * np.sin(t))
        lo, hi = np.zeros(len(t)), np.full(len(t), 0.5)
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            xm, ym = at(mid)
            hit = O.geom("sat_quads", PA, pose(xm, ym, hb, Lb, Wb)) != 0
            lo = np.where(hit, mid, lo); hi = np.where(hit, hi, mid)
        m = motif[ge, ia]
        s = np.where(m == "general_in", lo, np.where(m == "general_out", hi, np.where(m == "apart_general", hi + 0.06, 0.5 * lo)))
        x[ge, ib], y[ge, ib] = at(s)
    sc = _scene(n_env, A, x, y, h, tid, active, motif)
    base = (np.arange(n_env) * A)[:, None] + 2 * np.arange(npair)[None, :]
    is_box = (R[tid[:, 0:2 * npair:2], 18] == 0) & (R[tid[:, 1:2 * npair:2], 18] == 0)
    sc["pairs"] = np.stack([base[is_box], base[is_box] + 1], 1)
    sc["contact"] = np.isin(motif[:, 0:2 * npair:2][is_box], contact_kinds)
    _cache[key] = sc
    return sc


def pair_vertices(O, sc):
    """the oracle's vertices of both boxes of every box pair: [k, 8] each (deterministic trig: what the kernels and oracle.collide use)"""
    R = sc["rows"]

    def verts(idx):
        return np.stack([O.pose_obb(sc["x"][i], sc["y"][i], sc["heading"][i], R[sc["type_id"][i], 19], R[sc["type_id"][i], 20], trig=0).reshape(8)
                         for i in idx])
    return verts(sc["pairs"][:, 0]), verts(sc["pairs"][:, 1])


# ------------------------------------------------------------------------------------- statics, lane outline, boundary rectangle
MAP_PITCH = 0.5
# convex CCW polygons of 3 .. 8 vertices in units of 1/64 m: a vertical left edge x = -4 (last vertex -> first), one rightmost vertex (6, 0)
POLYGONS = {3: [(-4, -4), (6, 0), (-4, 4)],
            4: [(-4, -4), (2, -4), (6, 0), (-4, 4)],
            5: [(-4, -4), (2, -4), (6, 0), (2, 4), (-4, 4)],
            6: [(-4, -4), (0, -5), (4, -3), (6, 0), (4, 3), (-4, 4)],
            7: [(-4, -4), (0, -5), (4, -3), (6, 0), (4, 3), (0, 5), (-4, 4)],
            8: [(-4, -4), (0, -5), (4, -3), (6, 0), (4, 3), (0, 5), (-3, 5), (-4, 4)]}


def map_scene(n_env, A, seed=0, far_lanes=0, ego=False):
    """ego: a scene the wave-per-env ego kernel takes (A = 1, boxes only -- in the type table too --, no lanes).  far_lanes: that many extra lane polygons per env 300 m to the side of everything (they change no verdict), which push the
    env's geometry out of the LDS record into the HBM grid tier"""
    rng = np.random.default_rng([seed, n_env, A, 7])
    g, cx, cy = _cells(A, MAP_PITCH)
    assert g * MAP_PITCH <= 8.0
    x = np.zeros((n_env, A), np.float32); y = np.zeros((n_env, A), np.float32); h = np.zeros((n_env, A), np.float32)
    tid = np.zeros((n_env, A), np.uint8); motif = np.full((n_env, A), "", dtype=object)
    statics, lanes = [], []
    half = g * MAP_PITCH / 2
    boundary = np.tile(np.float32([-half, half, -half, half]), (n_env, 1))
    col, row = np.arange(A) % g, np.arange(A) // g
    outer = (col == 0) | (col == g - 1) | (row == 0) | (row == g - 1)
    for e in range(n_env):
        st, ln = [], []
        for c in range(A):
            X, Y = cx[c], cy[c]
            t = int(rng.integers(3, 5)); L_, W_ = BOXES[t]        # 0.125 x 0.125 or 0.125 x 0.0625
            disc = rng.random() < 0.15 and not ego
            # ulps off exact contact: 0, 1 or 2 the one way for four in ten, 1 or 2 the other way for the rest
            k = int(rng.integers(1, 3)) if rng.random() < 0.6 else -int(rng.integers(0, 3))
            if g == 1:
                pick = ("boundary", "static", "lane")[e % (2 if ego else 3)]
            elif outer[c] and rng.random() < (0.9 if g >= 6 else 0.4):
                pick = "boundary"
            else:
                pick = "static" if rng.random() < 0.55 else "lane"
            if pick == "boundary":
                # the boundary rectangle touched from inside (k <= 0 on the far side: contained) or crossed by k ulps
                sx = 1 if col[c] == g - 1 else (-1 if col[c] == 0 else 0)
                sy = 0 if sx else (1 if row[c] == g - 1 else -1)
                if g == 1:
                    sx, sy = 1, 0
                ext = (0.125 / 2 if disc else (L_ / 2 if sx else W_ / 2))
                px = _ulps(sx * (half - ext), k * sx) if sx else X + rng.integers(-4, 5) * U
                py = _ulps(sy * (half - ext), k * sy) if sy else Y + rng.integers(-4, 5) * U
                m = "boundary"
                full_lane = True
            elif pick == "static":
                nv = int(rng.integers(3, 9))
                pc = np.array([X - 2 * U, Y])
                st.append(np.float32(np.array(POLYGONS[nv]) * U + pc))
                ext = 0.125 / 2 if disc else L_ / 2
                way = rng.integers(0, 3)
                if way == 0:       # its side (or the disc) on the polygon's rightmost vertex
                    px, py, m = _ulps(pc[0] + 6 * U + ext, k), Y + rng.integers(-1, 2) * U, "static_vertex"
                elif way == 1:     # along the polygon's left edge
                    px, py, m = _ulps(pc[0] - 4 * U - ext, k), Y + rng.integers(-2, 3) * U, "static_edge"
                else:              # its centre on the left edge's line: the boundary of the `intersecting` certificate
                    px, py, m = _ulps(pc[0] - 4 * U, k), Y + rng.integers(-2, 3) * U, "static_centre_on_edge"
                full_lane = True
            else:
                # the cell's lane stops 1/8 m short of the cell's right side: an outer piece of the union's outline at X + 1/8
                ext = 0.125 / 2 if disc else L_ / 2
                way = rng.integers(0, 4)
                edge = X + 0.125
                if way == 0:
                    px, m = _ulps(edge - ext, k), "lane_inside"            # side along the piece from inside: contained unless k > 0
                elif way == 1:
                    px, m = _ulps(edge + ext, k), "lane_outside"           # in the gap: its centre is in no lane
                elif way == 2:
                    px, m = X - 0.25 + rng.integers(-2, 3) * U, "lane_across_shared_side"   # over the side shared with the left neighbour
                else:
                    px, m = edge, "lane_centre_on_outline"
                py = Y + rng.integers(-4, 5) * U
                full_lane = False
            x1 = X + 0.25 if full_lane else X + 0.125
            ln.append(np.float32([[X - 0.25, Y - 0.25], [x1, Y - 0.25], [x1, Y + 0.25], [X - 0.25, Y + 0.25]]))
            x[e, c], y[e, c], motif[e, c] = px, py, m
            tid[e, c] = T_DISC4 if disc else t
        for q in range(far_lanes):
            x0 = 300.0 + (q % 16) * 0.125; y0 = (q // 16) * 0.125
            ln.append(np.float32([[x0, y0], [x0 + 0.0625, y0], [x0 + 0.0625, y0 + 0.0625], [x0, y0 + 0.0625]]))
        statics.append(st); lanes.append(ln)
    import helpers as H
    sc = _scene(n_env, A, x, y, h, tid, np.ones((n_env, A), np.uint8), motif, static=H.to_csr(statics), lanes=H.to_csr(lanes),
                boundary=boundary, boundary_valid=np.ones(n_env, np.uint8))
    if ego:
        assert A == 1
        sc["rows"], sc["lanes"] = sc["rows"][:len(BOXES)], None
    return sc


# ----------------------------------------------------------------------------------------------------------- IoU in the kernels
def iou_scene(n_env, A, seed=0):
    """(x, y, heading of the ego of every env, target [n_env, 4, 2] fp32, name of every env's case): a 0.5 x 0.25 ego (type row 0 of
    iou_rows) against its target -- identical to it, nested with collinear sides, beside it along a side or at a corner (IoU exactly
    0), shifted along a side, across it, moved by micrometres (the NoAction regime against the first pose is the kernels' own), in a
    slightly larger bay -- axis-parallel with dyadic numbers and at general angles rounded to fp32 poses"""
    rng = np.random.default_rng([seed, n_env, A, 11])
    L_, W_ = 0.5, 0.25
    names = ["identical", "identical_general", "shared_side_front", "shared_side_left", "shared_side_rear", "shared_side_right",
             "shared_corner", "nested", "shifted_along_side", "cross", "moved_um", "bay", "bay_general", "apart"]
    x = np.zeros(n_env, np.float32); y = np.zeros(n_env, np.float32); h = np.zeros(n_env, np.float32)
    tgt = np.zeros((n_env, 4, 2), np.float32); case = []

    def rect(x0, y0, w, hh):
        return np.float32([[x0, y0], [x0 + w, y0], [x0 + w, y0 + hh], [x0, y0 + hh]])

    def box(cx_, cy_, th, l, w):
        c, s = np.cos(th), np.sin(th)
        loc = np.array([[l / 2, -w / 2], [l / 2, w / 2], [-l / 2, w / 2], [-l / 2, -w / 2]])
        return np.float32(loc @ np.array([[c, s], [-s, c]]) + [cx_, cy_])
    for e in range(n_env):
        m = names[e % len(names)]
        X, Y = rng.integers(-192, 193, 2) * U            # |x| <= 3 m, dyadic
        x[e], y[e] = X, Y
        x0, y0 = X - L_ / 2, Y - W_ / 2                  # the ego's rear-right corner at heading 0
        if m == "identical":
            T = rect(x0, y0, L_, W_)
        elif m in ("identical_general", "moved_um", "bay_general"):
            h[e] = np.float32(rng.uniform(0, 2 * np.pi))
            d = rng.normal(0, 2e-6, 2) if m == "moved_um" else np.zeros(2)
            T = box(X + d[0], Y + d[1], float(h[e]), *((L_ + 0.125, W_ + 0.0625) if m == "bay_general" else (L_, W_)))
        elif m == "shared_side_front":
            T = rect(x0 + L_, y0 + rng.integers(-8, 9) * U, 0.5, 0.25)
        elif m == "shared_side_rear":
            T = rect(x0 - 0.5, y0 + rng.integers(-8, 9) * U, 0.5, 0.25)
        elif m == "shared_side_left":
            T = rect(x0 + rng.integers(-8, 9) * U, y0 + W_, 0.5, 0.25)
        elif m == "shared_side_right":
            T = rect(x0 + rng.integers(-8, 9) * U, y0 - 0.25, 0.5, 0.25)
        elif m == "shared_corner":
            T = rect(x0 + L_, y0 + W_, 0.5, 0.25)
        elif m == "nested":
            T = rect(x0, y0, L_ + 0.25, W_ + 0.125)       # two sides collinear with the bay's
        elif m == "shifted_along_side":
            T = rect(x0 + 0.0625, y0, L_, W_)             # 7 / 9
        elif m == "cross":
            T = rect(X - W_ / 2, Y - L_ / 2, W_, L_)
        elif m == "bay":
            T = rect(x0 - 4 * U, y0 - 2 * U, L_ + 8 * U, W_ + 4 * U)
        else:
            T = rect(x0 + 1.0, y0, L_, W_)
        if rng.random() < 0.5:
            T = np.roll(T, int(rng.integers(0, 4)), axis=0)
        tgt[e] = T; case.append(m)
    return x, y, h, tgt, np.array(case)


def iou_rows():
    r = rows()[:len(BOXES)]           # (boxes only: a type table with a disc in it keeps a single-ego pool off the ego kernel)
    r[0, 19], r[0, 20] = 0.5, 0.25
    return r
