"""fp64 numpy restatement of the BEV camera's definition (include/t2d.h "BEV camera") -- TEST INFRASTRUCTURE,
never imported by the product.

What is restated:
  view window   x in [sx - left, sx + right], y in [sy - back, sy + front], then the short side widened about the centre to the
                image's aspect ratio height / width (MatplotlibRenderer._calculate_bounds / auto_scale)
  transform     v = R(+camera_yaw) (p - sensor) + sensor (MatplotlibRenderer._transform_to_camera_view); an agent of heading h
                points to the front for camera_yaw = pi / 2 - h
  draw order    stable sort of the listing by z-order: the topmost element containing a pixel centre is the one with the
                largest (z, listing position)
  listing       areas (the target, then the obstacles), lanes, then participants by slot, each body followed by its heading
                triangle (midpoints of edges 0-1, 1-2, 3-0 of the body ring); a pedestrian is a disc; inactive ones are skipped
  raster        pixel (r, c) = class of the topmost element containing the pixel CENTRE, row 0 at the front (max y) edge;
                even-odd crossing on the undivided ring, dx^2 + dy^2 <= r^2 for discs

render() also returns, per pixel, the distance from the pixel centre to the nearest element edge (capped: distances beyond
`dist_cap` are reported as inf), so that a test can leave out the pixels a rounding error may flip.
"""
import numpy as np

CLASS_NAMES = ("background", "lane", "obstacle", "target_area", "vehicle", "cyclist", "pedestrian", "heading_arrow")
BACKGROUND, LANE, OBSTACLE, TARGET, VEHICLE, CYCLIST, PEDESTRIAN, ARROW = range(8)
Z_ORDER = (0, 3, 5, 1, 1, 6, 1, 7)
SHAPE_OBB, SHAPE_CIRCLE = 0, 1


def window(perception_range, window_size, sensor=(0.0, 0.0)):
    """(x_min, x_max, y_min, y_max) of the view around `sensor`; window_size = (width, height)"""
    left, right, front, back = [float(v) for v in perception_range]
    sx, sy = float(sensor[0]), float(sensor[1])
    x0, x1, y0, y1 = sx - left, sx + right, sy - back, sy + front
    ww, wh = x1 - x0, y1 - y0
    cx, cy = (x0 + x1) / 2, (y0 + y1) / 2
    res_aspect = window_size[1] / window_size[0]
    if wh / ww > res_aspect:
        nw, nh = wh / res_aspect, wh
    else:
        nw, nh = ww, ww * res_aspect
    return cx - nw / 2, cx + nw / 2, cy - nh / 2, cy + nh / 2


def to_camera_view(points, sensor, yaw):
    """v = R(+yaw) (p - sensor) + sensor"""
    p = np.asarray(points, np.float64) - np.asarray(sensor, np.float64)
    c, s = np.cos(yaw), np.sin(yaw)
    return np.stack([p[..., 0] * c - p[..., 1] * s, p[..., 0] * s + p[..., 1] * c], axis=-1) + np.asarray(sensor, np.float64)


def camera_yaw(heading, heading_up=True):
    return np.pi / 2 - float(heading) if heading_up else 0.0


def body_ring(x, y, heading, length, width):
    """Vehicle / Cyclist body ring at a pose (the vertex order of `geometry`), and its heading triangle"""
    hl, hw = 0.5 * length, 0.5 * width
    local = np.array([[hl, -hw], [hl, hw], [-hl, hw], [-hl, -hw]])
    tri = np.array([(local[0] + local[1]) / 2, (local[1] + local[2]) / 2, (local[3] + local[0]) / 2])
    c, s = np.cos(heading), np.sin(heading)
    rot = np.array([[c, -s], [s, c]])
    return local @ rot.T + (x, y), tri @ rot.T + (x, y)


def elements(target=None, static=(), lanes=(), tiles=(), participants=(), arrows=True, z_order=Z_ORDER):
    """The listing of one env, world frame: dicts(kind, cls, z, xy | (centre, r)).  participants: iterable of
    (x, y, heading, shape, length, width, active, cls) in slot order."""
    out = []
    poly = lambda xy, cls: out.append(dict(kind="polygon", cls=cls, z=z_order[cls], xy=np.asarray(xy, np.float64).reshape(-1, 2)))
    if target is not None:
        poly(target, TARGET)
    for r in static:
        poly(r, OBSTACLE)
    for r in lanes:
        poly(r, LANE)
    for r in tiles:
        poly(r, LANE)
    for x, y, h, shape, length, width, active, cls in participants:
        if not active or cls == BACKGROUND or not np.all(np.isfinite([x, y, h])):
            continue
        if shape == SHAPE_CIRCLE:
            out.append(dict(kind="circle", cls=cls, z=z_order[cls], centre=np.array([x, y], np.float64), r=max(0.5 * width, 0.0)))
        else:
            ring, tri = body_ring(x, y, h, length, width)
            poly(ring, cls)
            if arrows:
                poly(tri, ARROW)
    return out


def _even_odd(xy, px, py):
    inside = np.zeros(px.shape, bool)
    n = len(xy)
    for k in range(n):
        x1, y1 = xy[k - 1]
        x2, y2 = xy[k]
        cross = (y1 > py) != (y2 > py)
        if y1 != y2:
            t = x1 + (x2 - x1) * (py - y1) / (y2 - y1)
            inside ^= cross & (px < t)
    return inside


def _seg_dist(xy, px, py):
    d = np.full(px.shape, np.inf)
    n = len(xy)
    for k in range(n):
        a, b = xy[k - 1], xy[k]
        ab = b - a
        L2 = ab @ ab
        if L2 == 0.0:
            t = np.zeros(px.shape)
        else:
            t = np.clip(((px - a[0]) * ab[0] + (py - a[1]) * ab[1]) / L2, 0.0, 1.0)
        d = np.minimum(d, np.hypot(px - (a[0] + t * ab[0]), py - (a[1] + t * ab[1])))
    return d


def render(elems, window_size, win, sensor, yaw, dist_cap=1.0):
    """class image uint8 [H, W] and edge distance float64 [H, W] (inf beyond dist_cap) of a listing, elements in the WORLD
    frame; win = window(...) around the sensor."""
    W, H = window_size
    x0, x1, y0, y1 = win
    pw, ph = (x1 - x0) / W, (y1 - y0) / H
    cx = x0 + (np.arange(W) + 0.5) * pw
    cy = y1 - (np.arange(H) + 0.5) * ph
    cls = np.zeros((H, W), np.uint8)
    key = np.full((H, W), -1, np.int64)
    dist = np.full((H, W), np.inf)
    for pos, el in enumerate(elems):
        k = el["z"] * (1 << 32) + pos
        if el["kind"] == "circle":
            c = to_camera_view(el["centre"], sensor, yaw)
            lo, hi = c - el["r"], c + el["r"]
        else:
            v = to_camera_view(el["xy"], sensor, yaw)
            lo, hi = v.min(axis=0), v.max(axis=0)
        # the pixels whose centre can be inside, or within dist_cap of the boundary
        c0 = max(int(np.floor((lo[0] - dist_cap - x0) / pw)) - 1, 0)
        c1 = min(int(np.ceil((hi[0] + dist_cap - x0) / pw)) + 1, W)
        r0 = max(int(np.floor((y1 - hi[1] - dist_cap) / ph)) - 1, 0)
        r1 = min(int(np.ceil((y1 - lo[1] + dist_cap) / ph)) + 1, H)
        if c0 >= c1 or r0 >= r1:
            continue
        px, py = np.meshgrid(cx[c0:c1], cy[r0:r1])
        if el["kind"] == "circle":
            rr = np.hypot(px - c[0], py - c[1])
            inside = (px - c[0]) ** 2 + (py - c[1]) ** 2 <= el["r"] ** 2
            d = np.abs(rr - el["r"])
        else:
            inside = _even_odd(v, px, py)
            d = _seg_dist(v, px, py)
        sub_d = dist[r0:r1, c0:c1]
        np.minimum(sub_d, np.where(d <= dist_cap, d, np.inf), out=sub_d)
        sub_k, sub_c = key[r0:r1, c0:c1], cls[r0:r1, c0:c1]
        take = inside & (k > sub_k)
        sub_k[take] = k
        sub_c[take] = el["cls"]
    return cls, dist


def render_pose(elems, window_size, perception_range, x, y, heading, heading_up=True, dist_cap=1.0):
    """render() for a camera bound to a participant at (x, y, heading)"""
    if not np.all(np.isfinite([x, y, heading])):
        return np.zeros((window_size[1], window_size[0]), np.uint8), np.full((window_size[1], window_size[0]), np.inf)
    return render(elems, window_size, window(perception_range, window_size, (x, y)), (x, y), camera_yaw(heading, heading_up), dist_cap)
