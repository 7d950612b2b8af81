#!/usr/bin/env python3
"""Golden data for the BEV camera -> camera.npz, camera_style.json, made by RUNNING the reference's own code.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script

  * puts stand-ins into sys.modules for what is not available to this build or is only a holder of data:
      shapely.geometry     Point (x, y, coords, distance), Polygon (exterior.coords, interiors, distance), LinearRing (coords,
                           closed; distance) -- `distance` is only asked by BEVCamera._in_perception_range, whose answer never
                           changes a pixel (the farthest window corner is sqrt(2) x the largest range away, the cut is at 1.5 x);
      tactics2d.map.element, tactics2d.participant.element
                           plain holders with the attributes BEVCamera reads: Area / Lane (id_, geometry, type_, subtype, color),
                           Junction, RoadLine, Map (junctions, areas, lanes, roadlines dicts); Vehicle / Cyclist (id_, type_,
                           color, geometry = the body ring in the reference's vertex order, get_pose, trajectory.get_state),
                           Pedestrian (get_pose -> (location, radius)), Obstacle.  Default type_ names and colours are the
                           reference's (vehicle.py:78-82, cyclist.py:56-58, pedestrian.py:49-52, generate_parking_lot.py:40,114,122,
                           generate_racing_track.py:181-185);
  * loads from their FILES, unmodified: sensor/sensor_base.py, sensor/camera.py (BEVCamera: update, _get_map_elements,
    _get_participants are EXECUTED for every scene), renderer/matplotlib_config.py and renderer/matplotlib_renderer.py
    (MatplotlibRenderer: update, auto_scale, _calculate_bounds, _transform_to_camera_view, _resolve_style, on matplotlib's Agg
    backend).

Per scene the reference renderer draws the geometry dicts BEVCamera produced; the figure's dpi is raised to DPI (the
reference never applies its own `dpi`, so its canvas would be 100 x 100) and the canvas is sampled at the centres of the
W x H grid over the axes limits auto_scale left -- through the axes' own data transform.

camera.npz
    class_names order is camera_style.json's.  Scenes s = 0 .. S - 1:
    scene_name, sensor [S, 2], heading [S] (of the bound agent), yaw [S] (= the camera_yaw handed over), prange [S, 4] (left,
    right, front, back), wsize [S, 2] (width, height), xlim / ylim [S, 2] (after auto_scale), scene_elem_off [S + 1];
    elements in listing order (map elements, then participants): elem_shape (0 polygon, 1 circle), elem_class, elem_z and
    elem_rgb (what _resolve_style gave THIS element), elem_drawn (0: MatplotlibRenderer.update skipped the element because it
    already held its id -- the parking target behind the back wall, see parking_map), elem_pos [N, 2] / elem_rot [N] ("position" / "rotation" of a participant
    dict; 0 for map elements), elem_radius, elem_vert_off [N + 1], elem_xy (the dict's "geometry" as listed: world frame for map
    elements, body frame for participants; a closing duplicate vertex dropped);
    rgb_<s> uint8 [H, W, 3]: the reference's colours at the pixel centres, row 0 at the top (max y).
    Rules recorded from the reference's functions: probe_heading [K], probe_front [K, 2] = _transform_to_camera_view of the
    unit vector (cos h, sin h) about the origin with camera_yaw = pi / 2 - h; probe_yaw, probe_rot [2] = the same function on
    (1, 0) with camera_yaw = probe_yaw; scalar_range [4] = BEVCamera(..., perception_range=25.0).perception_range.
camera_style.json
    class_names; per class rgb and z as _resolve_style resolved them, the (color key, type key) that were resolved, and the
    background = the figure's face colour.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_camera.py --ref REFERENCE_TREE [--out DIR]

The files are written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import importlib.util
import io
import json
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
DPI = 800
CLASS_NAMES = ("background", "lane", "obstacle", "target_area", "vehicle", "cyclist", "pedestrian", "heading_arrow")
TYPE_TO_CLASS = {"road": "lane", "obstacle": "obstacle", "target_area": "target_area", "medium_car": "vehicle", "cyclist": "cyclist",
                 "adult_male": "pedestrian", "heading_arrow": "heading_arrow"}


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


# ------------------------------------------------------------------------------------------------ shapely stand-ins
def _ring_distance(coords, p):
    v = np.asarray(coords, float)
    a, b = v, np.roll(v, -1, axis=0)
    ab = b - a
    L2 = np.maximum((ab * ab).sum(axis=1), 1e-300)
    t = np.clip(((p - a) * ab).sum(axis=1) / L2, 0.0, 1.0)
    return float(np.min(np.hypot(*(p - (a + t[:, None] * ab)).T)))


class Point:
    def __init__(self, *a):
        x, y = a if len(a) == 2 else a[0]
        self.x, self.y = float(x), float(y)
        self.coords = [(self.x, self.y)]

    def distance(self, other):
        return float(np.hypot(self.x - other.x, self.y - other.y))


class LinearRing:
    def __init__(self, coordinates):
        c = [(float(x), float(y)) for x, y in coordinates]
        if c[0] != c[-1]:
            c.append(c[0])
        self.coords = c

    def distance(self, point):
        return _ring_distance(self.coords[:-1], np.array([point.x, point.y]))


class Polygon:
    def __init__(self, shell):
        self.exterior = LinearRing(shell.coords if hasattr(shell, "coords") else shell)
        self.interiors = []

    def distance(self, point):
        v = np.array(self.exterior.coords[:-1])
        x, y = point.x, point.y
        inside = False
        for k in range(len(v)):
            (x1, y1), (x2, y2) = v[k - 1], v[k]
            if (y1 > y) != (y2 > y) and x < x1 + (x2 - x1) * (y - y1) / (y2 - y1):
                inside = not inside
        return 0.0 if inside else self.exterior.distance(point)


# ------------------------------------------------------------------------------- holders of map and participant data
class Area:
    def __init__(self, id_, geometry, type_=None, subtype=None, color=None):
        self.id_, self.geometry, self.type_, self.subtype, self.color = id_, geometry, type_, subtype, color
        self.custom_tags = {}


class Lane(Area):
    pass


class Junction(Area):
    pass


class RoadLine(Area):
    pass


class Map:
    def __init__(self):
        self.junctions, self.areas, self.lanes, self.roadlines = {}, {}, {}, {}
        self.boundary = (0.0, 1.0, 0.0, 1.0)


class _State:
    def __init__(self, x, y, heading):
        self.location, self.heading = (float(x), float(y)), float(heading)


class _Trajectory:
    def __init__(self, state):
        self._state = state

    def get_state(self, frame=None):
        return self._state


class _Boxed:
    def __init__(self, id_, x, y, heading, length, width):
        self.id_, self.length, self.width = id_, float(length), float(width)
        self.color = self._default_color
        self.type_ = self._default_type
        self.trajectory = _Trajectory(_State(x, y, heading))
        # the reference's vertex order (vehicle.py:133-140, cyclist.py:98-105)
        self._bbox = LinearRing([[0.5 * self.length, -0.5 * self.width], [0.5 * self.length, 0.5 * self.width],
                                 [-0.5 * self.length, 0.5 * self.width], [-0.5 * self.length, -0.5 * self.width]])

    @property
    def geometry(self):
        return self._bbox

    def get_pose(self, frame=None):
        s = self.trajectory.get_state(frame)
        c, sn = np.cos(s.heading), np.sin(s.heading)
        return LinearRing([(c * x - sn * y + s.location[0], sn * x + c * y + s.location[1]) for x, y in self._bbox.coords[:-1]])


class Vehicle(_Boxed):
    _default_color, _default_type = "#2bcbba", "medium_car"


class Cyclist(_Boxed):
    _default_color, _default_type = "#fd9644", "cyclist"


class Pedestrian:
    def __init__(self, id_, x, y, radius):
        self.id_, self.color, self.type_, self._radius = id_, "#45aaf2", "adult_male", float(radius)
        self.trajectory = _Trajectory(_State(x, y, 0.0))

    def get_pose(self, frame=None):
        return self.trajectory.get_state(frame).location, self._radius


class Obstacle:
    def __init__(self, id_, x, y):
        self.id_, self.color, self.type_ = id_, (0, 0, 0, 255), "unknown"
        self.trajectory = _Trajectory(_State(x, y, 0.0))

    def get_pose(self, frame=None):
        return Point(self.trajectory.get_state(frame).location)


# --------------------------------------------------------------------------------------------------- the reference
def load_file(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def load_reference(ref):
    sg = types.ModuleType("shapely.geometry")
    sg.Point, sg.Polygon, sg.LinearRing = Point, Polygon, LinearRing
    sh = types.ModuleType("shapely")
    sh.geometry = sg
    sys.modules["shapely"], sys.modules["shapely.geometry"] = sh, sg

    def pkg(name):
        m = types.ModuleType(name)
        m.__path__ = []
        sys.modules[name] = m
        return m

    for name in ("tactics2d", "tactics2d.map", "tactics2d.participant", "tactics2d.sensor", "tactics2d.renderer"):
        pkg(name)
    me = pkg("tactics2d.map.element")
    me.Area, me.Junction, me.Lane, me.Map, me.RoadLine = Area, Junction, Lane, Map, RoadLine
    pe = pkg("tactics2d.participant.element")
    pe.Cyclist, pe.Obstacle, pe.Pedestrian, pe.Vehicle = Cyclist, Obstacle, Pedestrian, Vehicle
    t = os.path.join(ref, "tactics2d")
    load_file(os.path.join(t, "sensor", "sensor_base.py"), "tactics2d.sensor.sensor_base")
    cam = load_file(os.path.join(t, "sensor", "camera.py"), "tactics2d.sensor.camera")
    load_file(os.path.join(t, "renderer", "matplotlib_config.py"), "tactics2d.renderer.matplotlib_config")
    ren = load_file(os.path.join(t, "renderer", "matplotlib_renderer.py"), "tactics2d.renderer.matplotlib_renderer")
    return cam.BEVCamera, ren.MatplotlibRenderer


# --------------------------------------------------------------------------------------------------------- scenes
def racing_map(tiles):
    m = Map()
    for k, t in enumerate(tiles):
        m.lanes[k] = Lane("%04d" % k, LinearRing(t), subtype="road")   # generate_racing_track.py:181-185
    return m


def parking_map(target, quads, ids, with_target, drop_back_wall):
    """ParkingLotGenerator.generate stores the obstacles first (generate_parking_lot.py:393-394, ids "0000" ...) and the target
    area (id 0) only for a flipped parallel lot, behind them (:424-432).  BEVCamera gives both the back wall "0000" and the target
    the element id 1e6 + 0, and MatplotlibRenderer.update skips an element whose id it already holds (:619-622): the target is
    drawn only when the back wall is not in the map (the generator drops each obstacle with probability 0.05, :390)."""
    m = Map()
    for q, i in zip(quads, ids):
        if not (drop_back_wall and i == 0):
            m.areas["%04d" % i] = Area("%04d" % i, Polygon(q), type_="obstacle")        # :122
    if with_target:
        m.areas[0] = Area(0, Polygon(target), subtype="target_area", color="#EE766E")   # :114, :429-432
    return m


def non_convex_tile(tiles):
    for k, t in enumerate(tiles):
        e = np.roll(t, -1, axis=0) - t
        cr = e[:, 0] * np.roll(e, -1, axis=0)[:, 1] - e[:, 1] * np.roll(e, -1, axis=0)[:, 0]
        if (cr > 1e-9).any() and (cr < -1e-9).any():
            return k
    raise SystemExit("no non-convex tile found")


def make_scenes():
    """(name, map, participants {id: object}, bound id, perception range, window size, heading_up)"""
    length, width = 4.76, 1.85   # medium_car (what the drives of racing_progress.npz use as well)
    rt = np.load(os.path.join(HERE, "racing_tracks.npz"))
    gr = np.load(os.path.join(HERE, "generator_replay.npz"))
    scenes = []
    racing = (30.0, 30.0, 50.0, 10.0)

    def track(k):
        t = rt["tiles"][rt["tile_offsets"][k]:rt["tile_offsets"][k + 1]]
        origin = (t.reshape(-1, 2).min(axis=0) + t.reshape(-1, 2).max(axis=0)) / 2
        return np.float64(np.float32(t - origin)), origin

    def on_tile(tiles, k, turn=0.0):
        c = tiles[k].mean(axis=0)
        d = tiles[(k + 1) % len(tiles)].mean(axis=0) - c
        return float(np.float32(c[0])), float(np.float32(c[1])), float(np.float32(np.arctan2(d[1], d[0]) + turn))

    for k in range(3):
        tiles, origin = track(k)
        x, y, h = rt["start_pose"][k]
        x, y = x - origin[0], y - origin[1]
        scenes.append((f"racing_seed{int(rt['seed'][k])}_start", racing_map(tiles), {0: Vehicle(0, np.float32(x), np.float32(y), np.float32(h % (2 * np.pi)), length, width)},
                       0, racing, (200, 200), True))
    tiles, _ = track(1)
    nc = non_convex_tile(tiles)
    x, y, h = on_tile(tiles, nc, 0.2)
    scenes.append(("racing_seed2_non_convex_tile", racing_map(tiles), {0: Vehicle(0, x, y, h, length, width)}, 0, racing, (200, 200), True))
    x, y, h = on_tile(tiles, (nc + len(tiles) // 3) % len(tiles), -0.9)
    scenes.append(("racing_seed2_across", racing_map(tiles), {0: Vehicle(0, x, y, h, length, width)}, 0, racing, (200, 200), True))
    tiles, _ = track(2)
    x, y, h = on_tile(tiles, len(tiles) // 2, 2.5)
    scenes.append(("racing_seed3_reversed", racing_map(tiles), {0: Vehicle(0, x, y, h, length, width)}, 0, racing, (200, 200), True))

    for j, lot in enumerate((0, 7, 101, 180)):   # two bay and two parallel lots of the replayed generator runs
        a0, a1 = gr["area_off"][lot], gr["area_off"][lot + 1]
        quads = np.float64(np.float32(gr["area_quad"][a0:a1]))
        x, y, h = gr["start"][lot]
        if j % 2:   # not only at the start pose: on the way to the bay
            tc = gr["target"][lot].mean(axis=0)
            x, y, h = 0.5 * (x + tc[0]), 0.5 * (y + tc[1]), h + 0.6
        # lot 0: no target in the map (the usual case); 7: target behind the back wall's id (not drawn); 101, 180: back wall dropped
        scenes.append((f"parking_lot{lot}", parking_map(np.float64(np.float32(gr["target"][lot])), quads, gr["area_id"][a0:a1], j > 0, j > 1),
                       {0: Vehicle(0, np.float32(x), np.float32(y), np.float32(h), 5.3, 2.5)}, 0, (20.0,) * 4, (200, 200), True))

    # traffic: lanes, an obstacle, cars, a cyclist, pedestrians and an Obstacle participant; bound to a car that is not slot 0
    def traffic(seed, bind, prange, wsize, heading_up):
        rng = np.random.RandomState(seed)
        m = Map()
        for k in range(2):   # (few, wide lanes: the comparison leaves out a band around every edge, at most 15 % of a scene)
            y0 = -7.0 + 7.0 * k
            m.lanes[10 + k] = Lane("%04d" % (10 + k), LinearRing([(-60, y0), (60, y0), (60, y0 + 7.0), (-60, y0 + 7.0)]), subtype="road")
        m.lanes[14] = Lane("0014", LinearRing([(-2, -40), (2, -40), (2, 40), (-2, 40)]), subtype="road")
        m.areas["0001"] = Area("0001", Polygon([(8, 9), (20, 10), (19, 18), (9, 16)]), type_="obstacle")
        m.areas["0002"] = Area("0002", Polygon([(-12, -1), (-9, -1), (-9, 1.5), (-12, 1.5)]), type_="obstacle")   # on the lanes
        parts = {}
        for i in range(4):
            parts[i] = Vehicle(i, np.float32(rng.uniform(-18, 18)), np.float32(-5.25 + 3.5 * rng.randint(4)), np.float32(rng.normal(0, 0.15) + np.pi * rng.randint(2)),
                               4.76, 1.85)
        parts[6] = Cyclist(6, np.float32(rng.uniform(-10, 10)), np.float32(8.5), np.float32(0.3), 1.8, 0.6)
        parts[7] = Pedestrian(7, np.float32(rng.uniform(-8, 8)), np.float32(-9.0), 0.4)
        parts[8] = Pedestrian(8, np.float32(1.0), np.float32(rng.uniform(-3, 3)), 0.4)      # on a lane, partly under a car's z
        parts[9] = Obstacle(9, 3.0, 3.0)                                                     # not drawn (camera.py:318-319)
        parts[10] = Vehicle(10, parts[8].trajectory.get_state().location[0] + 1.0, parts[8].trajectory.get_state().location[1], np.float32(1.1), 4.76, 1.85)
        return (f"traffic_seed{seed}", m, parts, bind, prange, wsize, heading_up)

    scenes.append(traffic(5, 2, (20.0,) * 4, (200, 200), True))
    scenes.append(traffic(6, 0, (20.0,) * 4, (200, 200), False))            # north-up
    scenes.append(traffic(7, 3, (24.0, 16.0, 25.0, 5.0), (200, 120), True))   # a non-square window: the width is widened
    scenes.append(traffic(8, 1, (8.0, 8.0, 6.0, 6.0), (150, 250), True))  # ... and here the height
    return scenes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args()
    BEVCamera, MatplotlibRenderer = load_reference(os.path.abspath(args.ref))
    import matplotlib.colors as mcolors
    import matplotlib.pyplot as plt

    out = {}
    scenes = make_scenes()
    S = len(scenes)
    per = dict(sensor=[], heading=[], yaw=[], prange=[], wsize=[], xlim=[], ylim=[])
    shape, cls, zs, rgbs, pos, rot, rad, voff, xy, eoff, drawn = [], [], [], [], [], [], [], [0], [], [0], []
    style = {}
    for s, (name, map_, parts, bind, prange, wsize, heading_up) in enumerate(scenes):
        st = parts[bind].trajectory.get_state()
        yaw = np.pi / 2 - st.heading if heading_up else 0.0
        camera = BEVCamera(1, map_, perception_range=prange)
        data, _, _ = camera.update(0, parts, list(parts), position=Point(st.location), heading=yaw)
        ren = MatplotlibRenderer(resolution=wsize)
        ren.fig.set_dpi(DPI)
        ren.update(data)
        ren.fig.canvas.draw()
        buf = np.asarray(ren.fig.canvas.buffer_rgba())[..., :3]
        W, H = wsize
        (x0, x1), (y0, y1) = ren.xlim, ren.ylim
        cx = x0 + (np.arange(W) + 0.5) * (x1 - x0) / W
        cy = y1 - (np.arange(H) + 0.5) * (y1 - y0) / H
        gx, gy = np.meshgrid(cx, cy)
        disp = ren.ax.transData.transform(np.stack([gx.ravel(), gy.ravel()], axis=1))
        col = np.floor(disp[:, 0]).astype(int)
        row = buf.shape[0] - 1 - np.floor(disp[:, 1]).astype(int)
        assert col.min() >= 0 and col.max() < buf.shape[1] and row.min() >= 0 and row.max() < buf.shape[0]
        out[f"rgb_{s}"] = buf[row, col].reshape(H, W, 3)
        for k, v in (("sensor", st.location), ("heading", st.heading), ("yaw", yaw), ("prange", camera.perception_range), ("wsize", wsize),
                     ("xlim", ren.xlim), ("ylim", ren.ylim)):
            per[k].append(v)
        listing = data["map_data"]["road_elements"] + data["participant_data"]["participants"]
        held = {**ren.road_polygons, **ren.participants}
        seen = set()
        for el in listing:
            assert el["shape"] in ("polygon", "circle"), el["shape"]
            drawn.append(el["id"] in held and el["id"] not in seen)   # (update() skips an id it already holds)
            seen.add(el["id"])
            color, z = ren._resolve_style(el["color"], el.get("type"))
            c = TYPE_TO_CLASS[el["type"]]
            rgb = [int(round(255 * v)) for v in mcolors.to_rgb(color)]
            rec = dict(rgb=rgb, z=int(z), color_key=str(el["color"]), type_key=str(el["type"]))
            assert style.setdefault(c, rec) == rec, (c, rec, style[c])
            shape.append(el["shape"] == "circle"); cls.append(CLASS_NAMES.index(c)); zs.append(z); rgbs.append(rgb)
            pos.append(el.get("position", (0.0, 0.0))); rot.append(el.get("rotation", 0.0)); rad.append(el.get("radius", 0.0))
            g = [tuple(p) for p in el.get("geometry", [])]
            if len(g) > 1 and g[0] == g[-1]:
                g = g[:-1]
            xy.extend(g)
            voff.append(len(xy))
        eoff.append(len(shape))
        face = [int(round(255 * v)) for v in ren.fig.get_facecolor()[:3]]
        assert style.setdefault("background", dict(rgb=face, z=0, color_key="figure", type_key="figure"))["rgb"] == face
        plt.close(ren.fig)

    out.update(scene_name=np.array([sc[0] for sc in scenes]), scene_elem_off=np.int32(eoff), elem_shape=np.uint8(shape), elem_class=np.uint8(cls), elem_drawn=np.uint8(drawn),
               elem_z=np.int32(zs), elem_rgb=np.uint8(rgbs), elem_pos=np.float64(pos), elem_rot=np.float64(rot), elem_radius=np.float64(rad),
               elem_vert_off=np.int32(voff), elem_xy=np.float64(xy).reshape(-1, 2))
    for k, v in per.items():
        out[k] = np.float64(v)
    # the rules, from the reference's own functions
    ren = MatplotlibRenderer(resolution=(200, 200))
    hs = np.array([0.0, 0.7, 2.0, -2.6, 4.0])
    front = []
    for h in hs:
        ren.sensor_position, ren.camera_yaw = np.array([0.0, 0.0]), np.pi / 2 - h
        front.append(ren._transform_to_camera_view([[np.cos(h), np.sin(h)]])[0])
    ren.camera_yaw = 0.3
    out.update(probe_heading=hs, probe_front=np.float64(front), probe_yaw=np.float64(0.3), probe_rot=np.float64(ren._transform_to_camera_view([[1.0, 0.0]])[0]),
               scalar_range=np.float64(BEVCamera(1, Map(), perception_range=25.0).perception_range))
    plt.close(ren.fig)
    assert set(style) == set(CLASS_NAMES), sorted(set(CLASS_NAMES) - set(style))
    write_npz(os.path.join(args.out, "camera.npz"), out)
    with open(os.path.join(args.out, "camera_style.json"), "w") as f:
        json.dump(dict(class_names=list(CLASS_NAMES), style={c: style[c] for c in CLASS_NAMES}, dpi=DPI), f, indent=1, sort_keys=True)
        f.write("\n")
    print(S, "scenes,", len(shape), "elements,", os.path.getsize(os.path.join(args.out, "camera.npz")), "bytes")


if __name__ == "__main__":
    main()
