#!/usr/bin/env python3
"""Golden data for the racing env -> racing_tracks.npz, racing_progress.npz, made by RUNNING the reference's own code.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script

  * compiles the reference's two small native modules (geometry/cpp_geometry: the three-point circle; interpolator/
    cpp_interpolator: the Bezier curve) into a temporary directory that is removed when the script ends;
  * puts stand-ins for `shapely.geometry` into sys.modules -- shapely / GEOS is not available to this build:
      LineString   coords, length (segment lengths sqrt(dx dx + dy dy) summed in order), interpolate(d) (the point on the first
                   segment whose end lies beyond d, p0 + frac (p1 - p0));  Point  x, y, coords;
      LinearRing   coords; intersects(Polygon) = one of the ring's edges meets the closed polygon, and contains(Polygon) = False
                   (a curve contains no area), both in EXACT rational arithmetic (tests/track_ref.py: touch_exact);
      Polygon      coords; contains(Polygon) (every vertex in the closed convex polygon), intersection(o).area and
                   union(o).area (convex clipping), all in exact rational arithmetic;
  * loads from their FILES, unmodified: geometry/circle.py, geometry/direction.py, interpolator/bezier.py,
    map/element/lane.py, map/element/roadline.py, participant/trajectory/state.py, traffic/status.py,
    traffic/event_detection/{event_base, time_exceed, no_action, out_bound, off_lane}.py and
    map/generator/generate_racing_track.py (the whole RacingTrackGenerator class), and executes from the parsed
    envs/racing.py the definitions RacingEnv._get_rewards and _RacingScenarioManager._locate_agent / _reset_agent /
    check_status as they stand.  `Map` is a plain holder of lanes / roadlines / customs (the generator only assigns them);
    its `boundary` restates Map.boundary: floor / ceil of the extreme coordinates of lanes and road lines.

As with every geometry fixture here this pins the WIRING and the RULE -- which draws, which tiles, which order of checks,
which reward -- and not GEOS: the stand-ins decide the geometric questions exactly.

racing_tracks.npz, per track k (np.random.seed(seed[k]) before generate()):
    seed, n_checkpoint, n_tile, rng_pos, rng_crc (position and CRC-32 of the MT19937 key afterwards: the same draws consumed),
    tile_offsets, tiles (fp64 [sum n_tile, 4, 2], ring order of Lane.geometry), start_line (fp64 [K, 2, 2]),
    start_pose (fp64 [K, 3]: x, y, heading of _reset_agent)
racing_progress.npz: scripted drives on those tracks, shifted to the centre of their bounding box and rounded to fp32 (what the
pool holds; tests/track_scenes.py: centred_f32).  A drive sets the car's pose step by step (no physics: `update`'s physics call
and renderer are not executed; cnt_step is counted as update does, racing.py:329), calls _locate_agent, check_status and
_get_rewards, and ends with the episode.  Per drive d: drive_name, drive_track, drive_max_step, drive_offsets, boundary (fp32
[D, 4]), visiting0 / mask0 (the progress state the drive starts from); per step: pose (fp32 x, y, heading), run_first / run_len
(the touched run, -1 / 0 when empty), tile_visiting, mask (bit-packed, little bit order, MASK_BYTES per step), scenario,
traffic, terminated, truncated, reward (fp64).  And the march alone: 600 records of the real _locate_agent run on rings of 3 .. 130
lanes whose `intersects` answers from a scripted list -- march_n, march_touched, march_visiting0 / march_mask0 (before),
march_visiting1 / march_mask1 (after), bit-packed like the masks.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_racing.py --ref REFERENCE_TREE [--out DIR]

The files are written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import ast
import importlib.util
import io
import logging
import os
import shutil
import subprocess
import sys
import sysconfig
import tempfile
import types
import zipfile
import zlib
from fractions import Fraction

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import track_ref as R      # noqa: E402
import track_scenes as TS  # noqa: E402

SEEDS = (1, 2, 3)          # seed 2: a non-convex tile; seed 3: a closing tile shorter than the car
MASK_BYTES = 64            # 512 tiles


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


# ------------------------------------------------------------------------------------------------ shapely stand-ins
class Point:
    def __init__(self, *a):
        x, y = a if len(a) == 2 else a[0]
        self.x, self.y = float(x), float(y)
        self.coords = [(self.x, self.y)]


def _xy(c):
    return [(float(p.x), float(p.y)) if isinstance(p, Point) else (float(p[0]), float(p[1])) for p in c]


class LineString:
    def __init__(self, coordinates):
        self.coords = _xy(coordinates)
        p = np.array(self.coords)
        d = np.diff(p, axis=0)
        self._seg = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]).tolist()
        total, self._before = 0.0, []
        for s in self._seg:
            self._before.append(total)
            total += s
        self.length = total

    def interpolate(self, dist):
        c = self.coords
        if dist <= 0.0:
            return Point(c[0])
        for k, s in enumerate(self._seg):
            if self._before[k] + s > dist:
                frac = (dist - self._before[k]) / s
                return Point(c[k][0] + frac * (c[k + 1][0] - c[k][0]), c[k][1] + frac * (c[k + 1][1] - c[k][1]))
        return Point(c[-1])


def _frac(c):
    return [(Fraction(x), Fraction(y)) for x, y in c]


def _ccw(P):
    a2 = sum(P[i][0] * P[(i + 1) % len(P)][1] - P[(i + 1) % len(P)][0] * P[i][1] for i in range(len(P)))
    return P if a2 > 0 else P[::-1]


def _area(P):
    return abs(sum(P[i][0] * P[(i + 1) % len(P)][1] - P[(i + 1) % len(P)][0] * P[i][1] for i in range(len(P)))) / 2 if len(P) > 2 else Fraction(0)


class Polygon:
    """a convex polygon (a car's box, the map rectangle)"""

    def __init__(self, coordinates):
        self.coords = _xy(coordinates.coords if hasattr(coordinates, "coords") else coordinates)
        if len(self.coords) > 1 and self.coords[0] == self.coords[-1]:
            self.coords = self.coords[:-1]
        self._q = _ccw(_frac(self.coords))

    def _inside(self, p, k):
        a, b = self._q[k], self._q[(k + 1) % len(self._q)]
        return (b[0] - a[0]) * (p[1] - a[1]) - (b[1] - a[1]) * (p[0] - a[0])

    def contains(self, other):
        return all(self._inside(p, k) >= 0 for p in other._q for k in range(len(self._q)))

    def intersection(self, other):
        out = list(other._q)
        for k in range(len(self._q)):             # Sutherland-Hodgman against each edge of self
            inp, out = out, []
            for i in range(len(inp)):
                p, q = inp[i], inp[(i + 1) % len(inp)]
                fp, fq = self._inside(p, k), self._inside(q, k)
                if fp >= 0:
                    out.append(p)
                if (fp > 0 and fq < 0) or (fp < 0 and fq > 0):
                    t = fp / (fp - fq)
                    out.append((p[0] + t * (q[0] - p[0]), p[1] + t * (q[1] - p[1])))
            if not out:
                break
        return types.SimpleNamespace(area=_area(out))

    def union(self, other):
        return types.SimpleNamespace(area=_area(self._q) + _area(other._q) - self.intersection(other).area)


class LinearRing:
    def __init__(self, coordinates):
        self.coords = _xy(coordinates)
        if self.coords[0] != self.coords[-1]:
            self.coords.append(self.coords[0])

    def intersects(self, polygon):
        return R.touch_exact(np.array([[float(x), float(y)] for x, y in polygon._q]), np.array(self.coords[:4]))

    def contains(self, polygon):
        return False


# --------------------------------------------------------------------------------------------------- the reference
def build_native(ref, tmp):
    inc = subprocess.check_output([sys.executable, "-m", "pybind11", "--includes"], text=True).split()
    suffix = sysconfig.get_config_var("EXT_SUFFIX")
    for name, d in (("cpp_geometry", "geometry/cpp_geometry"), ("cpp_interpolator", "interpolator/cpp_interpolator")):
        d = os.path.join(ref, "tactics2d", d)
        srcs = sorted(os.path.join(d, "src", f) for f in os.listdir(os.path.join(d, "src")) if f.endswith(".cpp"))
        subprocess.check_call(["c++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(d, "include"), *inc, *srcs,
                               "-o", os.path.join(tmp, name + suffix)])
    sys.path.insert(0, tmp)


def load_file(path, name):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    sys.modules[name] = m
    spec.loader.exec_module(m)
    return m


def defs_of(path, names, namespace):
    """execute the named definitions of `path` -- as they stand -- in `namespace`; nested names as 'A.B.c'"""
    tree = ast.parse(open(path).read(), filename=path)
    for dotted in names:
        node = tree
        for part in dotted.split("."):
            node = next(n for n in node.body if isinstance(n, (ast.ClassDef, ast.FunctionDef)) and n.name == part)
        exec(compile(ast.Module(body=[node], type_ignores=[]), path, "exec"), namespace)
        print(f"executing {dotted}: lines {node.lineno}-{node.end_lineno}")


class Map:
    """holder of what RacingTrackGenerator.generate assigns; `boundary` restates Map.boundary (map/element/map.py:92-167)"""

    def __init__(self, name=None, scenario_type=None):
        self.lanes, self.roadlines, self.customs = {}, {}, {}

    @property
    def boundary(self):
        pts = np.array([c for lane in self.lanes.values() for c in lane.geometry.coords] +
                       [c for line in self.roadlines.values() for c in line.geometry.coords])
        return (np.floor(pts[:, 0].min()), np.ceil(pts[:, 0].max()), np.floor(pts[:, 1].min()), np.ceil(pts[:, 1].max()))


def load_reference(ref):
    t2d = os.path.join(ref, "tactics2d")
    geometry = types.ModuleType("shapely.geometry")
    geometry.LineString, geometry.Point, geometry.LinearRing, geometry.Polygon = LineString, Point, LinearRing, Polygon
    shapely = types.ModuleType("shapely")
    shapely.geometry = geometry
    sys.modules["shapely"], sys.modules["shapely.geometry"] = shapely, geometry
    for pkg in ("tactics2d", "tactics2d.geometry", "tactics2d.interpolator", "tactics2d.map", "tactics2d.map.element",
                "tactics2d.participant", "tactics2d.participant.trajectory", "tactics2d.traffic", "tactics2d.traffic.event_detection"):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules[pkg] = m
    load_file(os.path.join(t2d, "geometry", "direction.py"), "tactics2d.geometry.direction")
    sys.modules["tactics2d.geometry"].Circle = load_file(os.path.join(t2d, "geometry", "circle.py"), "tactics2d.geometry.circle").Circle
    sys.modules["tactics2d.interpolator"].Bezier = load_file(os.path.join(t2d, "interpolator", "bezier.py"), "tactics2d.interpolator.bezier").Bezier
    lane = load_file(os.path.join(t2d, "map", "element", "lane.py"), "tactics2d.map.element.lane")
    roadline = load_file(os.path.join(t2d, "map", "element", "roadline.py"), "tactics2d.map.element.roadline")
    el = sys.modules["tactics2d.map.element"]
    el.Lane, el.LaneRelationship, el.RoadLine, el.Map = lane.Lane, lane.LaneRelationship, roadline.RoadLine, Map
    state = load_file(os.path.join(t2d, "participant", "trajectory", "state.py"), "tactics2d.participant.trajectory.state")
    sys.modules["tactics2d.participant.trajectory"].State = state.State
    status = load_file(os.path.join(t2d, "traffic", "status.py"), "tactics2d.traffic.status")
    ed = os.path.join(t2d, "traffic", "event_detection")
    load_file(os.path.join(ed, "event_base.py"), "tactics2d.traffic.event_detection.event_base")
    det = {n: getattr(load_file(os.path.join(ed, f + ".py"), "tactics2d.traffic.event_detection." + f), n)
           for n, f in (("TimeExceed", "time_exceed"), ("NoAction", "no_action"), ("OutBound", "out_bound"), ("OffLane", "off_lane"))}
    gen = load_file(os.path.join(t2d, "map", "generator", "generate_racing_track.py"), "tactics2d_ref_generate_racing_track")
    ns = {"np": np, "logging": logging, "Polygon": Polygon, "State": state.State, "ScenarioStatus": status.ScenarioStatus,
          "TrafficStatus": status.TrafficStatus, "Union": __import__("typing").Union}
    defs_of(os.path.join(t2d, "envs", "racing.py"),
            ["RacingEnv._get_rewards", "RacingEnv._RacingScenarioManager._locate_agent",
             "RacingEnv._RacingScenarioManager._reset_agent", "RacingEnv._RacingScenarioManager.check_status"], ns)
    return gen.RacingTrackGenerator, lane, det, ns


# ----------------------------------------------------------------------------------------------------------- drives
class Agent:
    """what the executed definitions ask of the Vehicle: length, get_pose() (Vehicle.get_pose with the event kernels'
    expressions, from fp32 x, y, heading: the box the device evaluates), reset(state)"""
    length, width = 4.284, 1.799      # participant_template.py: medium_car

    def __init__(self, oracle):
        self.O, self.state = oracle, None
        self.x = self.y = self.h = np.float32(0)

    def reset(self, state):
        self.state = state

    def get_pose(self):
        return self.O.pose_obb(self.x, self.y, self.h, self.length, self.width, 0).tolist()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of a tactics2d source tree")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args(argv)
    from oracle import oracle as O
    O.build()
    tmp = tempfile.mkdtemp(prefix="racing_native_")
    try:
        build_native(args.ref, tmp)
        Generator, lane_mod, det, ns = load_reference(args.ref)
        make(args, O, Generator, lane_mod, det, ns)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def make(args, O, Generator, lane_mod, det, ns):
    locate, reset_agent, check_status, get_rewards = (ns[k] for k in ("_locate_agent", "_reset_agent", "check_status", "_get_rewards"))
    logging.disable(logging.CRITICAL)
    # ---- tracks ------------------------------------------------------------------------------------------------------
    T = {k: [] for k in ("seed", "n_checkpoint", "n_tile", "rng_pos", "rng_crc", "tiles", "start_line", "start_pose")}
    for seed in SEEDS:
        np.random.seed(seed)
        calls = []
        orig = Generator._get_checkpoints
        Generator._get_checkpoints = lambda self, _o=orig, _c=calls: (_c.append(_o(self)) or _c[-1])   # (to read n_checkpoint off the last call)
        map_ = Map()
        Generator().generate(map_)
        Generator._get_checkpoints = orig
        st = np.random.get_state()
        tiles = np.array([list(map_.lanes["%04d" % i].geometry.coords)[:4] for i in range(len(map_.lanes))])
        agent = Agent(O)
        reset_agent(types.SimpleNamespace(map_=map_, agent=agent))
        s = agent.state
        T["seed"].append(seed); T["n_checkpoint"].append(calls[-1][0].shape[1]); T["n_tile"].append(len(tiles))
        T["rng_pos"].append(st[2]); T["rng_crc"].append(zlib.crc32(np.ascontiguousarray(st[1]).tobytes()))
        T["tiles"].append(tiles); T["start_line"].append(np.array(map_.roadlines["start_line"].shape))
        T["start_pose"].append([s.x, s.y, s.heading])
        convex = sum(len(set(np.sign([(q[(i + 1) % 4][0] - q[i][0]) * (q[(i + 2) % 4][1] - q[(i + 1) % 4][1]) -
                                      (q[(i + 1) % 4][1] - q[i][1]) * (q[(i + 2) % 4][0] - q[(i + 1) % 4][0]) for i in range(4)]))) == 1 for q in tiles)
        print(f"seed {seed}: {T['n_checkpoint'][-1]} checkpoints, {len(tiles)} tiles ({len(tiles) - convex} non-convex), closing tile "
              f"{np.linalg.norm(tiles[-1][1] - tiles[-1][0]):.2f} m, rng position {st[2]}")
    offs = np.concatenate([[0], np.cumsum(T["n_tile"])])
    write_npz(os.path.join(args.out, "racing_tracks.npz"),
              dict(seed=np.int32(T["seed"]), n_checkpoint=np.int32(T["n_checkpoint"]), n_tile=np.int32(T["n_tile"]),
                   rng_pos=np.int32(T["rng_pos"]), rng_crc=np.uint32(T["rng_crc"]), tile_offsets=np.int32(offs),
                   tiles=np.concatenate(T["tiles"]).astype(np.float64), start_line=np.float64(T["start_line"]),
                   start_pose=np.float64(T["start_pose"])))

    # ---- drives ------------------------------------------------------------------------------------------------------
    D = {k: [] for k in ("drive_name", "drive_track", "drive_max_step", "drive_offsets", "boundary", "visiting0", "mask0", "pose", "run_first",
                         "run_len", "tile_visiting", "mask", "scenario", "traffic", "terminated", "truncated", "reward")}
    D["drive_offsets"].append(0)
    pack = lambda v, n: np.packbits(np.concatenate([np.array([v["%04d" % i] for i in range(n)], bool), np.zeros(MASK_BYTES * 8 - n, bool)]),
                                    bitorder="little")
    for k, seed in enumerate(SEEDS):
        tiles = TS.centred_f32(T["tiles"][k])
        n = len(tiles)
        assert n <= MASK_BYTES * 8
        lanes = {}
        for i in range(n):       # the tiles of _get_tiles again, on the fp32 coordinates the pool holds
            q = tiles[i].astype(np.float64)
            t = lane_mod.Lane(id_="%04d" % i, left_side=LineString([q[0], q[1]]), right_side=LineString([q[3], q[2]]), subtype="road")
            t.add_related_lane("%04d" % ((i + 1) % n), lane_mod.LaneRelationship.SUCCESSOR)
            lanes[t.id_] = t
        map_ = Map()
        map_.lanes = lanes
        boundary = map_.boundary
        c, th, nrm, end_mid = TS.tile_frames(tiles)
        start_mid = (tiles[:, 0].astype(np.float64) + tiles[:, 3]) / 2

        def along(i0, s0, step, n_steps, lateral=0.0):
            """poses on the centre line: starting s0 metres into tile i0, `step` metres per step (negative: backwards)"""
            seg = np.linalg.norm(end_mid - start_mid, axis=1)
            i, s, out = i0, s0, []
            for _ in range(n_steps):
                s += step
                while s >= seg[i]:
                    s -= seg[i]; i = (i + 1) % n
                while s < 0:
                    i = (i - 1) % n; s += seg[i]
                p = start_mid[i] + (end_mid[i] - start_mid[i]) * (s / seg[i]) + lateral * nrm[i]
                out.append((p[0], p[1], np.mod(th[i], 2 * np.pi)))
            return out

        east = int(np.argmax(c[:, 0]))
        far = (c[:, 0].mean(), c[:, 1].mean(), 0.3)      # inside the map, on no tile: the middle of the ring
        driven = lambda i: {"%04d" % t: t <= i for t in range(n)}
        plans = [("forward 0.7 m per step", along(0, 2.9, 0.7, 60), 0, None, 100000),
                 ("forward 3.1 m per step", along(0, 2.9, 3.1, 60), 0, None, 100000),
                 ("forward 6.9 m per step", along(0, 2.9, 6.9, 60), 0, None, 100000),
                 ("standing on the start line", along(0, 7.8, 0.0, 120), 0, None, 100000),
                 ("standing inside tile 5", along(5, 5.0, 0.0, 8), 5, driven(5), 100000),
                 ("reversing 0.7 m per step", along(0, 2.9, -0.7, 30), 0, None, 100000),
                 ("leaving sideways", [(c[east, 0] + dx, c[east, 1], np.mod(th[east], 2 * np.pi)) for dx in (0.0, 0.0, 3.5)], east, driven(east), 100000),
                 ("crossing the closing tile", along(n - 3, 1.0, 1.9, 30), n - 3, driven(n - 3), 100000),
                 ("crossing the closing tile at 6.9 m per step", along(n - 6, 2.9, 6.9, 30), n - 6, driven(n - 6), 100000),
                 ("touching no tile", [far] * 4, 7, driven(7), 100000),
                 ("out of time", along(0, 2.9, 6.9, 12), 0, None, 9)]
        closing = np.linalg.norm(end_mid[n - 1] - start_mid[n - 1])
        if closing < 4.0:     # the car spans the closing tile: three tiles touched
            plans.append(("touching three tiles", along(n - 1, closing / 2, 0.0, 1), n - 3, driven(n - 3), 100000))
        for name, poses, visiting0, visited0, max_step in plans:
            agent = Agent(O)
            sm = types.SimpleNamespace(
                map_=map_, agent=agent, cnt_step=0, tile_visiting="%04d" % visiting0,
                tile_visited=dict(visited0) if visited0 is not None else {"%04d" % i: i == 0 for i in range(n)},
                status_checklist={"time_exceed": det["TimeExceed"](max_step), "no_action": det["NoAction"](100),
                                  "out_bound": det["OutBound"](boundary), "off_road": det["OffLane"]()})
            env = types.SimpleNamespace(scenario_manager=types.SimpleNamespace(num_tile=n, cnt_step=0, num_visited_tile=0))
            D["drive_name"].append(f"seed {seed}: {name}"); D["drive_track"].append(k); D["drive_max_step"].append(max_step)
            D["boundary"].append(boundary); D["visiting0"].append(visiting0); D["mask0"].append(pack(sm.tile_visited, n))
            steps = 0
            for x, y, h in poses:
                agent.x, agent.y, agent.h = np.float32(x), np.float32(y), np.float32(h)
                sm.cnt_step += 1                                                  # racing.py:329
                pose = Polygon(agent.get_pose())
                touched = [i for i in range(n) if lanes["%04d" % i].geometry.intersects(pose)]
                before = int(sm.tile_visiting)
                locate(sm)
                scen, traf = check_status(sm, None)
                env.scenario_manager.cnt_step, env.scenario_manager.num_visited_tile = sm.cnt_step, sum(sm.tile_visited.values())
                reward = get_rewards(env, scen, traf)
                terminated = scen == ns["ScenarioStatus"].COMPLETED                # racing.py:169-174
                truncated = not terminated and (scen != ns["ScenarioStatus"].NORMAL or traf != ns["TrafficStatus"].NORMAL)
                # the touched run as the march sees it: the first contiguous stretch from tile_visiting on
                order = [(before + j) % n for j in range(n)]
                hit = [t in touched for t in order]
                j0 = hit.index(True) if any(hit) else -1
                j1 = j0
                while 0 <= j1 < n and hit[j1]:
                    j1 += 1
                D["pose"].append([agent.x, agent.y, agent.h]); D["run_first"].append(order[j0] if j0 >= 0 else -1)
                D["run_len"].append(j1 - j0 if j0 >= 0 else 0); D["tile_visiting"].append(int(sm.tile_visiting))
                D["mask"].append(pack(sm.tile_visited, n)); D["scenario"].append(int(scen)); D["traffic"].append(int(traf))
                D["terminated"].append(terminated); D["truncated"].append(truncated); D["reward"].append(float(reward))
                steps += 1
                if terminated or truncated:
                    break
            D["drive_offsets"].append(D["drive_offsets"][-1] + steps)
            print(f"  {D['drive_name'][-1]}: {steps} steps, ends ({D['scenario'][-1]}, {D['traffic'][-1]}), visited "
                  f"{sum(sm.tile_visited.values())} / {n}, longest run {max(D['run_len'][-steps:])}")
    # ---- the march alone: the real _locate_agent on scripted touch verdicts -------------------------------------------
    # (rings of lanes whose geometry answers `intersects` from a list: what the loop does with ANY pattern of touched tiles,
    # two separate runs and the run [tile_visiting] alone included -- the restatement's march is held against these records)
    M = {k: [] for k in ("march_n", "march_touched", "march_visiting0", "march_mask0", "march_visiting1", "march_mask1")}
    rng = np.random.default_rng(20261017)
    bits = lambda v: np.packbits(np.concatenate([np.asarray(v, bool), np.zeros(MASK_BYTES * 8 - len(v), bool)]), bitorder="little")
    degenerate = 0
    for n in (3, 5, 17, 64, 65, 130):
        touched = [False] * n
        ring = {"%04d" % i: types.SimpleNamespace(geometry=types.SimpleNamespace(intersects=lambda pose, i=i: touched[i], contains=lambda pose: False),
                                                  successors={"%04d" % ((i + 1) % n)}) for i in range(n)}
        agent = types.SimpleNamespace(get_pose=lambda: [(0, 0), (1, 0), (1, 1), (0, 1)])
        for _ in range(100):
            v0 = int(rng.integers(n))
            t = np.zeros(n, bool)
            kind = int(rng.integers(0, 6))
            if kind:
                s0, ln = int(rng.integers(n)), (int(rng.integers(1, 4)) if kind < 4 else int(rng.integers(1, n + 1)))
                t[(s0 + np.arange(ln)) % n] = True
                if kind == 2:
                    t[int(rng.integers(n))] = True
                if kind == 5:
                    t[:] = False; t[v0] = True                                   # the run [tile_visiting] alone
            if rng.random() < 0.3:
                t[(v0 + np.arange(int(rng.integers(0, 3)))) % n] = True
            vis0 = rng.random(n) < 0.3
            vis0[v0] = True
            touched[:] = t.tolist()
            sm = types.SimpleNamespace(map_=types.SimpleNamespace(lanes=ring), agent=agent, tile_visiting="%04d" % v0,
                                       tile_visited={"%04d" % i: bool(vis0[i]) for i in range(n)})
            locate(sm)
            vis1 = [sm.tile_visited["%04d" % i] for i in range(n)]
            degenerate += bool(t[v0] and not t[(v0 + 1) % n])
            M["march_n"].append(n); M["march_touched"].append(bits(t)); M["march_visiting0"].append(v0); M["march_mask0"].append(bits(vis0))
            M["march_visiting1"].append(int(sm.tile_visiting)); M["march_mask1"].append(bits(vis1))
    print(f"march records: {len(M['march_n'])}, the run starting at tile_visiting and ending there {degenerate} times")
    write_npz(os.path.join(args.out, "racing_progress.npz"),
              dict(march_n=np.int32(M["march_n"]), march_touched=np.uint8(M["march_touched"]), march_visiting0=np.int32(M["march_visiting0"]),
                   march_mask0=np.uint8(M["march_mask0"]), march_visiting1=np.int32(M["march_visiting1"]), march_mask1=np.uint8(M["march_mask1"]),
                   drive_name=np.array(D["drive_name"]), drive_track=np.int32(D["drive_track"]), drive_max_step=np.int32(D["drive_max_step"]),
                   drive_offsets=np.int32(D["drive_offsets"]), boundary=np.float32(D["boundary"]), visiting0=np.int32(D["visiting0"]),
                   mask0=np.uint8(D["mask0"]), pose=np.float32(D["pose"]), run_first=np.int32(D["run_first"]), run_len=np.int32(D["run_len"]),
                   tile_visiting=np.int32(D["tile_visiting"]), mask=np.uint8(D["mask"]), scenario=np.uint8(D["scenario"]),
                   traffic=np.uint8(D["traffic"]), terminated=np.uint8(D["terminated"]), truncated=np.uint8(D["truncated"]),
                   reward=np.float64(D["reward"])))
    for f in ("racing_tracks.npz", "racing_progress.npz"):
        print(os.path.join(args.out, f), os.path.getsize(os.path.join(args.out, f)), "bytes")


if __name__ == "__main__":
    main()
