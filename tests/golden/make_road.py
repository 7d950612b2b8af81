#!/usr/bin/env python3
"""Golden data for the Spiral and ParamPoly3 curves and the plan-view reference lines -> road.npz, made by RUNNING the reference's
own code.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
interpolator/spiral.py and interpolator/param_poly3.py from their FILES, unmodified, and calls their own get_curve.  The parser
module map/parser/parse_xodr.py cannot be imported (shapely, pyproj and defusedxml are not needed for a reference line and need not
be installed): its file is parsed with `ast`, and the methods _sample_line, _sample_spiral, _sample_arc, _sample_poly3,
_sample_param_poly3, _sample_geometry and load_road are compiled from the parsed tree and executed -- load_road up to and including
its `if len(pts_arr) < 2` return, after which this script returns its locals pts_arr, s_arr, kappa_arr, keep and raw_pts.
geometry/circle.py is loaded from its file; the compiled module it imports is stood in for by this script's own statement of the
centre formula, centre = point + r (cos(h +- pi/2), sin(h +- pi/2)), + for the left side (as make_dubins.py does).

road.npz
  spirals (S rows): spiral_par f64 [S, 6] = length, x0, y0, heading, start_curvature, gamma; spiral_n i32 [S]; spiral_xy f64
      [sum spiral_n, 2] in row order.
  paramPoly3 (P rows): pp3_par f64 [P, 12] = length, x0, y0, heading, aU .. dV; pp3_range i32 [P] (0 normalized, 1 arcLength);
      pp3_count i32 [P]; pp3_xy f64 [sum pp3_count, 2].
  roads (R roads, G geometries in road order): road_n_geom i32 [R]; geom_kind i32 [G] (0 line, 1 spiral, 2 arc, 3 poly3,
      4 paramPoly3), geom_range i32 [G], geom_val f64 [G, 5] = s, x, y, hdg, length, geom_par f64 [G, 8] (the kind's attributes in
      the order of the XML schema, zero padded), geom_points i32 [G] = points _sample_geometry returned, geom_popped bool [G] = it
      dropped the geometry's last point; road_raw i32 [R] = raw points, raw_xy f64 [sum road_raw, 2], keep bool [sum road_raw];
      road_count i32 [R] = len(pts_arr) (0 where load_road returned before it had a line: such a road has no raw_xy either),
      xy f64 [sum road_count, 2], s and kappa f64 [sum road_count].
  refusal_name / refusal_message: the ValueError text of each invalid call of REFUSALS.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_road.py --ref REFERENCE_TREE [--out DIR]

Every discrete decision of the recorded data is kept away from its threshold (the script draws again otherwise): no raw
consecutive distance within 1e-6 of 0.02, no |curvature| of an arc within 1e-12 of 1e-9, no length / 0.1 within 1e-9 of an integer.
The file is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import ast
import importlib.util
import io
import logging
import os
import sys
import types
import xml.etree.ElementTree as ET
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261020
KINDS = ("line", "spiral", "arc", "poly3", "paramPoly3")
ATTRS = {"line": (), "spiral": ("curvStart", "curvEnd"), "arc": ("curvature",), "poly3": ("a", "b", "c", "d"),
         "paramPoly3": ("aU", "bU", "cU", "dU", "aV", "bV", "cV", "dV")}
METHODS = ("_sample_line", "_sample_spiral", "_sample_arc", "_sample_poly3", "_sample_param_poly3", "_sample_geometry", "load_road")


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


class _StandInCircle:
    @staticmethod
    def get_circle_by_tangent_vector(point, heading, radius, side):
        a = heading + np.pi / 2 if side == "L" else heading - np.pi / 2
        return [point[0] + np.cos(a) * radius, point[1] + np.sin(a) * radius], radius


def load_reference(ref):
    """Spiral, ParamPoly3 and a parser object holding the reference's own sampling methods"""
    names = ("cpp_geometry", "tactics2d", "tactics2d.geometry", "tactics2d.geometry.direction", "tactics2d.geometry.circle")
    saved = {k: sys.modules.get(k) for k in names}
    cpp = types.ModuleType("cpp_geometry")
    cpp.Circle = _StandInCircle
    pkg, geo = types.ModuleType("tactics2d"), types.ModuleType("tactics2d.geometry")
    pkg.geometry = geo
    sys.modules.update({"cpp_geometry": cpp, "tactics2d": pkg, "tactics2d.geometry": geo})

    def load(name, *rel):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref, "tactics2d", *rel))
        mod = importlib.util.module_from_spec(spec)
        sys.modules[name] = mod
        spec.loader.exec_module(mod)
        return mod

    try:
        load("tactics2d.geometry.direction", "geometry", "direction.py")
        Circle = load("tactics2d.geometry.circle", "geometry", "circle.py").Circle
        Spiral = load("_ref_spiral", "interpolator", "spiral.py").Spiral
        ParamPoly3 = load("_ref_param_poly3", "interpolator", "param_poly3.py").ParamPoly3
    finally:
        for k in names + ("_ref_spiral", "_ref_param_poly3"):
            v = saved.get(k)
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v

    path = os.path.join(ref, "tactics2d", "map", "parser", "parse_xodr.py")
    tree = ast.parse(open(path).read(), path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and any(getattr(f, "name", "") == "load_road" for f in n.body))
    fns = {f.name: f for f in cls.body if isinstance(f, ast.FunctionDef) and f.name in METHODS}
    assert set(fns) == set(METHODS), sorted(fns)
    road = fns["load_road"]
    stop = next(i for i, st in enumerate(road.body) if isinstance(st, ast.If) and "len(pts_arr) < 2" in ast.unparse(st.test))
    road.body = road.body[:stop + 1] + ast.parse("return pts_arr, s_arr, kappa_arr, keep, raw_pts").body
    for f in fns.values():
        f.returns = None
        for a in f.args.args:
            a.annotation = None
    module = ast.Module(body=[ast.ClassDef(name="PlanView", bases=[], keywords=[], body=[fns[m] for m in METHODS], decorator_list=[])],
                        type_ignores=[])
    ast.fix_missing_locations(module)
    scope = dict(np=np, logging=logging, ET=ET, Spiral=Spiral, ParamPoly3=ParamPoly3, Circle=Circle)
    exec(compile(module, path, "exec"), scope)
    return Spiral, ParamPoly3, scope["PlanView"]()


def geometry_node(g):
    node = ET.Element("geometry", {k: repr(float(g[k])) for k in ("s", "x", "y", "hdg", "length")})
    attrs = {k: repr(float(g[k])) for k in ATTRS[g["kind"]]}
    if g["kind"] == "paramPoly3" and g.get("pRange") is not None:
        attrs["pRange"] = g["pRange"]
    ET.SubElement(node, g["kind"], attrs)
    return node


def road_node(road):
    node = ET.Element("road", {"id": "1"})
    plan = ET.SubElement(node, "planView")
    for g in road:
        plan.append(geometry_node(g))
    return node


def off_grid(rng, lo, hi):
    """a length whose tenth count is nowhere near a step"""
    while True:
        v = float(rng.uniform(lo, hi))
        q = v / 0.1
        if abs(q - round(q)) > 1e-3:
            return v


def end_heading(g):
    L = g["length"]
    if g["kind"] == "arc":
        return g["hdg"] + g["curvature"] * L
    if g["kind"] == "spiral":
        return g["hdg"] + (g["curvStart"] + g["curvEnd"]) / 2 * L
    if g["kind"] == "poly3":
        return g["hdg"] + np.arctan(g["b"] + 2 * g["c"] * L + 3 * g["d"] * L * L)
    if g["kind"] == "paramPoly3":
        p = L if g.get("pRange") == "arcLength" else 1.0
        return g["hdg"] + np.arctan2(g["bV"] + 2 * g["cV"] * p + 3 * g["dV"] * p * p, g["bU"] + 2 * g["cU"] * p + 3 * g["dU"] * p * p)
    return g["hdg"]


def draw_geometry(rng, kind, s, x, y, hdg, length=None):
    L = off_grid(rng, 2.5, 14.0) if length is None else length
    g = dict(kind=kind, s=s, x=x, y=y, hdg=hdg, length=L)
    if kind == "spiral":
        g.update(curvStart=float(rng.choice([0.0, rng.uniform(-0.08, 0.08)])), curvEnd=float(rng.uniform(-0.12, 0.12)))
    elif kind == "arc":
        g.update(curvature=float(rng.choice([-1, 1]) * rng.uniform(0.01, 0.2)))
    elif kind == "poly3":
        g.update(a=0.0, b=float(rng.uniform(-0.1, 0.1)), c=float(rng.uniform(-0.02, 0.02)), d=float(rng.uniform(-0.002, 0.002)))
    elif kind == "paramPoly3":
        arc = bool(rng.integers(0, 2))
        k = 1.0 if arc else L
        g.update(aU=0.0, bU=k, cU=float(rng.uniform(-0.02, 0.02)) * k * k, dU=float(rng.uniform(-0.002, 0.002)) * k ** 3, aV=0.0,
                 bV=float(rng.uniform(-0.05, 0.05)) * k, cV=float(rng.uniform(-0.02, 0.02)) * k * k,
                 dV=float(rng.uniform(-0.002, 0.002)) * k ** 3, pRange="arcLength" if arc else rng.choice(["normalized", None]))
    return g


def chain(rng, parser, specs):
    """a road: specs = [(kind, length or None, overrides)]; each geometry starts where the reference's samples of the one before
    it end (an arc, which never samples its end: at its analytic end), so that seams repeat a point exactly"""
    road, s = [], float(rng.uniform(0.0, 50.0))
    x, y, hdg = float(rng.uniform(-100, 100)), float(rng.uniform(-100, 100)), float(rng.uniform(-np.pi, np.pi))
    for kind, length, over in specs:
        g = draw_geometry(rng, kind, s, x, y, hdg, length)
        g.update(over)
        road.append(g)
        pts, _ = parser._sample_geometry(geometry_node(g))
        if kind == "arc" and abs(g["curvature"]) >= 1e-9:
            k, L = g["curvature"], g["length"]
            x, y = x + (np.sin(hdg + k * L) - np.sin(hdg)) / k, y + (np.cos(hdg) - np.cos(hdg + k * L)) / k
        else:
            x, y = (float(v) for v in pts[-1])
        hdg, s = float(end_heading(g)), s + g["length"]
    return road


def stable(road, raw):
    for g in road:
        q = g["length"] / 0.1
        if g["length"] > 1e-6 and abs(q - round(q)) < 1e-9:
            return False
        if g["kind"] == "arc" and abs(abs(g["curvature"]) - 1e-9) < 1e-12:
            return False
    if len(raw) > 1:
        d = np.diff(np.asarray(raw, np.float64), axis=0)
        if np.any(np.abs(np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) - 0.02) < 1e-6):
            return False
    return True


def refusals(Spiral):
    calls = (("spiral_negative_length", lambda: Spiral.get_curve(-1.0, [0.0, 0.0], 0.0, 0.0, 0.01)),
             ("spiral_negative_n_interpolation", lambda: Spiral.get_curve(1.0, [0.0, 0.0], 0.0, 0.0, 0.01, -1)))
    names, messages = [], []
    for name, call in calls:
        try:
            call()
        except ValueError as exc:
            names.append(name)
            messages.append(str(exc))
        else:
            raise AssertionError(f"{name}: the reference did not refuse")
    return names, messages


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    logging.disable(logging.WARNING)      # (planView discontinuity warnings: the reference's Spiral does not end where a clothoid does)
    Spiral, ParamPoly3, parser = load_reference(a.ref)
    rng = np.random.default_rng(SEED)

    # ---- spirals: every branch, every sign combination, the point counts at which a wave's passes change
    sp_par, sp_n, sp_xy = [], [], []
    for n in (1, 2, 63, 64, 65, 100, 129):
        for branch in ("line", "arc", "euler", "gamma<0", "k0!=0", "k0!=0,gamma<0", "k0<0", "tiny gamma"):
            for _ in range(2):
                k0 = 0.0 if branch in ("line", "euler", "gamma<0", "tiny gamma") else float(rng.uniform(0.005, 0.1))
                k0 = -k0 if branch == "k0<0" else k0
                gamma = 0.0 if branch in ("line", "arc") else float(rng.uniform(0.0005, 0.05))
                gamma = -gamma if "gamma<0" in branch else 1e-6 * (1 + gamma) if branch == "tiny gamma" else gamma
                row = [float(rng.uniform(0.5, 60.0)), float(rng.uniform(-100, 100)), float(rng.uniform(-100, 100)),
                       float(rng.uniform(-np.pi, np.pi)), k0, gamma]
                sp_par.append(row)
                sp_n.append(n)
                sp_xy.append(Spiral.get_curve(row[0], row[1:3], row[3], row[4], row[5], n))
    sp_par.append([0.0, 3.0, -4.0, 0.7, 0.02, 0.01])   # length 0: n copies of the start point
    sp_n.append(5)
    sp_xy.append(Spiral.get_curve(0.0, [3.0, -4.0], 0.7, 0.02, 0.01, 5))

    # ---- paramPoly3: both ranges, the shortest lengths (the count's floor of 2), a length just under and just over a step
    pp_par, pp_range, pp_xy = [], [], []
    lengths = [0.0, 0.05, 0.1999, 0.2001, 0.31, 6.3500001, 6.4499999] + [off_grid(rng, 0.5, 18.0) for _ in range(41)]
    for i, L in enumerate(lengths):
        arc = i % 2
        k = 1.0 if arc else max(L, 1.0)
        c = [float(rng.uniform(-1, 1)), k, float(rng.uniform(-0.03, 0.03)) * k * k, float(rng.uniform(-0.003, 0.003)) * k ** 3,
             float(rng.uniform(-1, 1)), float(rng.uniform(-0.2, 0.2)) * k, float(rng.uniform(-0.03, 0.03)) * k * k,
             float(rng.uniform(-0.003, 0.003)) * k ** 3]
        row = [L, float(rng.uniform(-100, 100)), float(rng.uniform(-100, 100)), float(rng.uniform(-np.pi, np.pi))] + c
        pp_par.append(row)
        pp_range.append(arc)
        pp_xy.append(ParamPoly3.get_curve(L, (row[1], row[2]), row[3], *c, "arcLength" if arc else "normalized"))

    # ---- roads
    def fixed(rng):
        yield [("line", None, {}), ("spiral", None, dict(curvStart=0.0, curvEnd=0.05)), ("arc", None, dict(curvature=0.05)),
               ("spiral", None, dict(curvStart=0.05, curvEnd=0.0)), ("line", None, {})]                 # k0 != 0 in the 2nd spiral
        yield [("line", None, {}), ("spiral", None, dict(curvStart=0.0, curvEnd=-0.06)), ("arc", None, dict(curvature=-0.06))]   # gamma < 0
        yield [("line", None, {}), ("spiral", off_grid(rng, 0.8, 1.7), {}), ("line", None, {})]         # a spiral under 1.98 m
        yield [("line", 1e-17, dict(x=1.0)), ("line", None, {})]                                        # two equal points, one popped
        yield [("arc", None, dict(curvature=1e-10)), ("arc", None, dict(curvature=-3e-10)), ("poly3", None, {})]   # the line sampler
        yield [("paramPoly3", None, {}), ("paramPoly3", None, {}), ("paramPoly3", None, {}), ("paramPoly3", None, {})]
        yield [("spiral", off_grid(rng, 0.8, 1.7), {})]                                                 # one kept point: no line
        yield [("line", 0.0, {}), ("arc", None, {})]                                                    # length 0: one point
        yield [("spiral", 5e-7, {}), ("poly3", None, {})]                                               # a spiral under 1e-6: one point
        yield [("line", 0.05, {}), ("line", 0.13, {})]
        yield [(k, None, {}) for k in ("arc", "line", "poly3", "spiral", "paramPoly3", "arc")]
        yield [("line", 38.73, {})]
    specs = list(fixed(rng))
    while len(specs) < 36:
        specs.append([(KINDS[int(rng.integers(0, 5))], None, {}) for _ in range(int(rng.integers(1, 7)))])

    roads, out_rows = [], []
    for spec in specs:
        for _ in range(100):
            road = chain(rng, parser, spec)
            got = parser.load_road(road_node(road))
            sampled = [parser._sample_geometry(geometry_node(g))[0] for g in road]
            raw = [p for pts in sampled for p in pts]
            if stable(road, raw):
                break
        else:
            raise AssertionError("no stable draw")
        popped = []
        for g, pts in zip(road, sampled):
            node = geometry_node(g)
            full = getattr(parser, "_sample_" + {"paramPoly3": "param_poly3"}.get(g["kind"], g["kind"]))(node)[0]
            popped.append(len(full) != len(pts))
        roads.append(road)
        if isinstance(got[0], np.ndarray):
            pts_arr, s_arr, kappa_arr, keep, raw_pts = got
            assert np.array_equal(np.asarray(raw_pts, np.float64), np.asarray(raw, np.float64))
            out_rows.append(dict(raw=np.asarray(raw_pts, np.float64), keep=np.asarray(keep, bool), xy=pts_arr, s=s_arr, kappa=kappa_arr,
                                 popped=popped, points=[len(p) for p in sampled]))
        else:   # load_road returned before it had a line
            out_rows.append(dict(raw=np.zeros((0, 2)), keep=np.zeros(0, bool), xy=np.zeros((0, 2)), s=np.zeros(0), kappa=np.zeros(0),
                                 popped=popped, points=[len(p) for p in sampled]))

    geoms = [g for road in roads for g in road]
    names, messages = refusals(Spiral)
    out = dict(
        spiral_par=np.array(sp_par), spiral_n=np.array(sp_n, np.int32), spiral_xy=np.concatenate(sp_xy),
        pp3_par=np.array(pp_par), pp3_range=np.array(pp_range, np.int32), pp3_count=np.array([len(c) for c in pp_xy], np.int32),
        pp3_xy=np.concatenate(pp_xy),
        road_n_geom=np.array([len(r) for r in roads], np.int32), geom_kind=np.array([KINDS.index(g["kind"]) for g in geoms], np.int32),
        geom_range=np.array([1 if g.get("pRange") == "arcLength" else 0 for g in geoms], np.int32),
        geom_val=np.array([[g[k] for k in ("s", "x", "y", "hdg", "length")] for g in geoms], np.float64),
        geom_par=np.array([[g[k] for k in ATTRS[g["kind"]]] + [0.0] * (8 - len(ATTRS[g["kind"]])) for g in geoms], np.float64),
        geom_points=np.array([n for r in out_rows for n in r["points"]], np.int32),
        geom_popped=np.array([p for r in out_rows for p in r["popped"]], bool),
        road_raw=np.array([len(r["raw"]) for r in out_rows], np.int32), raw_xy=np.concatenate([r["raw"] for r in out_rows]),
        keep=np.concatenate([r["keep"] for r in out_rows]), road_count=np.array([len(r["xy"]) for r in out_rows], np.int32),
        xy=np.concatenate([r["xy"] for r in out_rows]), s=np.concatenate([r["s"] for r in out_rows]),
        kappa=np.concatenate([r["kappa"] for r in out_rows]), refusal_name=np.array(names), refusal_message=np.array(messages))
    print(f"spirals: {len(sp_n)} ({len(out['spiral_xy'])} points), paramPoly3: {len(pp_par)} ({len(out['pp3_xy'])} points), roads: "
          f"{len(roads)} of {len(geoms)} geometries ({len(out['raw_xy'])} raw, {len(out['xy'])} kept points; "
          f"{int(out['geom_popped'].sum())} popped; {int((out['road_count'] == 0).sum())} without a line)")
    path = os.path.join(a.out, "road.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
