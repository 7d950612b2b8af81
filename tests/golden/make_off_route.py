#!/usr/bin/env python3
"""Golden answers for the off-route detector -> off_route.npz, made by RUNNING the reference's own `OffRoute` class
(traffic/event_detection/off_route.py:12-51).

TEST INFRASTRUCTURE (generation time only).  Loads off_route.py (and the event_base.py it imports) from their FILES in a
reference tree, with a stand-in `shapely.geometry` in sys.modules: `LineString` (refuses what is not a sequence of at least two
points of two or three numbers, as shapely does; keeps the coordinates) and `Point`, with `LineString.distance(Point)` evaluated
in exact rational arithmetic (tests/route_ref.py: exact_d2) and rounded once at the end.  shapely / GEOS is not available to
this build, so this file pins the reference's WIRING -- which point, which comparison (strict >), which exceptions, what
`reset` accepts -- and NOT the GEOS arithmetic: the kernel's arithmetic is pinned against exact rational arithmetic by
tests/test_off_route.py.  Stores numbers and names only:

    case_name  (C,)     what the case is
    offsets    (C + 1,) the route of case c is vertices offsets[c] .. offsets[c + 1] - 1
    verts      (V, 2)   route vertices (fp32 values)
    as_linestring (C,)  1: reset() got a ready-made LineString, 0: the list of points
    point      (C, 2)   the location (fp32 values)
    threshold  (C,)     fp32 values
    off        (C,)     what update() returned: 1 / 0
    exact_d2_num / exact_d2_den (C,)  the exact squared distance the stand-in computed, as decimal strings of a fraction
    before_reset_exc (1,) type name of what update() raises before reset()
    refused_name (R,), refused_exc (R,)  routes reset() refuses (route_ref.UNCOERCIBLE) and the type name it raises with

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_off_route.py --ref REFERENCE_TREE [--out DIR]

The npz is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import importlib.util
import io
import math
import os
import sys
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import route_ref as R   # noqa: E402


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (reproducible bytes)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)


class Point:
    def __init__(self, x, y):
        self.x, self.y = float(x), float(y)


class LineString:
    def __init__(self, coordinates):
        pts = [tuple(float(v) for v in p) for p in coordinates]
        if len(pts) < 2 or any(len(p) not in (2, 3) for p in pts):
            raise ValueError("LineStrings must have at least 2 coordinate tuples of 2 or 3 numbers")
        self.coords = [p[:2] for p in pts]
        self.exact_d2 = None

    def distance(self, other):
        """exact squared distance, one square root at the end (a stand-in for GEOS: see the module docstring)"""
        self.exact_d2, _ = R.exact_d2(np.float32(self.coords), other.x, other.y)
        return math.sqrt(float(self.exact_d2))   # (float(Fraction) and sqrt are both correctly rounded)


def load_reference(ref):
    geometry = types.ModuleType("shapely.geometry")
    geometry.LineString, geometry.Point = LineString, Point
    shapely = types.ModuleType("shapely")
    shapely.geometry = geometry
    sys.modules["shapely"], sys.modules["shapely.geometry"] = shapely, geometry
    d = os.path.join(ref, "tactics2d", "traffic", "event_detection")
    pkg = types.ModuleType("t2d_ref_event_detection")
    pkg.__path__ = [d]
    sys.modules[pkg.__name__] = pkg
    spec = importlib.util.spec_from_file_location(pkg.__name__ + ".off_route", os.path.join(d, "off_route.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    return mod.OffRoute


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of a tactics2d source tree")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args(argv)
    OffRoute = load_reference(args.ref)

    try:
        OffRoute(1.0).update(Point(0, 0))
        before = ""
    except Exception as e:   # noqa: BLE001 (the type name is the datum)
        before = type(e).__name__

    cases = [(n, r, p, t) for n, r, p, t, *_ in R.kats()]
    for k, (route, px, py, thr) in enumerate(R.random_cases(48, seed=11)):
        cases.append((f"random {k}", route, (px, py), thr))
    names, offs, verts, as_ls, pts, thrs, off, num, den = [], [0], [], [], [], [], [], [], []
    for k, (name, route, p, thr) in enumerate(cases):
        route = np.float32(route)
        det = OffRoute(float(np.float32(thr)))
        ready = k % 2
        det.reset(LineString(route.tolist()) if ready else route.tolist())
        verdict = det.update(Point(float(np.float32(p[0])), float(np.float32(p[1]))))
        names.append(name); verts.append(route); offs.append(offs[-1] + len(route)); as_ls.append(ready)
        pts.append([np.float32(p[0]), np.float32(p[1])]); thrs.append(np.float32(thr)); off.append(int(bool(verdict)))
        num.append(str(det.route.exact_d2.numerator)); den.append(str(det.route.exact_d2.denominator))

    refused_name, refused_exc = [], []
    for name, value in R.UNCOERCIBLE.items():
        try:
            OffRoute(1.0).reset(value)
            exc = ""
        except Exception as e:   # noqa: BLE001
            exc = type(e).__name__
        refused_name.append(name); refused_exc.append(exc)

    out = os.path.join(args.out, "off_route.npz")
    write_npz(out, dict(case_name=np.array(names), offsets=np.int32(offs), verts=np.concatenate(verts).astype(np.float32),
                        as_linestring=np.uint8(as_ls), point=np.float32(pts), threshold=np.float32(thrs), off=np.uint8(off),
                        exact_d2_num=np.array(num), exact_d2_den=np.array(den), before_reset_exc=np.array(before),
                        refused_name=np.array(refused_name), refused_exc=np.array(refused_exc)))
    print(out, len(cases), "cases,", int(np.sum(off)), "off;", "before reset:", before, "; refused:",
          dict(zip(refused_name, refused_exc)))


if __name__ == "__main__":
    main()
