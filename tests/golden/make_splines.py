#!/usr/bin/env python3
"""Golden data for the Bezier, B-spline and cubic spline curves -> splines.npz, made by RUNNING the reference's own classes.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script compiles
tactics2d/interpolator/cpp_interpolator into a temporary directory (the recipe of make_racing.py::build_native: c++ -O3, no
-march, so no multiply-add is contracted), loads interpolator/bezier.py, b_spline.py and cubic_spline.py from their FILES,
unmodified, and calls their own get_curve.

splines.npz, one row per curve (C curves), in the order Bezier, B-spline, cubic:
  kind i32 [C] (0 Bezier, 1 B-spline, 2 cubic), n_ctrl i32 [C], n_interpolation i32 [C], degree i32 [C] (B-spline, else 0),
  knot_kind i32 [C] (B-spline: 0 the Python default (knot_vectors=None), 1 random non-decreasing, 2 clamped: degree + 1 repeats
  at both ends, 3 interior repeats, 4 all equal; else -1), boundary i32 [C] (cubic: 1 Natural, 2 Clamped, 3 NotAKnot; else 0),
  spacing i32 [C] (cubic: index into SPACINGS; else -1), derivs f64 [C, 2] (cubic first_derivatives), count i32 [C] = the
  number of points get_curve returned; concatenated in curve order: ctrl f64 [sum n_ctrl, 2], knots f64 [K] (only the curves
  with knot_kind >= 1: n_ctrl + degree + 1 each), xy f64 [sum count, 2].
  refusal_name / refusal_message: the ValueError text of each invalid call of REFUSALS.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_splines.py --ref REFERENCE_TREE [--out DIR]

Prints the reference's time per call on this machine.  The file is written with fixed zip time stamps: the same inputs give the
same bytes.
"""
import argparse
import importlib.util
import io
import os
import subprocess
import sys
import sysconfig
import tempfile
import time
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED = 20261019
BEZIER_N, BEZIER_NI = (2, 3, 4, 5, 8, 16, 32), (2, 3, 50, 63, 64, 65)
BSPLINE_NI = (1, 2, 64, 65, 100)
KNOT_KINDS = ("default", "random", "clamped", "interior_repeats", "all_equal")
CUBIC_N, CUBIC_NI = (3, 4, 5, 9, 32), (2, 3, 20, 64)
SPACINGS = ("random", "first_longer", "first_shorter", "equal", "last_longer", "last_shorter", "wide")


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(), compress_type=zipfile.ZIP_DEFLATED)


def build_native(ref, tmp):
    inc = subprocess.check_output([sys.executable, "-m", "pybind11", "--includes"], text=True).split()
    suffix = sysconfig.get_config_var("EXT_SUFFIX")
    d = os.path.join(ref, "tactics2d", "interpolator", "cpp_interpolator")
    srcs = sorted(os.path.join(d, "src", f) for f in os.listdir(os.path.join(d, "src")) if f.endswith(".cpp"))
    subprocess.check_call(["c++", "-O3", "-std=c++17", "-shared", "-fPIC", "-I" + os.path.join(d, "include"), *inc, *srcs,
                           "-o", os.path.join(tmp, "cpp_interpolator" + suffix)])
    sys.path.insert(0, tmp)


def load_reference(ref):
    out = []
    for f, cls in (("bezier.py", "Bezier"), ("b_spline.py", "BSpline"), ("cubic_spline.py", "CubicSpline")):
        spec = importlib.util.spec_from_file_location("_ref_" + f[:-3], os.path.join(ref, "tactics2d", "interpolator", f))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        out.append(getattr(mod, cls))
    return out


def knots_of(rng, kind, n_ctrl, degree):
    m = n_ctrl + degree + 1
    if kind == 1:
        return np.sort(rng.uniform(-2.0, 5.0, m))
    if kind == 2:
        inner = np.sort(rng.uniform(0.0, 1.0, m - 2 * (degree + 1)))   # (n_ctrl >= degree + 1: never negative)
        return np.concatenate([np.zeros(degree + 1), inner, np.ones(degree + 1)])
    if kind == 3:
        distinct = np.sort(rng.uniform(0.0, 3.0, max(2, (m + 1) // 2)))
        return np.sort(distinct[rng.integers(0, len(distinct), m)])
    return np.full(m, float(rng.uniform(-1.0, 1.0)))


def abscissae(rng, spacing, n_ctrl):
    h = rng.uniform(0.5, 6.0, n_ctrl - 1)
    if spacing == 1:
        h[0] = h[1] + rng.uniform(0.5, 3.0)
    elif spacing == 2:
        h[1] = h[0] + rng.uniform(0.5, 3.0)
    elif spacing == 3:
        h[:] = float(rng.choice([0.5, 1.0, 2.5, 3.7]))
    elif spacing == 4:
        h[-1] = h[-2] + rng.uniform(0.5, 3.0)
    elif spacing == 5:
        h[-2] = h[-1] + rng.uniform(0.5, 3.0)
    elif spacing == 6:
        h *= 300.0 / h.sum()
    return rng.uniform(-40.0, 40.0) + np.concatenate([[0.0], np.cumsum(h)])


def refusals(Bezier, BSpline, CubicSpline):
    pts = np.array([[0.0, 0.0], [1.0, 2.0], [3.0, 1.0], [4.0, 4.0]])
    calls = (
        ("bezier_shape", lambda: Bezier.get_curve(np.zeros((4, 3)), 10)),
        ("bezier_order_zero", lambda: Bezier.get_curve(pts, 10, order=0)),
        ("bezier_order_mismatch", lambda: Bezier.get_curve(pts, 10, order=2)),
        ("bezier_one_point", lambda: Bezier.get_curve(pts[:1], 10)),
        ("bezier_n_interpolation", lambda: Bezier.get_curve(pts, 1)),
        ("bspline_degree_negative", lambda: BSpline.get_curve(pts, degree=-1)),
        ("bspline_shape", lambda: BSpline.get_curve(np.zeros((4, 3)), degree=2)),
        ("bspline_knot_count", lambda: BSpline.get_curve(pts, np.linspace(0, 1, 5), degree=2)),
        ("bspline_knots_decreasing", lambda: BSpline.get_curve(pts, np.array([0, 1, 2, 3, 2.5, 4, 5.0]), degree=2)),
        ("bspline_too_few_control_points", lambda: BSpline.get_curve(pts, degree=4)),
        ("bspline_n_interpolation", lambda: BSpline.get_curve(pts, degree=2, n_interpolation=0)),
        ("cubic_boundary_type", lambda: CubicSpline.get_curve(pts, boundary_type=0)),
        ("cubic_shape", lambda: CubicSpline.get_curve(np.zeros((4, 3)))),
        ("cubic_too_few_control_points", lambda: CubicSpline.get_curve(pts[:2])),
        ("cubic_x_not_increasing", lambda: CubicSpline.get_curve(pts[[0, 2, 1, 3]])),
        ("cubic_n_interpolation", lambda: CubicSpline.get_curve(pts, n_interpolation=1)),
    )
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
    with tempfile.TemporaryDirectory() as tmp:
        build_native(a.ref, tmp)
        Bezier, BSpline, CubicSpline = load_reference(a.ref)
        rng = np.random.default_rng(SEED)
        rows = {k: [] for k in ("kind", "n_ctrl", "n_interpolation", "degree", "knot_kind", "boundary", "spacing", "derivs", "count")}
        ctrl, knots, xy = [], [], []

        def keep(kind, pts, ni, curve, degree=0, knot_kind=-1, boundary=0, spacing=-1, derivs=(0.0, 0.0)):
            for k, v in zip(rows, (kind, len(pts), ni, degree, knot_kind, boundary, spacing, derivs, len(curve))):
                rows[k].append(v)
            ctrl.append(pts)
            xy.append(curve)

        for N in BEZIER_N:
            for ni in BEZIER_NI:
                pts = rng.uniform(-30.0, 30.0, (N, 2))
                keep(0, pts, ni, Bezier.get_curve(pts, ni))

        # every (degree, knot kind, n_interpolation); the number of control points walks degree + 1 .. 32, both ends included
        sizes = {d: [d + 1, 32, d + 2, 8 + d, 17, d + 1, 31, 12, d + 3, 32] for d in range(6)}
        turn = 0
        for degree in range(6):
            for knot_kind in range(len(KNOT_KINDS)):
                for ni in BSPLINE_NI:
                    n_ctrl = sizes[degree][turn % len(sizes[degree])]
                    turn += 1
                    pts = rng.uniform(-30.0, 30.0, (n_ctrl, 2))
                    kv = None if knot_kind == 0 else knots_of(rng, knot_kind, n_ctrl, degree)
                    curve = BSpline.get_curve(pts, kv, degree, ni)
                    keep(1, pts, ni, curve, degree=degree, knot_kind=knot_kind)
                    if kv is not None:
                        knots.append(kv)
        assert any(d == 0 and n == 1 for d, n, k in zip(rows["degree"], rows["n_ctrl"], rows["kind"]) if k == 1)

        def cubic(boundary, n_ctrl, ni, spacing, derivs):
            pts = np.stack([abscissae(rng, spacing, n_ctrl), rng.uniform(-8.0, 8.0, n_ctrl)], 1)
            curve = CubicSpline.get_curve(pts, tuple(derivs), ni, boundary)
            keep(2, pts, ni, curve, boundary=boundary, spacing=spacing, derivs=derivs)

        turn = 0
        for boundary in (1, 2, 3):
            for n_ctrl in CUBIC_N:
                for ni in CUBIC_NI:
                    derivs = tuple(rng.uniform(-2.0, 2.0, 2)) if boundary == 2 or turn % 5 == 0 else (0.0, 0.0)
                    cubic(boundary, n_ctrl, ni, turn % len(SPACINGS), derivs)
                    turn += 1
            for spacing in range(len(SPACINGS)):   # every spacing at every boundary type: 3 points (the singular not-a-knot), 4 and 9
                for n_ctrl in (3, 4, 9):
                    cubic(boundary, n_ctrl, 20, spacing, tuple(rng.uniform(-2.0, 2.0, 2)) if boundary == 2 else (0.0, 0.0))

        names, messages = refusals(Bezier, BSpline, CubicSpline)

        def per_call(fn, reps=200):
            fn()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            return (time.perf_counter() - t0) / reps * 1e6

        p8, p16 = rng.uniform(-30, 30, (8, 2)), rng.uniform(-30, 30, (16, 2))
        c16 = np.stack([np.cumsum(rng.uniform(0.5, 6.0, 16)), rng.uniform(-8, 8, 16)], 1)
        print(f"reference Bezier, 8 control points, 100 points: {per_call(lambda: Bezier.get_curve(p8, 100)):.1f} us per call on this machine")
        print(f"reference cubic B-spline, 16 control points, 100 points: {per_call(lambda: BSpline.get_curve(p16, None, 3, 100)):.1f} us per call")
        print(f"reference not-a-knot cubic spline, 16 control points, n_interpolation 100: {per_call(lambda: CubicSpline.get_curve(c16, (0, 0), 100, 3)):.1f} us per call")

    out = dict(kind=np.array(rows["kind"], np.int32), n_ctrl=np.array(rows["n_ctrl"], np.int32),
               n_interpolation=np.array(rows["n_interpolation"], np.int32), degree=np.array(rows["degree"], np.int32),
               knot_kind=np.array(rows["knot_kind"], np.int32), boundary=np.array(rows["boundary"], np.int32),
               spacing=np.array(rows["spacing"], np.int32), derivs=np.array(rows["derivs"], np.float64),
               count=np.array(rows["count"], np.int32), ctrl=np.concatenate(ctrl), knots=np.concatenate(knots),
               xy=np.concatenate(xy), refusal_name=np.array(names), refusal_message=np.array(messages))
    print(f"curves: {len(out['kind'])} ({np.bincount(out['kind']).tolist()} per family), points: {len(out['xy'])}")
    path = os.path.join(a.out, "splines.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
