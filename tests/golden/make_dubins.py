#!/usr/bin/env python3
"""Golden data for the Dubins paths and the sampled curve lines -> dubins_curves.npz, made by RUNNING the reference's own classes.

TEST INFRASTRUCTURE (generation time only; nothing of the reference is kept).  From a reference tree this script loads
tactics2d/geometry/direction.py, geometry/circle.py, interpolator/dubins.py and interpolator/reeds_shepp.py from their FILES,
unmodified.  circle.py imports a compiled module `cpp_geometry`; the stand-in below gives its get_circle_by_tangent_vector as this
script's own statement of the centre formula: centre = point + r (cos(h +- pi/2), sin(h +- pi/2)), + for the left side.

dubins_curves.npz
  (a) paths: N = 1200 seeded random queries, float32-representable (stored as float32, to be widened): start / goal [N, 3] as
      (x, y, heading), start uniform in +-20 m, goal = start + uniform +-15 m, headings uniform in [-pi, pi) with a multiple of
      2 pi added to both in every tenth query.  radius [2]; queries 0 .. N/2 - 1 use radius[0], the others radius[1]
      (query_radius [N]).  valid u8 [N]: bit s = slot s of Dubins.get_all_path is a path.  For the valid (query, slot) pairs in
      ascending (query, slot): length f64 [M] and seg f64 [M, 3] = path.segments.  get_path i32 [N]: the index of get_path's
      object in get_all_path's list.  stable u8 [N]: the mask is the same for the goal shifted by +-1e-9 in x, y and heading.
      For the queries k < LAST_N of each radius and every valid slot, in the same order: last f64 [M2, 3] = the last point and
      last yaw of that slot's get_curve_line at the default step, with last_query i32 [M2] and last_slot i32 [M2].
  (b) curves: for seeded queries of their own (goal = start + uniform +-10 m), the shortest path's curve line --
      Dubins.get_path + DubinsPath.get_curve_line (rule 0) and ReedsShepp.get_path + ReedsSheppPath.get_curve_line (rule 1) --
      in the groups (radius[0], step 0.5), (radius[1], step 0.5), (radius[0], step 0.1), (radius[1], step 0.1).  Per curve:
      c_start / c_goal f32 [C, 3], c_radius i32 [C], c_step f64 [C], c_rule i32 [C], c_seg f64 [C, 5] (signed: signs * segments,
      units of the radius), c_letters i8 [C, 5], c_n_seg i32 [C], c_slot i32 [C] (Dubins: the slot; Reeds-Shepp: -1),
      c_count i32 [C], and concatenated c_xy f64 [P, 2], c_yaw f64 [P].  c_stable u8 [C]: the point count is the same with every
      segment scaled by 1 + 1e-9 and by 1 - 1e-9.
  (c) degenerate Dubins queries (start == goal, goal straight ahead, goal abeam, at both radii): deg_start / deg_goal f64 [K, 3],
      deg_radius f64 [K], deg_shortest f64 [K], deg_slot i32 [K].
  (d) words: the curve_type of the six slots as get_all_path's objects report them, as letters i8 [6, 3].

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_dubins.py --ref REFERENCE_TREE [--out DIR]

Prints the shares of unstable queries and the reference's time per call on this machine.  The file is written with fixed zip
time stamps: the same inputs give the same bytes.
"""
import argparse
import importlib.util
import io
import os
import sys
import time
import types
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, LAST_N = 20261019, 1200, 250
RADII = (4.0, 2.637 / np.tan(0.98 * 0.524))   # a round one and the tutorial's for a medium_car
GROUPS = ((0, 0.5, 50), (1, 0.5, 50), (0, 0.1, 12), (1, 0.1, 12))   # (radius index, step, curves per family)
LETTER = {"L": 1, "R": -1, "S": 0}
WORDS = ("LRL", "RLR", "LSL", "RSL", "RSR", "LSR")


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
        return [point[0] + radius * np.cos(a), point[1] + radius * np.sin(a)], radius


def load_reference(ref):
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
        geo.Circle = load("tactics2d.geometry.circle", "geometry", "circle.py").Circle
        dub = load("_ref_dubins", "interpolator", "dubins.py")
        rs = load("_ref_reeds_shepp", "interpolator", "reeds_shepp.py")
    finally:
        for k in names + ("_ref_dubins", "_ref_reeds_shepp"):
            v = saved.get(k)
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    return dub, rs


def queries(rng, n, reach):
    start, goal = np.empty((n, 3)), np.empty((n, 3))
    start[:, :2] = rng.uniform(-20, 20, (n, 2))
    goal[:, :2] = start[:, :2] + rng.uniform(-reach, reach, (n, 2))
    start[:, 2] = rng.uniform(-np.pi, np.pi, n)
    goal[:, 2] = rng.uniform(-np.pi, np.pi, n)
    turns = rng.choice([-2, -1, 1, 2], (n, 2)) * 2 * np.pi
    wide = np.arange(n) % 10 == 3
    start[wide, 2] += turns[wide, 0]
    goal[wide, 2] += turns[wide, 1]
    return start.astype(np.float32), goal.astype(np.float32)


def mask_of(paths):
    return sum(1 << s for s, p in enumerate(paths) if p is not None)


def pick_of(paths):
    k, shortest = -1, np.inf
    for s, p in enumerate(paths):
        if p is None or p.length > shortest:
            continue
        k, shortest = s, p.length
    return k


def degenerate(radius):
    R, pi = radius, np.pi
    g = [((0, 0, 0), (0, 0, 0)), ((1, 2, 0), (1, 2, 0)), ((0, 0, 0), (5, 0, 0)), ((0, 0, 0), (3 * R, 0, 0)), ((0, 0, 0), (0.05, 0, 0)),
         ((0, 0, 0), (0, 2 * R, 0)), ((0, 0, 0), (0, -2 * R, 0)), ((0, 0, 0), (0, 4 * R, 0)), ((0, 0, 0), (0, R, 0)),
         ((3, -2, pi / 2), (3, 4, pi / 2))]
    return np.array([a for a, _ in g], float), np.array([b for _, b in g], float)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    dub, rsm = load_reference(a.ref)
    rng = np.random.default_rng(SEED)
    start32, goal32 = queries(rng, N, 15)
    start, goal = start32.astype(np.float64), goal32.astype(np.float64)
    planners = [dub.Dubins(r) for r in RADII]
    rs_planners = [rsm.ReedsShepp(r) for r in RADII]
    which = (np.arange(N) >= N // 2).astype(np.int32)

    # (a) paths
    valid, pick, stable = np.zeros(N, np.uint8), np.zeros(N, np.int32), np.zeros(N, np.uint8)
    lengths, segs, last, last_q, last_s = [], [], [], [], []
    for i in range(N):
        d = planners[which[i]]
        paths = d.get_all_path(start[i, :2], start[i, 2], goal[i, :2], goal[i, 2])
        assert len(paths) == 6
        valid[i] = mask_of(paths)
        for s, p in enumerate(paths):
            if p is None:
                continue
            assert p.curve_type == WORDS[s]
            lengths.append(p.length)
            segs.append([float(v) for v in p.segments])
            if i % (N // 2) < LAST_N:
                p.get_curve_line(start[i, :2], start[i, 2], d.radius)
                last.append([p.curve[-1, 0], p.curve[-1, 1], p.yaw[-1]])
                last_q.append(i)
                last_s.append(s)
        best = d.get_path(start[i, :2], start[i, 2], goal[i, :2], goal[i, 2])
        k = pick_of(paths)
        assert best is not None and best.length == paths[k].length and best.curve_type == paths[k].curve_type
        pick[i] = k
        ok = True
        for axis in range(3):
            for dlt in (1e-9, -1e-9):
                g = goal[i].copy()
                g[axis] += dlt
                ok &= mask_of(d.get_all_path(start[i, :2], start[i, 2], g[:2], g[2])) == int(valid[i])
        stable[i] = ok
    print(f"unstable masks: {1 - stable.mean():.4%} of {N}")
    print("valid per slot:", [int(((valid >> s) & 1).sum()) for s in range(6)], "get_path per slot:", np.bincount(pick, minlength=6).tolist())

    # (b) curves
    c = {k: [] for k in ("start", "goal", "radius", "step", "rule", "seg", "letters", "n_seg", "slot", "count", "stable")}
    xy, yaw = [], []
    t_ref, n_ref = 0.0, 0
    for ri, step, per_family in GROUPS:
        s32, g32 = queries(rng, per_family, 10)
        for rule in (0, 1):
            for i in range(per_family):
                s, g = s32[i].astype(np.float64), g32[i].astype(np.float64)
                t0 = time.perf_counter()
                if rule == 0:
                    p = planners[ri].get_path(s[:2], s[2], g[:2], g[2])
                    p.get_curve_line(s[:2], s[2], RADII[ri], step)
                else:
                    p = rs_planners[ri].get_path(s[:2], s[2], g[:2], g[2])
                    p.get_curve_line(s[:2], s[2], RADII[ri], step)
                t_ref += time.perf_counter() - t0
                n_ref += 1
                if rule == 0:
                    word, signed = p.curve_type, np.array([float(v) for v in p.segments])
                    slot = WORDS.index(word)
                else:
                    word, signed, slot = p.actions, np.asarray(p.signs, float) * np.asarray(p.segments, float), -1
                curve, yw = p.curve.copy(), p.yaw.copy()
                ok = True
                for f in (1 + 1e-9, 1 - 1e-9):
                    keep = p.segments
                    p.segments = tuple(v * f for v in keep) if rule == 0 else np.asarray(keep) * f
                    p.get_curve_line(s[:2], s[2], RADII[ri], step)
                    ok &= len(p.curve) == len(curve)
                    p.segments = keep
                seg5, let5 = np.zeros(5), np.zeros(5, np.int8)
                seg5[:len(word)], let5[:len(word)] = signed, [LETTER[ch] for ch in word]
                for k, v in zip(("start", "goal", "radius", "step", "rule", "seg", "letters", "n_seg", "slot", "count", "stable"),
                                (s32[i], g32[i], ri, step, rule, seg5, let5, len(word), slot, len(curve), ok)):
                    c[k].append(v)
                xy.append(curve)
                yaw.append(yw)
    c_stable = np.array(c["stable"], np.uint8)
    print(f"unstable counts: {1 - c_stable.mean():.4%} of {len(c_stable)}; points: {sum(len(v) for v in xy)}")
    print(f"reference get_path + get_curve_line: {t_ref / n_ref * 1e3:.3f} ms per query on this machine (both families, steps 0.5 and 0.1)")
    # the defaults: Dubins at step 0.1, Reeds-Shepp at step 0.01
    t0 = time.perf_counter()
    for i in range(40):
        s, g = start[i], goal[i]
        p = planners[0].get_path(s[:2], s[2], g[:2], g[2])
        p.get_curve_line(s[:2], s[2], RADII[0])
        p = rs_planners[0].get_path(s[:2], s[2], g[:2], g[2])
        p.get_curve_line(s[:2], s[2], RADII[0])
    print(f"reference Dubins + Reeds-Shepp get_path + get_curve_line at their default steps: {(time.perf_counter() - t0) / 40 * 1e3:.3f} ms per query pair")
    assert stable.mean() >= 0.99 and c_stable.mean() >= 0.99, "change the seed"

    # (c) degenerate
    ds, dg, dr, dl, dk = [], [], [], [], []
    for r, d in zip(RADII, planners):
        a_, b_ = degenerate(r)
        for p0, p1 in zip(a_, b_):
            paths = d.get_all_path(p0[:2], p0[2], p1[:2], p1[2])
            k = pick_of(paths)
            ds.append(p0); dg.append(p1); dr.append(r); dl.append(paths[k].length); dk.append(k)

    out = dict(start=start32, goal=goal32, radius=np.array(RADII), query_radius=which, valid=valid, length=np.array(lengths),
               seg=np.array(segs), get_path=pick, stable=stable, last=np.array(last), last_query=np.array(last_q, np.int32),
               last_slot=np.array(last_s, np.int32),
               c_start=np.array(c["start"], np.float32), c_goal=np.array(c["goal"], np.float32), c_radius=np.array(c["radius"], np.int32),
               c_step=np.array(c["step"]), c_rule=np.array(c["rule"], np.int32), c_seg=np.array(c["seg"]),
               c_letters=np.array(c["letters"], np.int8), c_n_seg=np.array(c["n_seg"], np.int32), c_slot=np.array(c["slot"], np.int32),
               c_count=np.array(c["count"], np.int32), c_stable=c_stable, c_xy=np.concatenate(xy), c_yaw=np.concatenate(yaw),
               deg_start=np.array(ds), deg_goal=np.array(dg), deg_radius=np.array(dr), deg_shortest=np.array(dl),
               deg_slot=np.array(dk, np.int32), letters=np.array([[LETTER[ch] for ch in w] for w in WORDS], np.int8))
    path = os.path.join(a.out, "dubins_curves.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
