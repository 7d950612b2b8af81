"""The BEV camera launch (`t2d_camera_render`): the binned kernel beside the naive form, the store floor, and the racing
vector step with and without it.

    python scripts/camera_probe.py [--envs 4096] [--reps 5] [--out profiles/camera.json] [--kernels-only]

Rows, each the mean over --reps windows of INNER back-to-back launches between two device events, after a clock ramp of RAMP
untimed launches of the same work (what bench.py does before its timed region):

    racing_class          4096 racing envs (one generated track of about 300 tiles per 256 envs, cars on the track), 200 x 200,
                          perception range (30, 30, 50, 10), the class image alone
    racing_class_rgb      the same, class + RGB
    racing_class_naive    the same scene and format with T2D_CAMERA_FORMAT_NAIVE: every pixel tests every element
    parking_class_rgb     4096 parking envs (scenarios.parking: 8 obstacles, the target, the car), range (20, 20, 20, 20)
    traffic_class_rgb     1024 envs x 64 participants (scenarios.highway), bound to slot 0, range (30, 30, 50, 10)
    step / vector_step / vector_step_camera
                          the racing step launch alone, step + progress, step + progress + camera (class + RGB)

store floor: the bytes a launch must write (envs x 40 000 B for the class image, three times that for RGB) at the HBM peak
bench.py's roofline uses (8000 GB/s); `floor_frac` = floor time / measured time.

--kernels-only: 20 launches of each camera case and nothing timed, for a `rocprofv3 --kernel-trace --stats` run of its own (its
kernel durations go beside the event times by hand: profiles/README.md).  One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tactics2d_amd import layout as L, mapgeom, scenarios, sensor
from tactics2d_amd.generator import RacingTrackGenerator
from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
from tactics2d_amd.pool import ParticipantPool

INNER, RAMP = 20, 60
HBM_PEAK_GBS = 8000.0   # bench.py's roofline
WINDOW = (200, 200)


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def series(us):
    return dict(us=[round(t, 2) for t in us], mean_us=round(float(np.mean(us)), 2), median_us=round(float(np.median(us)), 2),
                min_us=round(min(us), 2), max_us=round(max(us), 2))


def racing_pool(E):
    gen, tracks = RacingTrackGenerator(), []
    for s in range(max(1, E // 256)):
        np.random.seed(s)
        t = gen.generate().tiles
        pts = t.reshape(-1, 2)
        tracks.append(np.float32(t - (pts.min(axis=0) + pts.max(axis=0)) / 2))
    S = len(tracks)
    soe = (np.arange(E) * S // E).astype(np.int32)
    rng = np.random.default_rng(0)
    length, width = VEHICLE_TEMPLATE["medium_car"][:2]
    rows = vehicle_model("medium_car", "kinematics", steer_range=(-0.5, 0.5), accel_range=(-4.0, 2.0)).param_row(L.SHAPE_OBB, length, width)[None]
    x = np.zeros(E, np.float32); y = np.zeros(E, np.float32); h = np.zeros(E, np.float32)
    for e in range(E):
        t = tracks[soe[e]].astype(np.float64)
        i = int(rng.integers(len(t)))
        a, b = (t[i, 0] + t[i, 3]) / 2, (t[i, 1] + t[i, 2]) / 2
        p = a + (b - a) * rng.uniform(0.0, 1.0)
        x[e], y[e], h[e] = p[0], p[1], np.mod(np.arctan2(b[1] - a[1], b[0] - a[0]), 2 * np.pi)
    pool = ParticipantPool(E, 1)
    pool.set_param_table(rows)
    pool.set_static_geometry(None, np.float32([mapgeom.map_boundary(tracks[s].reshape(-1, 2)) for s in soe]))
    pool.set_status_config(max_step=100000, check_no_action=1, no_action_max_step=100)
    pool.reset(x, y, h, np.zeros(E, np.float32), np.zeros(E, np.uint8))
    pool.snapshot()
    pool.set_tracks(tracks, soe, 0, "forward", 8)
    return pool, [len(t) for t in tracks]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    E = args.envs
    stream = torch.cuda.current_stream().cuda_stream
    cases = {}

    def run(name, fn, note, nbytes=None, inner=INNER, ramp=RAMP):
        if args.kernels_only:
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            cases[name] = dict(launches=20)
            return
        for _ in range(ramp):
            fn()
        torch.cuda.synchronize()
        us = [timed(lambda: [fn() for _ in range(inner)]) / inner * 1e3 for _ in range(args.reps)]
        cases[name] = dict(series(us), note=note)
        if nbytes:
            floor_us = nbytes / (HBM_PEAK_GBS * 1e9) * 1e6
            cases[name].update(store_bytes=nbytes, store_floor_us=round(floor_us, 2), floor_frac=round(floor_us / float(np.mean(us)), 3),
                               store_gbs=round(nbytes / (float(np.mean(us)) * 1e-6) / 1e9, 1))

    px = WINDOW[0] * WINDOW[1]
    racing = ("tracks", "participants", "arrows")
    pool, n_tiles = racing_pool(E)
    cam = sensor.BEVCamera(pool, (30, 30, 50, 10), WINDOW, 0, True, racing, rgb=False)
    run("racing_class", lambda: pool.camera_render(stream), "class image alone", E * px)
    ref = None if args.kernels_only else cam.render_numpy()["image_class"]
    cam = sensor.BEVCamera(pool, (30, 30, 50, 10), WINDOW, 0, True, racing)
    run("racing_class_rgb", lambda: pool.camera_render(stream), "class + RGB", 4 * E * px)
    cam = sensor.BEVCamera(pool, (30, 30, 50, 10), WINDOW, 0, True, racing, rgb=False, naive=True)
    run("racing_class_naive", lambda: pool.camera_render(stream), "class image alone, every pixel tests every element", E * px, inner=4, ramp=4)
    same = None if args.kernels_only else bool(np.array_equal(cam.render_numpy()["image_class"], ref))
    if not args.kernels_only:
        act = torch.zeros((E, 2), dtype=torch.float32, device="cuda")
        pool.bind_actions(act.data_ptr() + 4, act.data_ptr(), stride=2)
        cam = sensor.BEVCamera(pool, (30, 30, 50, 10), WINDOW, 0, True, racing)
        run("step", lambda: pool.step(100, stream), "t2d_step alone: " + pool.step_form(), inner=200, ramp=2000)

        def vector_step():
            pool.step(100, stream)
            pool.track_progress(True, stream)

        def vector_step_camera():
            pool.step(100, stream)
            pool.track_progress(True, stream)
            pool.camera_render(stream)
        run("vector_step", vector_step, "t2d_step + t2d_track_progress", inner=200, ramp=2000)
        run("vector_step_camera", vector_step_camera, "t2d_step + t2d_track_progress + t2d_camera_render (class + RGB)")
        pool.bind_actions(None, None)
    pool.close()

    sc = scenarios.parking(E, seed0=0)
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    cam = sensor.BEVCamera(pool, (20, 20, 20, 20), WINDOW, 0, True, ("static", "target", "participants", "arrows"))
    run("parking_class_rgb", lambda: pool.camera_render(stream), "class + RGB, 8 obstacles + target + car per env", 4 * E * px)
    pool.close()

    Et = max(1, E // 4)
    sc = scenarios.highway(Et, A=64, seed=1)
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    layers = ("participants", "arrows") + (("static",) if sc.static is not None else ()) + (("lanes",) if sc.lanes is not None else ())
    cam = sensor.BEVCamera(pool, (30, 30, 50, 10), WINDOW, 0, True, layers)
    run("traffic_class_rgb", lambda: pool.camera_render(stream), f"class + RGB, {Et} envs x 64 participants", 4 * Et * px)
    pool.close()

    out = dict(script="scripts/camera_probe.py", device=torch.cuda.get_device_name(0), envs=E, window=list(WINDOW), tiles_per_track=n_tiles,
               inner_launches=INNER, ramp_launches=RAMP, reps=args.reps, hbm_peak_gbs=HBM_PEAK_GBS, cases=cases)
    if not args.kernels_only:
        c = cases
        out["naive_image_equals_binned"] = same
        out["binned_speedup_over_naive"] = round(c["racing_class_naive"]["mean_us"] / c["racing_class"]["mean_us"], 2)
        out["camera_share_of_vector_step"] = round(1 - c["vector_step"]["mean_us"] / c["vector_step_camera"]["mean_us"], 3)
        out["not_measured"] = ["rocprofv3 kernel durations (run with --kernels-only under rocprofv3 --kernel-trace --stats)",
                               "hardware counters"]
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
