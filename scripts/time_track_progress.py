"""The racing tile progress launch (`t2d_track_progress`) beside the step launch it rides behind.

    python scripts/time_track_progress.py [--envs 4096] [--reps 7] [--out profiles/track_progress.json] [--kernels-only]

One pool of --envs single-ego racing envs, one reference-sized generated track per 256 envs (RacingTrackGenerator, seeds 0 ..),
every env's car on the centre line of a tile of its track with the matching tile_visiting.  Rows, each the mean over --reps
windows of 200 back-to-back launches between two device events, after a clock ramp of 3000 untimed launches of the same work
(what bench.py does before its timed region):

    progress_common    the progress launch alone, forward rule, window 8, the cars on the track (the march ends in round 0)
    progress_worst     the progress launch alone with the whole ring as window and the cars in the middle of the ring, where
                       they touch nothing: every tile of the ring is read and tested (5 - 8 rounds of 64 tiles)
    progress_window    the same poses under the forward rule's default window: 9 tiles read, none touched
    step               the step launch alone (t2d_step, zero-copy actions bound once)
    vector_step        step launch + progress launch (VecRacingEnv.step_torch without auto_reset)

--kernels-only: 50 launches of each, for a `rocprofv3 --kernel-trace --stats` run of its own.  One JSON object on stdout (and
in --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tactics2d_amd import layout as L, mapgeom
from tactics2d_amd.generator import RacingTrackGenerator
from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
from tactics2d_amd.pool import ParticipantPool

INNER, RAMP = 200, 3000


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


def tracks_for(n):
    gen, out = RacingTrackGenerator(), []
    for s in range(n):
        np.random.seed(s)
        t = gen.generate().tiles
        pts = t.reshape(-1, 2)
        out.append(np.float32(t - (pts.min(axis=0) + pts.max(axis=0)) / 2))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    E = args.envs
    tracks = tracks_for(max(1, E // 256))
    S = len(tracks)
    soe = (np.arange(E) * S // E).astype(np.int32)
    rng = np.random.default_rng(0)
    length, width = VEHICLE_TEMPLATE["medium_car"][:2]
    rows = vehicle_model("medium_car", "kinematics", steer_range=(-0.5, 0.5), accel_range=(-4.0, 2.0)).param_row(L.SHAPE_OBB, length, width)[None]
    x = np.zeros(E, np.float32); y = np.zeros(E, np.float32); h = np.zeros(E, np.float32)
    visiting = np.zeros(E, np.int32)
    T = max(len(t) for t in tracks)
    visited = np.zeros((E, T), bool)
    for e in range(E):
        t = tracks[soe[e]].astype(np.float64)
        i = int(rng.integers(len(t)))
        a, b = (t[i, 0] + t[i, 3]) / 2, (t[i, 1] + t[i, 2]) / 2
        p = a + (b - a) * rng.uniform(0.0, 1.0)
        x[e], y[e], h[e] = p[0], p[1], np.mod(np.arctan2(b[1] - a[1], b[0] - a[0]), 2 * np.pi)
        visiting[e] = i
        visited[e, :i + 1] = True
    boundary = np.float32([mapgeom.map_boundary(tracks[s].reshape(-1, 2)) for s in soe])
    pool = ParticipantPool(E, 1)
    pool.set_param_table(rows)
    pool.set_static_geometry(None, boundary)
    pool.set_status_config(max_step=100000, check_no_action=1, no_action_max_step=100)
    zeros = np.zeros(E, np.float32)

    def place(middle):
        pool.reset(zeros if middle else x, zeros if middle else y, h, zeros, np.zeros(E, np.uint8))
        pool.snapshot()

    stream = torch.cuda.current_stream().cuda_stream
    act = torch.zeros((E, 2), dtype=torch.float32, device="cuda")   # (zero actions: the cars stay where the common case has them)
    cases = {}

    def run(name, fn, note):
        if args.kernels_only:
            for _ in range(50):
                fn()
            torch.cuda.synchronize()
            cases[name] = dict(launches=50)
            return
        for _ in range(RAMP):
            fn()
        torch.cuda.synchronize()
        us = [timed(lambda: [fn() for _ in range(INNER)]) / INNER * 1e3 for _ in range(args.reps)]
        cases[name] = dict(series(us), note=note)

    def install(rule, max_advance):
        pool.set_tracks(tracks, soe, 0, rule, max_advance)
        pool.set_track_state(visiting, visited)

    place(False)
    install("forward", 8)
    run("progress_common", lambda: pool.track_progress(False, stream), "cars on the track, forward rule, window 8")
    common = pool.track_state()
    place(True)
    install("forward", 0)
    run("progress_worst", lambda: pool.track_progress(False, stream), "cars in the middle of the ring, whole ring read")
    worst = pool.track_state()
    install("forward", 8)
    run("progress_window", lambda: pool.track_progress(False, stream), "cars in the middle of the ring, window 8")
    place(False)
    install("forward", 8)
    pool.bind_actions(act.data_ptr() + 4, act.data_ptr(), stride=2)
    run("step", lambda: pool.step(100, stream), "t2d_step alone: " + pool.step_form())
    place(False)
    install("forward", 8)

    def vector_step():
        pool.step(100, stream)
        pool.track_progress(True, stream)
    run("vector_step", vector_step, "t2d_step + t2d_track_progress(write_status = 1)")
    pool.bind_actions(None, None)
    out = dict(script="scripts/time_track_progress.py", device=torch.cuda.get_device_name(0), envs=E, tracks=S,
               tiles_per_track=[len(t) for t in tracks], inner_launches=INNER, ramp_launches=RAMP, reps=args.reps, cases=cases)
    if not args.kernels_only:
        out["touched_runs_common"] = int((common["num_visited"] > visited.sum(axis=1)).sum())
        out["worst_case_moved_nothing"] = bool((worst["tile_visiting"] == visiting).all())
        c = cases
        out["progress_share_of_vector_step"] = round(1 - c["step"]["mean_us"] / c["vector_step"]["mean_us"], 3)
        out["worst_over_step"] = round(c["progress_worst"]["mean_us"] / c["step"]["mean_us"], 2)
        out["not_measured"] = ["rocprofv3 kernel durations", "hardware counters (VALU utilisation, L2 hit rate of the tile reads)"]
    pool.close()
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
