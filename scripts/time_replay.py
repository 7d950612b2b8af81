"""Replayed participants: what `replay_kernel` costs next to `record_kernel`, and what a log-replay step costs.

    python scripts/time_replay.py [--reps 7] [--out profiles/replay.json] [--kernels-only]

1. `replay_kernel` (pool.replay_apply: every participant of a 4096 x 64 pool replayed, every window open) against
   `record_kernel` (DeviceTrajectory's record of the same pool) in the same run: both warmed up, then record, replay, record,
   replay, ... `--reps` windows of INNER back-to-back launches each, timed with device events around work that ends in a
   synchronise.  They move the same six rows in opposite directions; replay adds the ids word (read, and written where it
   changes) and two window words per participant.
2. `t2d_step` on the metric scene (mixed 4096 x 64) with 63 of 64 participants replayed from a recording of the scene itself,
   beside the same library's step with everybody integrated.  The replayed participants' 25 types are folded onto seven
   replayed rows (five car sizes, a cyclist, a pedestrian) -- the table holds 32 rows --, so their shapes are the nearest of
   those, not their own: a timing, not a parity run.

--kernels-only: part 1's launches alone, 50 of each, for a `rocprofv3 --kernel-trace --stats` run of its own.
One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tactics2d_amd import layout as L, scenarios as S
from tactics2d_amd.history import DeviceTrajectory, ReplaySource
from tactics2d_amd.participant import replayed_shape_row
from tactics2d_amd.pool import ParticipantPool

INNER = 200      # launches per timed window of part 1
STEPS = 10       # steps per timed window of part 2


def timed(fn):
    """milliseconds of fn() between two device events, ending in a synchronise"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def series(us):
    return dict(us=[round(t, 2) for t in us], mean_us=round(float(np.mean(us)), 2), median_us=round(float(np.median(us)), 2),
                min_us=round(min(us), 2), max_us=round(max(us), 2))


def kernels(reps, stream, only):
    n_env, A, n_slots = 4096, 64, 4
    n = n_env * A
    rng = np.random.default_rng(0)
    pool = ParticipantPool(n_env, A)
    pool.set_param_table(replayed_shape_row(L.SHAPE_OBB, 4.3, 1.8)[None])
    x = rng.uniform(-200, 200, (4, n)).astype(np.float32)
    pool.reset(x[0], x[1], x[2], x[3], np.zeros(n, np.uint8))
    traj = DeviceTrajectory(pool, 0, capacity=n_slots)
    for k in range(n_slots):
        traj.record(pool, k * 40)
    pool.replay_bind(ReplaySource.from_device(traj, 0, 40))
    buf = traj._buf

    def run_record():
        for k in range(INNER):
            buf.record(k % n_slots, stream)

    def run_replay():
        for _ in range(INNER):
            pool.replay_apply(stream)

    if only:
        for _ in range(50):
            buf.record(0, stream)
            pool.replay_apply(stream)
        torch.cuda.synchronize()
        return dict(launches_of_each=50)
    for _ in range(3):
        run_record()
        run_replay()
    torch.cuda.synchronize()
    t_rec, t_rep = [], []
    for _ in range(reps):
        t_rec.append(timed(run_record) / INNER * 1e3)
        t_rep.append(timed(run_replay) / INNER * 1e3)
    after = np.stack([pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED)])
    same = bool((after == x).all())      # (the recording is of the pool itself: a replay of stamp 0 changes nothing)
    pool.replay_unbind()
    pool.close()
    rec, rep = series(t_rec), series(t_rep)
    return dict(shape="4096 x 64", participants=n, launches_per_window=INNER, record_kernel=rec, replay_kernel=rep,
                ratio=round(rep["mean_us"] / rec["mean_us"], 3), ratio_of_medians=round(rep["median_us"] / rec["median_us"], 3),
                bytes_per_participant=dict(record=48, replay=64),
                ratio_by_bytes=round(64 / 48, 3), replay_left_the_recorded_state=same)


def replay_step(reps, stream):
    sc = S.mixed(4096, 64, seed=3)
    n, A = sc.n, sc.A
    acts = sc.sample_actions(np.random.default_rng(0))
    n_slots = 8 + (reps + 4) * STEPS
    a = ParticipantPool(sc.n_env, A)
    sc.load(a)
    a.set_actions(*acts)
    traj = DeviceTrajectory(a, 0, capacity=n_slots)
    traj.record(a, 0)
    for k in range(1, n_slots):
        a.step(100, stream)
        traj.record(a, k * 100, stream)
    a.sync()
    # the all-integrated step of the same library, timed on the pool that made the recording
    t_all = [timed(lambda: [a.step(100, stream) for _ in range(STEPS)]) / STEPS * 1e3 for _ in range(reps)]
    form_all = a.step_form(1)
    # seven replayed rows: the car sizes nearest to each vehicle template, a cyclist, a pedestrian
    names = sc.type_names
    dims = np.stack([sc.rows[:, L.P_SHAPE], sc.rows[:, L.P_LENGTH], sc.rows[:, L.P_WIDTH]], 1)
    proto = [names.index(k) for k in ("mini_car:kin", "small_car:kin", "medium_car:kin", "large_car:kin", "luxury_car:kin",
                                      "cyclist", "adult_male")]
    nearest = [min(proto, key=lambda p: (dims[p, 0] != dims[t, 0], abs(dims[p, 1] - dims[t, 1]))) for t in range(len(names))]
    rows = np.concatenate([sc.rows, np.stack([replayed_shape_row(*dims[p]) for p in proto])])
    ego = (np.arange(n) % A) == 0
    tid = np.where(ego, sc.type_id, len(names) + np.array([proto.index(nearest[t]) for t in sc.type_id])).astype(np.uint8)
    b = ParticipantPool(sc.n_env, A)
    b.set_param_table(rows)
    b.set_static_geometry(sc.static, sc.boundary, sc.boundary_valid)
    b.set_lane_geometry(sc.lanes)
    b.set_status_config(**sc.status)
    b.reset(sc.x, sc.y, sc.heading, sc.speed, tid, sc.active)
    b.replay_bind(ReplaySource.from_device(traj, 0, 100))
    b.set_actions(*acts)
    for _ in range(STEPS):
        b.step(100, stream)
    torch.cuda.synchronize()
    t_rep = [timed(lambda: [b.step(100, stream) for _ in range(STEPS)]) / STEPS * 1e3 for _ in range(reps)]
    # the step launch alone (device events around it, a pass of its own: the events cost the stream time)
    b.profile_enable(True)
    for _ in range(2 * STEPS):
        b.step(100, stream)
    b.sync()
    prof = {"step launch": b.profile_read(2)}
    active = int(((b.download(L.F_IDS) >> 16) & 0xff).sum())
    out = dict(scene="metric: mixed 4096 x 64", replayed_per_env=A - 1, steps_per_window=STEPS,
               all_integrated=dict(series(t_all), form=form_all, kernels=["collide_kernel (fused step)"]),
               replayed=dict(series(t_rep), form=b.step_form(1), kernels=["replay_kernel", "collide_kernel (fused step)"],
                             step_launch_alone_us=round(prof["step launch"][0] / max(prof["step launch"][1], 1) * 1e3, 2)),
               active_after=active, participants=n)
    b.replay_unbind()
    b.close()
    a.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--kernels-only", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    res = dict(script="scripts/time_replay.py", device=torch.cuda.get_device_name(0),
               kernels=kernels(args.reps, stream, args.kernels_only))
    if not args.kernels_only:
        res["step"] = replay_step(args.reps, stream)
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
