"""Time of the Reeds-Shepp path follower: t2d_rs_follow alone and inside VecParkingEnv.step_torch.

    python scripts/time_rs_follow.py [--envs 4096] [--reps 5] [--limit 240] [--out profiles/rs_follow.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child:
  follow  a pool of --envs parked medium_cars.  "none": no env holds a path and no plan record reads FOUND (every lane passes the
          policy's row through).  "all": every env has adopted a four-segment plan written by the probe and acts on it in every
          call (the cars do not move, so no segment is ever popped).  A ramp of 3000 launches, then `--reps` windows of 10
          launches between device events.
  step    VecParkingEnv(--envs, scene_source="generator", lidar_beams=120, rs_planner=True) without and with rs_follow=True: 20
          steps to settle, then `--reps` windows of 10 step_torch calls; with the follower, the share of envs executing.
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-call times in
microseconds.  Asserts nothing.  Kernel name for a `rocprofv3 --kernel-trace --stats` run of its own: rs_follow_kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER = 10


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from tactics2d_amd import layout as L
    from tactics2d_amd.envs import VecParkingEnv
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    from tactics2d_amd.planner import RSFollower, RSPlanner
    from tactics2d_amd.pool import ParticipantPool

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(INNER):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / INNER

    def stats(fn, ramp):
        for _ in range(ramp):
            fn()
        torch.cuda.synchronize()
        t = sorted(timed(fn) for _ in range(args.reps))
        return dict(us_median=round(t[len(t) // 2], 2), us_spread=round(t[-1] - t[0], 2))

    rows, n = [], args.envs
    rng = np.random.default_rng(0)
    pool = ParticipantPool(n, 1)
    ego = vehicle_model("medium_car", "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0), steer_range=(-0.524, 0.524))
    pool.set_param_table(ego.param_row(L.SHAPE_OBB, *VEHICLE_TEMPLATE["medium_car"][:2])[None])
    pool.set_status_config()
    pool.set_target_areas(np.tile(np.float64([30, 30, 32, 30, 32, 35, 30, 35]), (n, 1)))
    pool.set_target_headings(np.zeros(n))
    z = np.zeros(n, np.float32)
    pool.reset(rng.uniform(-5, 5, n).astype(np.float32), rng.uniform(-5, 5, n).astype(np.float32),
               rng.uniform(-3, 3, n).astype(np.float32), z, np.zeros(n, np.int32))
    pool.lidar_config(24, 20.0)
    follower = RSFollower(pool, RSPlanner(pool, "medium_car", steer_hi=0.524))
    policy = torch.as_tensor(rng.uniform(-1, 1, (n, 2)).astype(np.float32), device="cuda")
    rec = np.zeros((n, L.RS_RECORD_BYTES // 8))
    none = dict(status=torch.as_tensor(rec, device="cuda"))
    rows.append(dict(what="rs_follow", n_envs=n, executing="none", **stats(lambda: follower.follow(policy, plan=none), 3000)))
    print(json.dumps(rows[-1]), flush=True)
    i32 = rec.view(np.int32).reshape(n, -1)
    i32[:, 0], i32[:, 2] = L.RS_FOUND, 4
    i32[:, 4:8] = [1, 0, -1, 0]
    rec[:, 5:9] = [2.0, 1.5, -2.0, 1.0]
    found = dict(status=torch.as_tensor(rec, device="cuda"))
    out = follower.follow(policy, plan=found)
    rows.append(dict(what="rs_follow", n_envs=n, executing="all", **stats(lambda: follower.follow(policy, plan=found), 3000),
                     share_executing=round(float((out["executing"] > 0).float().mean()), 3)))
    print(json.dumps(rows[-1]), flush=True)
    pool.close()
    for follow in (False, True):
        env = VecParkingEnv(n, scene_source="generator", lidar_beams=120, rs_planner=True, rs_follow=follow, seed=1)
        env.reset()
        act = torch.as_tensor(rng.uniform([-0.5, -1.0], [0.5, 1.0], (n, 2)).astype(np.float32), device="cuda")
        r = stats(lambda: env.step_torch(act), 20)
        extra = {}
        if follow:
            extra["share_executing"] = round(float((env.step_torch(act)["rs_follow"]["executing"] > 0).float().mean()), 3)
        rows.append(dict(what="step_torch", n_envs=n, rs_follow=follow, **r, **extra))
        print(json.dumps(rows[-1]), flush=True)
        env.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds the GPU child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--envs", str(args.envs),
           "--reps", str(args.reps)]
    cmd += ["--out", args.out] if args.out else []
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
