"""Time of the Reeds-Shepp launches: t2d_rs_paths for batches of queries and t2d_rs_plan behind a parking env's scan.

    python scripts/time_rs_plan.py [--reps 5] [--limit 240] [--small] [--out profiles/rs_plan.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape:
  paths   n random queries (goal within +-15 m, radius 4.68 m) resident on the device; `--reps` windows of 10
          ReedsShepp.get_all_path launches each, device events around a window that ends in a synchronise.
  plan    VecParkingEnv(n_envs, scene_source="generator", lidar_beams=beams): 20 random step_torch steps to leave the start
          poses, then `--reps` windows of 10 RSPlanner.plan(lidar) launches on the scan of the last step; beside it one
          pool.step + lidar_scan at the same shape for scale, and the share of each plan status.
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch times in
microseconds.  Kernel names for a `rocprofv3 --kernel-trace --stats` run of its own: rs_paths_kernel, rs_plan_kernel."""
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

    from tactics2d_amd.envs import VecParkingEnv
    from tactics2d_amd.interpolator import ReedsShepp
    from tactics2d_amd.planner import STATUS_NAMES

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(INNER):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / INNER

    def stats(fn):
        fn()
        torch.cuda.synchronize()
        t = sorted(timed(fn) for _ in range(args.reps))
        return dict(us_median=round(t[len(t) // 2], 2), us_spread=round(t[-1] - t[0], 2))

    rows = []
    rng = np.random.default_rng(0)
    rs = ReedsShepp(4.68)
    for n in ((1024,) if args.small else (4096, 65536)):
        start = torch.as_tensor(np.concatenate([rng.uniform(-20, 20, (n, 2)), rng.uniform(-3.14, 3.14, (n, 1))], 1), device="cuda")
        goal = start + torch.as_tensor(np.concatenate([rng.uniform(-15, 15, (n, 2)), rng.uniform(-3.14, 3.14, (n, 1))], 1), device="cuda")
        sp, sh, gp, gh = start[:, :2].contiguous(), start[:, 2].contiguous(), goal[:, :2].contiguous(), goal[:, 2].contiguous()
        rows.append(dict(what="rs_paths", n=n, **stats(lambda: rs.get_all_path(sp, sh, gp, gh))))
        print(json.dumps(rows[-1]), flush=True)
    for n_envs, beams in (((256, 120),) if args.small else ((4096, 120), (4096, 360), (1024, 360))):
        env = VecParkingEnv(n_envs, scene_source="generator", lidar_beams=beams, rs_planner=True, seed=1)
        env.reset()
        for _ in range(20):
            act = torch.as_tensor(rng.uniform([-0.5, -1.0], [0.5, 1.0], (n_envs, 2)).astype(np.float32), device="cuda")
            out = env.step_torch(act)
        torch.cuda.synchronize()
        pool, lidar = env.scenario_manager.pool, out["lidar"]
        stream = torch.cuda.current_stream().cuda_stream
        status = out["rs_plan"]["status"].cpu().numpy()
        share = {STATUS_NAMES[k]: round(float((status == k).mean()), 3) for k in range(len(STATUS_NAMES))}

        def step_scan():
            pool.step(100, stream)
            pool.lidar_scan(lidar.data_ptr(), stream)

        rows.append(dict(what="rs_plan", n_envs=n_envs, beams=beams, status_share=share, **stats(lambda: env.planner.plan(lidar)),
                         step_and_scan=stats(step_scan)))
        print(json.dumps(rows[-1]), flush=True)
        env.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--limit", type=int, default=240, help="seconds the GPU child may take")
    ap.add_argument("--small", action="store_true")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    cmd += ["--small"] if args.small else []
    cmd += ["--out", args.out] if args.out else []
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
