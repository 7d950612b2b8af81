"""Time of the hybrid A* launch: t2d_hybrid_astar for batches of queries on generated obstacle grids.

    python scripts/time_hybrid_astar.py [--reps 3] [--limit 400] [--small] [--out profiles/hybrid_astar.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape: the inputs and the workspace are resident on the device and the outputs are allocated once; after a ramp of 2
launches, `--reps` windows of 10 launches each, every launch one ctypes call of the C entry point, device events around a window
that ends in a synchronise.  What a row holds is the time from launch to launch in such a loop (launches of milliseconds: what
the host and the queue add between two of them does not show); the kernel's own time would come from a rocprofv3 run of its own.
  n = 4096 queries on grids of 16 x 16 and 24 x 24 from the host GridMapGenerator (costs 1 .. 5, 10 % and 30 % of the cells
  obstacles, its start and goal), the start heading aimed at the goal, the target heading the same, boundary [0, W, 0, H],
  step_size 1.0, steering (-0.5, 0, 0.5), wheelbase 2.5, max_iter 50000: the reference's defaults
Every row records the pops per query (mean and maximum over the batch: one wave runs one query, so a launch lasts as long as its
slowest query, and `us_per_max_iteration` is the launch time over the maximum), the nodes, the status histogram, and stands beside
the reference's HybridAStar.plan on one CPU core as tests/golden/make_hybrid_astar.py timed it where the fixture was made, for
the fixture's cases on grids of the same size and proportion (REFERENCE_MS per query; those cases also vary the start heading,
the step and the steering set).  One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of
the per-launch times in microseconds.  Kernel name for a `rocprofv3 --kernel-trace --stats` run: hybrid_astar_kernel."""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 10, 2
REFERENCE_MS = {(16, 0.1): 80.5, (16, 0.3): 2.4, (24, 0.1): 236.6, (24, 0.3): 24.0}   # make_hybrid_astar.py's print-out
STATUS = ("found", "no_path", "max_iter", "truncated", "overflow", "invalid")


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from tactics2d_amd import _ffi, search
    from tactics2d_amd.generator import GridMapGenerator

    lib = _ffi.lib()
    stream = torch.cuda.current_stream().cuda_stream

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(INNER):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / INNER

    def stats(fn):
        for _ in range(RAMP):
            fn()
        torch.cuda.synchronize()
        t = sorted(timed(fn) for _ in range(args.reps))
        return dict(us_median=round(t[len(t) // 2], 2), us_spread=round(t[-1] - t[0], 2))

    rows = []
    n = 256 if args.small else 4096
    step, max_iter, max_nodes, max_path = 1.0, 50000, 65536, 128
    deltas = search.steer_deltas((-0.5, 0.0, 0.5), 2.5, step)
    state = np.random.get_state()
    for side in (16, 24):
        for proportion in (0.1, 0.3):
            grids, starts, goals = GridMapGenerator((side, side), 1, 5, proportion, random_seed=7).generate_batch(n)
            sx, sy, gx, gy = (np.float64(v) for v in (starts[:, 1], starts[:, 0], goals[:, 1], goals[:, 0]))
            aim = np.arctan2(gy - sy, gx - sx)
            dev = lambda v, dt=np.float64: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
            weight = dev(grids.reshape(n, side * side))
            hw = torch.full((n, 2), side, dtype=torch.int32, device="cuda")
            start, target = dev(np.stack([sx, sy, aim], 1)), dev(np.stack([gx, gy, aim], 1))
            boundary = dev(np.tile([0.0, float(side), 0.0, float(side)], (n, 1)))
            delta = dev(deltas)
            need = lib.t2d_hybrid_astar_workspace_bytes(n, max_nodes)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            path = torch.empty((n, max_path, 3), dtype=torch.float64, device="cuda")
            path_len, status, iterations, nodes = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4))

            def call():
                rc = lib.t2d_hybrid_astar(0, n, weight.data_ptr(), hw.data_ptr(), side * side, start.data_ptr(), target.data_ptr(),
                                          boundary.data_ptr(), delta.data_ptr(), len(deltas), step, 1.0, 0.0, 0.0, max_iter, max_nodes,
                                          max_path, ws.data_ptr(), need, path.data_ptr(), path_len.data_ptr(), status.data_ptr(),
                                          iterations.data_ptr(), nodes.data_ptr(), stream)
                assert rc == 0
            st = stats(call)
            it, nd, code = iterations.cpu().numpy(), nodes.cpu().numpy(), status.cpu().numpy()
            ref_ms = REFERENCE_MS[(side, proportion)]
            rows.append(dict(what="hybrid_astar", n=n, height=side, width=side, obstacle_proportion=proportion, step_size=step, n_steer=3,
                             max_iter=max_iter, max_nodes=max_nodes, iterations_mean=round(float(it.mean()), 1), iterations_max=int(it.max()),
                             nodes_mean=round(float(nd.mean()), 1), nodes_max=int(nd.max()),
                             status={name: int((code == k).sum()) for k, name in enumerate(STATUS)},
                             us_per_query=round(st["us_median"] / n, 3), us_per_max_iteration=round(st["us_median"] / max(int(it.max()), 1), 3),
                             workspace_bytes=int(need), reference_cpu_ms_per_query=ref_ms, kernel_us="unmeasured", **st))
            print(json.dumps(rows[-1]), flush=True)
            del ws
    np.random.set_state(state)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=400, help="seconds the GPU child may take")
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
