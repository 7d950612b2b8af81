"""Time of the sampling planners' launch: t2d_sample_plan for batches of RRT, RRT* and RRT-Connect queries on generated obstacle
grids, and one timing of t2d_polyline_routes.

    python scripts/time_sample_plan.py [--reps 3] [--limit 500] [--small] [--out profiles/sample_plan.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape and kind: the inputs and the workspace are resident on the device and the outputs are allocated once; after a
ramp of 2 launches, `--reps` windows of 5 launches each, every launch one ctypes call of the C entry point, device events around
a window that ends in a synchronise.  What a row holds is the time from launch to launch in such a loop (launches of milliseconds:
what the host and the queue add between two of them does not show); the kernel's own time would come from a rocprofv3 run of its
own and is unmeasured here.
  n = 4096 queries on grids of 16 x 16 and 24 x 24 from the host GridMapGenerator (costs 1 .. 5, 10 % and 30 % of the cells
  obstacles, its start and goal), boundary [0, W, 0, H], extension_step 1.0, radius 3.0, max_iter 3000, max_nodes 4096, one seed per
  row derived from 7 (search.row_seeds)
Every row records the iterations and the tree size per query (mean and maximum over the batch: one wave runs one query, so a
launch lasts as long as its slowest query, and `us_per_max_iteration` is the launch time over the largest iteration count), the
status histogram, and stands beside the reference's plan on one CPU core for 8 queries of the same generator, sizes and settings
fed the same kind of draws (REFERENCE_MS: mean and slowest per query).  The last row is t2d_polyline_routes for 4096 envs of one
vehicle with a route of 256 vertices each, written from paths of 128 points.  One JSON line per measurement on stdout (and in
--out): the median and the spread (max - min) of the per-launch times in microseconds.  Kernel names for a
`rocprofv3 --kernel-trace --stats` run: sample_plan_kernel, polyline_routes_kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 5, 2
KINDS = ("rrt", "rrt_star", "rrt_connect")
STATUS = ("found", "max_iter", "truncated", "overflow", "invalid")
# the reference's plan on one CPU core of the build machine, 8 queries each at these settings, fed the counter stream through the
# fixture maker's shim: (kind, side, proportion) -> (mean ms per query, the slowest query's ms, mean iterations)
REFERENCE_MS = {
    ("rrt", 16, 0.1): (32.7, 81.6, 258.9),
    ("rrt_star", 16, 0.1): (324.8, 999.8, 258.9),
    ("rrt_connect", 16, 0.1): (0.6, 2.3, 11.2),
    ("rrt", 16, 0.3): (166.4, 559.0, 985.6),
    ("rrt_star", 16, 0.3): (3026.2, 10492.1, 985.6),
    ("rrt_connect", 16, 0.3): (62.1, 396.1, 505.6),
    ("rrt", 24, 0.1): (61.2, 183.7, 441.6),
    ("rrt_star", 24, 0.1): (874.4, 2751.9, 441.6),
    ("rrt_connect", 24, 0.1): (1.0, 4.2, 11.9),
    ("rrt", 24, 0.3): (311.1, 910.8, 1282.4),
    ("rrt_star", 24, 0.3): (4437.4, 20094.2, 1282.4),
    ("rrt_connect", 24, 0.3): (58.9, 342.8, 468.6),
}


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
    step, radius, max_iter, max_nodes, max_path = 1.0, 3.0, 3000, 4096, 256
    dev = lambda v, dt=np.float64: torch.as_tensor(np.ascontiguousarray(v, dt), device="cuda")
    state = np.random.get_state()
    for side in (16, 24):
        for proportion in (0.1, 0.3):
            grids, starts, goals = GridMapGenerator((side, side), 1, 5, proportion, random_seed=7).generate_batch(n)
            weight = dev(grids.reshape(n, side * side))
            hw = torch.full((n, 2), side, dtype=torch.int32, device="cuda")
            start = dev(np.stack([starts[:, 1], starts[:, 0]], 1))
            target = dev(np.stack([goals[:, 1], goals[:, 0]], 1))
            boundary = dev(np.tile([0.0, float(side), 0.0, float(side)], (n, 1)))
            seed = dev(search.row_seeds(7, n).view(np.int64), np.int64)
            need = lib.t2d_sample_plan_workspace_bytes(n, max_nodes)
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            path = torch.empty((n, max_path, 2), dtype=torch.float64, device="cuda")
            path_len, status, iterations = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))
            nodes = torch.empty((n, 2), dtype=torch.int32, device="cuda")
            for kind, name in enumerate(KINDS):
                def call():
                    rc = lib.t2d_sample_plan(0, n, kind, weight.data_ptr(), hw.data_ptr(), side * side, start.data_ptr(), target.data_ptr(),
                                             boundary.data_ptr(), seed.data_ptr(), step, radius, 1.0, 0.0, 0.0, max_iter, max_nodes, max_path,
                                             ws.data_ptr(), need, path.data_ptr(), path_len.data_ptr(), status.data_ptr(),
                                             iterations.data_ptr(), nodes.data_ptr(), stream)
                    assert rc == 0
                st = stats(call)
                it, nd, code = iterations.cpu().numpy(), nodes.cpu().numpy().sum(axis=1), status.cpu().numpy()
                ref = REFERENCE_MS.get((name, side, proportion))
                rows.append(dict(what=name, n=n, height=side, width=side, obstacle_proportion=proportion, extension_step=step, radius=radius,
                                 max_iter=max_iter, max_nodes=max_nodes, iterations_mean=round(float(it.mean()), 1), iterations_max=int(it.max()),
                                 nodes_mean=round(float(nd.mean()), 1), nodes_max=int(nd.max()),
                                 status={label: int((code == k).sum()) for k, label in enumerate(STATUS)},
                                 us_per_query=round(st["us_median"] / n, 3), us_per_max_iteration=round(st["us_median"] / max(int(it.max()), 1), 3),
                                 workspace_bytes=int(need),
                                 reference_cpu_ms_per_query="unmeasured" if ref is None else ref[0],
                                 reference_cpu_ms_slowest_query="unmeasured" if ref is None else ref[1],
                                 reference_cpu_iterations_mean="unmeasured" if ref is None else ref[2], kernel_us="unmeasured", **st))
                print(json.dumps(rows[-1]), flush=True)
            del ws
    np.random.set_state(state)

    # ---- t2d_polyline_routes: one route of 256 vertices per env, written from an S-curve of 128 points per env ----
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, full_type_table
    from tactics2d_amd.pool import ParticipantPool
    table, names = full_type_table()
    ty = names.index(list(VEHICLE_TEMPLATE)[0] + ":kin")
    pool = ParticipantPool(n, 1)
    pool.set_param_table(table)
    pool.set_status_config(max_step=100000)
    z = np.zeros(n, np.float32)
    pool.reset(z, z, z, z, np.full(n, ty, np.uint8))
    cap, pts = 256, 128
    line = np.stack([np.linspace(0.0, 95.0, cap), np.zeros(cap)], 1).astype(np.float32)
    pool.set_routes([[line] for _ in range(n)], np.arange(n), 0, 1.0)
    s = np.linspace(0.0, 127.0, pts)
    points = dev(np.tile(np.stack([s, 3.0 * np.sin(s / 18.0)], 1)[None], (n, 1, 1)))
    counts = torch.full((n,), pts, dtype=torch.int32, device="cuda")
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    st = stats(lambda: pool.polyline_routes(points, counts, count=count))
    rows.append(dict(what="polyline_routes", n_env=n, route_vertices=cap, points=pts, kernel_us="unmeasured", **st))
    print(json.dumps(rows[-1]), flush=True)
    pool.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--limit", type=int, default=500, help="seconds the GPU child may take")
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
