"""Time of the probabilistic roadmap's launch: t2d_prm_plan for batches of queries on generated obstacle grids.

    python scripts/time_prm.py [--reps 3] [--limit 500] [--small] [--out profiles/prm.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape and setting: the inputs and the workspace are resident on the device and the outputs are allocated once; after a
ramp of 2 launches, `--reps` windows of 5 launches each, every launch one ctypes call of the C entry point, device events around
a window that ends in a synchronise.  What a row holds is the time from launch to launch in such a loop (launches of milliseconds:
what the host and the queue add between two of them does not show); the kernel's own time would come from a rocprofv3 run of its
own and is unmeasured here.
  n = 4096 queries on grids of 16 x 16 and 24 x 24 from the host GridMapGenerator (costs 1 .. 5, 10 % and 30 % of the cells
  obstacles, its start and goal), boundary [0, W, 0, H], n_samples 126, 254 and 1000 with k_nearest 10, and n_samples 254 with
  connection_radius 2.5 and max_degree 64, one seed per row derived from 7 (search.row_seeds)
Every row records the edges and the sweeps per query (mean and maximum over the batch), the path length of the rows that found one,
the status histogram, and stands beside the reference's PRM.plan on one CPU core for ONE query of the same generator, size and
settings fed the same kind of draws (REFERENCE_MS, printed by tests/golden/make_prm.py --time).  This script neither reads nor runs
the reference.  One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch
times in microseconds.  Kernel name for a `rocprofv3 --kernel-trace --stats` run: prm_plan_kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 5, 2
STATUS = ("found", "no_path", "truncated", "overflow", "invalid")
SETTINGS = ((126, 10, None), (254, 10, None), (1000, 10, None), (254, 10, 2.5))   # n_samples, k_nearest, connection_radius
MAX_DEGREE = 64
# the reference's PRM.plan on one CPU core of the build machine, ONE query at these settings, fed the counter stream through the
# fixture maker's shim: (side, proportion, n_samples, radius) -> (ms, edges)
REFERENCE_MS = {
    (16, 0.1, 126, None): (23.5, 430), (16, 0.1, 254, None): (48.3, 953), (16, 0.1, 1000, None): (202.0, 4227), (16, 0.1, 254, 2.5): (67.5, 1569),
    (16, 0.3, 126, None): (43.7, 225), (16, 0.3, 254, None): (95.9, 597), (16, 0.3, 1000, None): (410.8, 2765), (16, 0.3, 254, 2.5): (143.6, 870),
    (24, 0.1, 126, None): (40.6, 387), (24, 0.1, 254, None): (86.7, 885), (24, 0.1, 1000, None): (354.3, 3985), (24, 0.1, 254, 2.5): (67.5, 730),
    (24, 0.3, 126, None): (73.8, 108), (24, 0.3, 254, None): (176.0, 344), (24, 0.3, 1000, None): (770.3, 2348), (24, 0.3, 254, 2.5): (157.4, 323),
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
    max_path = 256
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
            path = torch.empty((n, max_path, 2), dtype=torch.float64, device="cuda")
            path_len, status, n_edges, sweeps = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4))
            for n_samples, k, radius in SETTINGS:
                need = lib.t2d_prm_plan_workspace_bytes(n, n_samples, k if radius is None else MAX_DEGREE)
                ws = torch.empty(need, dtype=torch.uint8, device="cuda")

                def call():
                    rc = lib.t2d_prm_plan(0, n, weight.data_ptr(), hw.data_ptr(), side * side, start.data_ptr(), target.data_ptr(),
                                          boundary.data_ptr(), seed.data_ptr(), n_samples, k, 0.0 if radius is None else radius, MAX_DEGREE,
                                          1.0, 0.0, 0.0, max_path, ws.data_ptr(), need, path.data_ptr(), path_len.data_ptr(),
                                          status.data_ptr(), n_edges.data_ptr(), sweeps.data_ptr(), stream)
                    assert rc == 0
                st = stats(call)
                ne, sw, code, pl = (x.cpu().numpy() for x in (n_edges, sweeps, status, path_len))
                ok = code == search.PRM_FOUND
                ref = REFERENCE_MS.get((side, proportion, n_samples, radius))
                rows.append(dict(what="prm", n=n, height=side, width=side, obstacle_proportion=proportion, n_samples=n_samples,
                                 k_nearest=k if radius is None else None, connection_radius=radius,
                                 max_degree=MAX_DEGREE if radius is not None else None, edges_mean=round(float(ne.mean()), 1),
                                 edges_max=int(ne.max()), sweeps_mean=round(float(sw.mean()), 1), sweeps_max=int(sw.max()),
                                 path_len_mean=round(float(pl[ok].mean()), 1) if ok.any() else None,
                                 status={label: int((code == q).sum()) for q, label in enumerate(STATUS)},
                                 us_per_query=round(st["us_median"] / n, 3), workspace_bytes=int(need),
                                 reference_cpu_ms_one_query="unmeasured" if ref is None else ref[0],
                                 reference_cpu_edges_one_query="unmeasured" if ref is None else ref[1], kernel_us="unmeasured", **st))
                print(json.dumps(rows[-1]), flush=True)
                del ws
    np.random.set_state(state)
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
