"""Time of the grid shortest-path launch: t2d_grid_dijkstra for batches of weighted obstacle grids.

    python scripts/time_grid_dijkstra.py [--reps 5] [--limit 240] [--small] [--out profiles/grid_dijkstra.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape: the inputs are resident on the device and the outputs are allocated once; after a ramp of 10 launches,
`--reps` windows of 50 launches each, every launch one ctypes call of the C entry point, device events around a window that
ends in a synchronise.  What a row holds is the time from launch to launch in such a loop (a launch of milliseconds: what the
host and the queue add between two of them does not show); the kernel's own time comes from a rocprofv3 run of its own.
  n = 4096 grids of 32 x 32 (the 256-lane form) and of 64 x 64 (the cap, the 1024-lane form), integer costs 1 .. 5, 10 % and
  30 % of the cells obstacles, connectivity 8, source the first cell and target the last one (both kept free)
Every row records the relaxation rounds the grids took (`sweeps`: median and maximum over the batch) and how many rows found a
path, and stands beside the reference's Dijkstra.plan_graph on one CPU core as tests/golden/make_grid_search.py timed it on
grids of at most 24 x 24 where the fixture was made (REFERENCE_MS per query: a LOWER bound for these larger grids).
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch times in
microseconds.  Kernel names for a `rocprofv3 --kernel-trace --stats` run: grid_dijkstra_kernel<1024, 256> and <4096, 1024>."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 50, 10
REFERENCE_MS = 5.0   # per query of the reference (half of make_grid_search.py's print-out, which times plan_graph + plan)


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from tactics2d_amd import _ffi, layout as L

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
    rng = np.random.default_rng(0)
    n = 512 if args.small else 4096
    for side in (32, 64):
        for proportion in (0.1, 0.3):
            cells = side * side
            assert cells <= L.GRID_MAX_CELLS
            w = rng.integers(1, 6, (n, cells)).astype(np.float64)
            w[rng.random((n, cells)) < proportion] = np.inf
            w[:, 0] = w[:, -1] = 1.0
            weight = torch.as_tensor(w, device="cuda")
            hw = torch.full((n, 2), side, dtype=torch.int32, device="cuda")
            source = torch.zeros(n, dtype=torch.int32, device="cuda")
            target = torch.full((n,), cells - 1, dtype=torch.int32, device="cuda")
            g = torch.empty((n, cells), dtype=torch.float64, device="cuda")
            path = torch.empty((n, cells), dtype=torch.int32, device="cuda")
            path_len, status, sweeps = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(3))

            def call():
                rc = lib.t2d_grid_dijkstra(0, n, weight.data_ptr(), hw.data_ptr(), source.data_ptr(), target.data_ptr(), cells, 8,
                                           1.4142135623730951, cells, g.data_ptr(), path.data_ptr(), path_len.data_ptr(),
                                           status.data_ptr(), sweeps.data_ptr(), stream)
                assert rc == 0
            st = stats(call)
            sw = sweeps.cpu().numpy()
            rows.append(dict(what="grid_dijkstra", n=n, height=side, width=side, obstacle_proportion=proportion, connectivity=8,
                             found=int((status == L.GRID_FOUND).sum()), no_path=int((status == L.GRID_NO_PATH).sum()),
                             sweeps_median=int(np.median(sw)), sweeps_max=int(sw.max()),
                             bytes_moved=n * cells * 20 + 12 * n, reference_cpu_us=round(REFERENCE_MS * 1e3 * n, 1), **st))
            print(json.dumps(rows[-1]), flush=True)
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
