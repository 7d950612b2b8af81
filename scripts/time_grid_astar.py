"""Time of the grid A* launch: t2d_grid_astar for batches of weighted obstacle grids, beside t2d_grid_dijkstra on the same grids.

    python scripts/time_grid_astar.py [--reps 5] [--limit 400] [--small] [--out profiles/grid_astar.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape: the inputs and the workspace are resident on the device and the outputs are allocated once; after a ramp of 3
launches, `--reps` windows of 10 launches each, every launch one ctypes call of the C entry point, device events around a window
that ends in a synchronise.  What a row holds is the time from launch to launch in such a loop; the kernel's own time comes from a
rocprofv3 run of its own.  A launch lasts as long as its slowest query, so every row records the pops per query (the reference's
iterations plus the final pop of a found target): mean and maximum over the batch.
  n = 4096 queries of 32 x 32 and of 64 x 64 (the cap), integer costs 1 .. 5, 10 % and 30 % of the cells obstacles, connectivity
  8, source the first cell and target the last one (both kept free): time_grid_dijkstra.py's grids;
  heuristic zero, euclidean, and euclidean with heuristic_scale 2.5, against the target cell; the optional state outputs NULL;
  and in the same run t2d_grid_dijkstra with its path on the same grids.
Whether the goal-directed search beats the whole-field solve at these sizes is the finding; there is no threshold.
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch times in
microseconds.  Kernel name for a `rocprofv3 --kernel-trace --stats` run: grid_astar_kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 10, 3


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
            point = torch.full((n, 2), float(side - 1), dtype=torch.float64, device="cuda")
            g = torch.empty((n, cells), dtype=torch.float64, device="cuda")
            path = torch.empty((n, cells), dtype=torch.int32, device="cuda")
            path_len, status, iterations, expanded = (torch.empty(n, dtype=torch.int32, device="cuda") for _ in range(4))
            need = int(lib.t2d_grid_astar_workspace_bytes(n, cells, 8))
            ws = torch.empty(need, dtype=torch.uint8, device="cuda")
            shape = dict(n=n, height=side, width=side, obstacle_proportion=proportion, connectivity=8)

            def dijkstra():
                rc = lib.t2d_grid_dijkstra(0, n, weight.data_ptr(), hw.data_ptr(), source.data_ptr(), target.data_ptr(), cells, 8,
                                           1.4142135623730951, cells, g.data_ptr(), path.data_ptr(), path_len.data_ptr(),
                                           status.data_ptr(), iterations.data_ptr(), stream)
                assert rc == 0
            st = stats(dijkstra)
            sw = iterations.cpu().numpy()
            rows.append(dict(what="grid_dijkstra", **shape, found=int((status == L.GRID_FOUND).sum()), sweeps_median=int(np.median(sw)),
                             sweeps_max=int(sw.max()), **st))
            print(json.dumps(rows[-1]), flush=True)
            for name, kind, scale in (("zero", L.ASTAR_H_ZERO, 1.0), ("euclidean", L.ASTAR_H_EUCLIDEAN, 1.0),
                                      ("euclidean", L.ASTAR_H_EUCLIDEAN, 2.5)):
                def astar():
                    rc = lib.t2d_grid_astar(0, n, weight.data_ptr(), hw.data_ptr(), source.data_ptr(), target.data_ptr(), cells, 8,
                                            1.4142135623730951, kind, point.data_ptr(), None, scale, 100000, cells, 1.0, 0.0, 0.0,
                                            ws.data_ptr(), need, path.data_ptr(), path_len.data_ptr(), None, status.data_ptr(),
                                            iterations.data_ptr(), expanded.data_ptr(), None, None, None, stream)
                    assert rc == 0
                st = stats(astar)
                ok = (status == L.GRID_FOUND).cpu().numpy()
                pops = iterations.cpu().numpy() + ok
                rows.append(dict(what="grid_astar", heuristic=name, heuristic_scale=scale, **shape, found=int(ok.sum()),
                                 no_path=int((status == L.GRID_NO_PATH).sum()), pops_mean=round(float(pops.mean()), 1),
                                 pops_max=int(pops.max()), expanded_mean=round(float(expanded.cpu().numpy().mean()), 1),
                                 workspace_bytes=need, us_per_pop_of_the_slowest=round(st["us_median"] / max(int(pops.max()), 1), 3), **st))
                print(json.dumps(rows[-1]), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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
