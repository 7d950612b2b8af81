"""Time of the Dubins and curve-line launches: t2d_dubins_paths for batches of queries, t2d_curve_lines for batches of curves
and t2d_curve_routes for the envs of a pool.

    python scripts/time_curve_lines.py [--reps 5] [--limit 240] [--small] [--out profiles/curve_lines.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape: the inputs are resident on the device and the outputs are allocated once; after a ramp of 200 launches,
`--reps` windows of 1000 launches each (10 - 20 ms), every launch one ctypes call of the C entry point, device events around a
window that ends in a synchronise.  What a row holds is the time from launch to launch in such a loop: the kernel AND whatever
the host and the queue add between two back-to-back launches; the kernels' own times come from the rocprofv3 run named below.
  dubins_paths   n random queries (goal within +-15 m, radius 4.68 m), both LRL rules
  curve_lines    n curves = the shortest Dubins paths of such queries at step 0.1 and 0.5, beside the STORE FLOOR of the launch:
                 the bytes it must write (24 per point actually stored + 28 per curve) over 6.29 TB/s, the copy rate measured on
                 this GPU (a floor for the stores alone: it leaves out the launch and the serial walk of each word)
  curve_routes   one such curve per env of a pool of n envs x 1 whose route sets hold one 256-vertex route each, step 0.5
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch times in
microseconds.  Kernel names for a `rocprofv3 --kernel-trace --stats` run of its own: dubins_paths_kernel, curve_lines_kernel,
curve_routes_kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 1000, 200
COPY_RATE = 6.29e12   # bytes per second: the float4 copy measured on an MI355X


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.interpolator import Dubins, pack_words
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, full_type_table
    from tactics2d_amd.pool import ParticipantPool

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

    def queries(n, rng):
        start = torch.as_tensor(np.concatenate([rng.uniform(-20, 20, (n, 2)), rng.uniform(-3.14, 3.14, (n, 1))], 1), device="cuda")
        goal = start + torch.as_tensor(np.concatenate([rng.uniform(-15, 15, (n, 2)), rng.uniform(-3.14, 3.14, (n, 1))], 1), device="cuda")
        return start.contiguous(), goal.contiguous()

    def dubins_words(db, start, goal):
        path = db.get_path(start, None, goal, None)
        pad = torch.zeros((start.shape[0], 2), dtype=torch.float64, device="cuda")
        return pack_words(torch.cat([path.segments, pad], 1), torch.cat([path.steer, pad.to(torch.int8)], 1), path.n_seg)

    rows = []
    rng = np.random.default_rng(0)
    radius = 4.68
    for n in ((1024,) if args.small else (4096, 65536)):
        start, goal = queries(n, rng)
        mask = torch.empty(n, dtype=torch.uint8, device="cuda")
        seg = torch.empty((n, 6, 3), dtype=torch.float64, device="cuda")
        length = torch.empty((n, 6), dtype=torch.float64, device="cuda")
        short = torch.empty((n, 2), dtype=torch.int32, device="cuda")
        for rule in (0, 1):
            def call():
                rc = lib.t2d_dubins_paths(0, n, radius, start.data_ptr(), goal.data_ptr(), rule, mask.data_ptr(), seg.data_ptr(),
                                          length.data_ptr(), short.data_ptr(), stream)
                assert rc == 0
            rows.append(dict(what="dubins_paths", n=n, lrl_rule=rule, **stats(call)))
            print(json.dumps(rows[-1]), flush=True)
    n = 1024 if args.small else 4096
    start, goal = queries(n, rng)
    words = dubins_words(Dubins(radius, "standard"), start, goal)
    for step in (0.1, 0.5):
        max_points = int(np.ceil((22.0 + 7 * np.pi * radius) / step)) + 10
        xy = torch.empty((n, max_points, 2), dtype=torch.float64, device="cuda")
        yaw = torch.empty((n, max_points), dtype=torch.float64, device="cuda")
        count = torch.empty(n, dtype=torch.int32, device="cuda")
        end = torch.empty((n, 3), dtype=torch.float64, device="cuda")

        def call():
            rc = lib.t2d_curve_lines(0, n, words.data_ptr(), start.data_ptr(), radius, step, L.CURVE_DUBINS, max_points, xy.data_ptr(),
                                     yaw.data_ptr(), count.data_ptr(), end.data_ptr(), stream)
            assert rc == 0
        st = stats(call)
        c = count.cpu().numpy().astype(np.int64)
        stored = int(np.minimum(c, max_points).sum())
        nbytes = 24 * stored + 28 * n
        rows.append(dict(what="curve_lines", n=n, step=step, max_points=max_points, points_stored=stored, truncated=int((c > max_points).sum()),
                         bytes_stored=nbytes, store_floor_us=round(nbytes / COPY_RATE * 1e6, 2), **st))
        print(json.dumps(rows[-1]), flush=True)
    # curve_routes: one env per curve, one 256-vertex route per env
    table, names = full_type_table()
    ty = names.index(list(VEHICLE_TEMPLATE)[0] + ":kin")
    pool = ParticipantPool(n, 1)
    pool.set_param_table(table)
    pool.set_status_config(max_step=100000)
    z = np.zeros(n, np.float32)
    pool.reset(z, z, z, z, np.full(n, ty, np.uint8))
    cap = 256
    t = np.linspace(0, 1, cap, dtype=np.float32)
    vo = (np.arange(n + 1) * cap).astype(np.int32)
    xyv = np.tile(np.stack([t, 0 * t], 1), (n, 1)).astype(np.float32)
    pool.set_routes((np.arange(n + 1, dtype=np.int32), vo, xyv.reshape(-1)), np.arange(n), 0, 1.0)
    count = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        rc = lib.t2d_curve_routes(pool._h, words.data_ptr(), start.data_ptr(), radius, 0.5, L.CURVE_DUBINS, 0, count.data_ptr(), stream)
        assert rc == 0
    st = stats(call)
    rows.append(dict(what="curve_routes", n_env=n, step=0.5, capacity=cap, bytes_stored=8 * cap * n + 4 * n,
                     store_floor_us=round((8 * cap * n + 4 * n) / COPY_RATE * 1e6, 2), **st))
    print(json.dumps(rows[-1]), flush=True)
    pool.close()
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
