"""Time of the spline launches: t2d_spline_curves for batches of control polygons and t2d_spline_routes for the envs of a pool.

    python scripts/time_splines.py [--reps 5] [--limit 240] [--small] [--out profiles/splines.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape: the inputs are resident on the device and the outputs are allocated once; after a ramp of 200 launches,
`--reps` windows of 1000 launches each, every launch one ctypes call of the C entry point, device events around a window that
ends in a synchronise.  What a row holds is the time from launch to launch in such a loop: the kernel AND whatever the host and
the queue add between two back-to-back launches; the kernels' own times come from a rocprofv3 run of its own.
  bezier         n = 4096 curves of 8 control points, n_interpolation 100
  bspline        n = 4096 cubic (degree 3) B-splines of 16 control points, the default knots, n_interpolation 100
  cubic          n = 4096 not-a-knot cubic splines of 16 control points, n_interpolation 100 (1501 points each)
  spline_routes  one such B-spline per env of a pool of 4096 envs x 1 whose route sets hold one 128-vertex route each
Every row stands beside the STORE FLOOR of its launch: the bytes it must write (16 per point + 4 per curve; 8 per route vertex)
over 6.29 TB/s, the copy rate measured on this GPU -- a floor for the stores alone, it leaves out the launch, the serial set-up
of each curve and the arithmetic of each point --, and beside the reference's compiled module on one CPU core, as
tests/golden/make_splines.py timed it where the fixture was made (REFERENCE_US, per curve, times n).
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch times in
microseconds.  Kernel names for a `rocprofv3 --kernel-trace --stats` run: spline_curves_kernel<0|1|2>, spline_routes_kernel<1>."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER, RAMP = 1000, 200
COPY_RATE = 6.29e12   # bytes per second: the float4 copy measured on an MI355X
REFERENCE_US = {"bezier": 29.5, "bspline": 83.3, "cubic": 491.6}   # per call of the reference's get_curve (make_splines.py's print-out)


def child(args):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    from tactics2d_amd import _ffi, layout as L
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

    rows = []
    rng = np.random.default_rng(0)
    n, ni = (512 if args.small else 4096), 100
    shapes = (("bezier", L.SPLINE_BEZIER, 8, 0, L.SPLINE_NOT_A_KNOT), ("bspline", L.SPLINE_BSPLINE, 16, 3, L.SPLINE_NOT_A_KNOT),
              ("cubic", L.SPLINE_CUBIC, 16, 0, L.SPLINE_NOT_A_KNOT))
    inputs = {}
    for what, kind, m, degree, boundary in shapes:
        pts = np.stack([np.cumsum(rng.uniform(0.5, 6.0, (n, m)), 1), rng.uniform(-8.0, 8.0, (n, m))], 2)
        ctrl = torch.as_tensor(pts, device="cuda")
        n_ctrl = torch.full((n,), m, dtype=torch.int32, device="cuda")
        inputs[what] = (ctrl, n_ctrl)
        points = (m - 1) * ni + 1 if kind == L.SPLINE_CUBIC else ni
        xy = torch.empty((n, points, 2), dtype=torch.float64, device="cuda")
        count = torch.empty(n, dtype=torch.int32, device="cuda")

        def call():
            rc = lib.t2d_spline_curves(0, n, kind, ctrl.data_ptr(), n_ctrl.data_ptr(), m, ni, degree, None, boundary, None, points,
                                       xy.data_ptr(), count.data_ptr(), stream)
            assert rc == 0
        st = stats(call)
        assert (count == points).all()
        nbytes = 16 * points * n + 4 * n
        rows.append(dict(what=what, n=n, n_ctrl=m, n_interpolation=ni, degree=degree, points_per_curve=points, bytes_stored=nbytes,
                         store_floor_us=round(nbytes / COPY_RATE * 1e6, 2), reference_cpu_us=round(REFERENCE_US[what] * n, 1), **st))
        print(json.dumps(rows[-1]), flush=True)
    # spline_routes: one env per curve, one 128-vertex route per env
    table, names = full_type_table()
    ty = names.index(list(VEHICLE_TEMPLATE)[0] + ":kin")
    pool = ParticipantPool(n, 1)
    pool.set_param_table(table)
    pool.set_status_config(max_step=100000)
    z = np.zeros(n, np.float32)
    pool.reset(z, z, z, z, np.full(n, ty, np.uint8))
    cap = 128
    t = np.linspace(0, 1, cap, dtype=np.float32)
    vo = (np.arange(n + 1) * cap).astype(np.int32)
    xyv = np.tile(np.stack([t, 0 * t], 1), (n, 1)).astype(np.float32)
    pool.set_routes((np.arange(n + 1, dtype=np.int32), vo, xyv.reshape(-1)), np.arange(n), 0, 1.0)
    count = torch.zeros(n, dtype=torch.int32, device="cuda")
    ctrl, n_ctrl = inputs["bspline"]

    def call():
        rc = lib.t2d_spline_routes(pool._h, L.SPLINE_BSPLINE, ctrl.data_ptr(), n_ctrl.data_ptr(), 16, ni, 3, None, 0, None, 0,
                                   count.data_ptr(), stream)
        assert rc == 0
    st = stats(call)
    rows.append(dict(what="spline_routes", n_env=n, kind="bspline", n_ctrl=16, n_interpolation=ni, capacity=cap,
                     bytes_stored=8 * cap * n + 4 * n, store_floor_us=round((8 * cap * n + 4 * n) / COPY_RATE * 1e6, 2), **st))
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
