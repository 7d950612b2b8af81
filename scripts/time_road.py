"""Time of the road launches: t2d_spiral_curves, t2d_param_poly3_curves and t2d_planview_lines for batches, t2d_planview_routes for
the envs of a pool.

    python scripts/time_road.py [--reps 5] [--limit 240] [--small] [--out profiles/road.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child, per shape: the inputs are resident on the device and the outputs are allocated once; after a ramp of 200 launches,
`--reps` windows of 1000 launches each, every launch one ctypes call of the C entry point, device events around a window that
ends in a synchronise.  What a row holds is the time from launch to launch in such a loop: the kernel AND whatever the host and
the queue add between two back-to-back launches; the kernels' own times come from a rocprofv3 run of its own.
  spiral           n = 4096 spirals of the Fresnel branch (k0 != 0, either sign of gamma), n_interpolation 100, both rules
  param_poly3      n = 4096 curves of 20 - 40 m (200 - 400 points each), both pRange kinds
  planview_lines   n = 4096 roads straight - clothoid - arc - clothoid - straight of about 125 m (about 1 060 kept points), xy + s + kappa
  planview_routes  one such road per env of a pool of 4096 envs x 1 whose route sets hold one 160-vertex route each, stride 10
Every row stands beside the STORE FLOOR of its launch: the bytes it must write (16 per point, + 16 with s and kappa, + 4 per row;
8 per route vertex) over 6.29 TB/s, the copy rate measured on this GPU -- a floor for the stores alone, it leaves out the launch
and the arithmetic of each point.
One JSON line per measurement on stdout (and in --out): the median and the spread (max - min) of the per-launch times in
microseconds.  Kernel names for a `rocprofv3 --kernel-trace --stats` run: spiral_curves_kernel, param_poly3_curves_kernel,
planview_kernel<0|1>."""
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

    from tactics2d_amd import _ffi, interpolator as I, layout as L
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
    dev = lambda a, dt=np.float64: torch.as_tensor(np.ascontiguousarray(a, dt), device="cuda")

    par = dev(np.stack([rng.uniform(10, 40, n), rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(-3, 3, n),
                        rng.uniform(0.01, 0.05, n), rng.choice([-1, 1], n) * rng.uniform(0.001, 0.01, n)], 1))
    xy = torch.empty((n, ni, 2), dtype=torch.float64, device="cuda")
    count = torch.empty(n, dtype=torch.int32, device="cuda")
    for rule, name in ((L.SPIRAL_REFERENCE, "reference"), (L.SPIRAL_STANDARD, "standard")):
        def call():
            assert lib.t2d_spiral_curves(0, n, par.data_ptr(), ni, rule, ni, xy.data_ptr(), count.data_ptr(), stream) == 0
        st = stats(call)
        assert (count == ni).all()
        nbytes = 16 * ni * n + 4 * n
        rows.append(dict(what="spiral", rule=name, n=n, n_interpolation=ni, bytes_stored=nbytes,
                         store_floor_us=round(nbytes / COPY_RATE * 1e6, 2), **st))
        print(json.dumps(rows[-1]), flush=True)

    length = rng.uniform(20, 40, n)
    arc = np.arange(n) % 2
    k = np.where(arc == 1, 1.0, length)
    pp = dev(np.stack([length, rng.uniform(-100, 100, n), rng.uniform(-100, 100, n), rng.uniform(-3, 3, n), 0 * k, k,
                       rng.uniform(-0.01, 0.01, n) * k ** 2, rng.uniform(-0.001, 0.001, n) * k ** 3, 0 * k, rng.uniform(-0.05, 0.05, n) * k,
                       rng.uniform(-0.01, 0.01, n) * k ** 2, rng.uniform(-0.001, 0.001, n) * k ** 3], 1))
    p_range = dev(arc, np.int32)
    xy = torch.empty((n, 400, 2), dtype=torch.float64, device="cuda")

    def call():
        assert lib.t2d_param_poly3_curves(0, n, pp.data_ptr(), p_range.data_ptr(), 400, xy.data_ptr(), count.data_ptr(), stream) == 0
    st = stats(call)
    points = int(count.sum())
    nbytes = 16 * points + 4 * n
    rows.append(dict(what="param_poly3", n=n, points=points, bytes_stored=nbytes, store_floor_us=round(nbytes / COPY_RATE * 1e6, 2), **st))
    print(json.dumps(rows[-1]), flush=True)

    roads = []
    for e in range(n):
        kap = float(rng.choice([-1, 1]) * rng.uniform(0.03, 0.05))
        x, y, h, s, road = 0.0, float(rng.uniform(-3, 3)), float(rng.uniform(-0.3, 0.3)), 0.0, []
        for kind, ln, k0, k1 in (("line", 30.3, 0, 0), ("spiral", 20.2, 0.0, kap), ("arc", 25.5, kap, kap), ("spiral", 20.2, kap, 0.0), ("line", 30.3, 0, 0)):
            g = dict(type=kind, s=s, x=x, y=y, hdg=h, length=ln, curvStart=k0, curvEnd=k1, curvature=kap)
            road.append(g)
            # (the start of the next geometry: a coarse walk along the curvature is all a timing needs)
            for t in np.linspace(0, 1, 200, endpoint=False):
                hh = h + (k0 + (k1 - k0) * t / 2) * ln * t
                x, y = x + np.cos(hh) * ln / 200, y + np.sin(hh) * ln / 200
            s, h = s + ln, h + (k0 + k1) / 2 * ln
        roads.append(road)
    rec, ng = I.pack_planview(roads)
    rec, ng = rec.cuda(), ng.cuda()
    mp = 1280
    xy = torch.empty((n, mp, 2), dtype=torch.float64, device="cuda")
    sv, kv = torch.empty((n, mp), dtype=torch.float64, device="cuda"), torch.empty((n, mp), dtype=torch.float64, device="cuda")

    def call():
        assert lib.t2d_planview_lines(0, n, rec.data_ptr(), ng.data_ptr(), 5, L.SPIRAL_STANDARD, mp, xy.data_ptr(), sv.data_ptr(), kv.data_ptr(),
                                      count.data_ptr(), stream) == 0
    st = stats(call)
    points = int(count.sum())
    assert int(count.max()) <= mp and int(count.min()) > 900
    nbytes = 32 * points + 4 * n
    rows.append(dict(what="planview_lines", n=n, geometries=5, kept_points=points, bytes_stored=nbytes,
                     store_floor_us=round(nbytes / COPY_RATE * 1e6, 2), **st))
    print(json.dumps(rows[-1]), flush=True)

    table, names = full_type_table()
    ty = names.index(list(VEHICLE_TEMPLATE)[0] + ":kin")
    pool = ParticipantPool(n, 1)
    pool.set_param_table(table)
    pool.set_status_config(max_step=100000)
    z = np.zeros(n, np.float32)
    pool.reset(z, z, z, z, np.full(n, ty, np.uint8))
    cap = 160
    t = np.linspace(0, 1, cap, dtype=np.float32)
    vo = (np.arange(n + 1) * cap).astype(np.int32)
    xyv = np.tile(np.stack([t, 0 * t], 1), (n, 1)).astype(np.float32)
    pool.set_routes((np.arange(n + 1, dtype=np.int32), vo, xyv.reshape(-1)), np.arange(n), 0, 1.0)
    rcount = torch.zeros(n, dtype=torch.int32, device="cuda")

    def call():
        assert lib.t2d_planview_routes(pool._h, rec.data_ptr(), ng.data_ptr(), 5, L.SPIRAL_STANDARD, 10, 0, rcount.data_ptr(), stream) == 0
    st = stats(call)
    assert int(rcount.max()) < cap
    rows.append(dict(what="planview_routes", n_env=n, stride=10, capacity=cap, bytes_stored=8 * cap * n + 4 * n,
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
