"""The off-route detector: one `t2d_off_route` launch (A) against the same quantity as a torch expression on the device (B).

    python scripts/time_off_route.py [--reps 7] [--out profiles/off_route.json] [--a-only]

B is what a user can do without the detector and without leaving the device: the pool's zero-copy x / y columns, the routes as
padded fp64 tensors [N, S] made once (outside the timing), and one broadcast expression -- the detector's own arithmetic,
operation for operation -- giving distance and verdict.  A and B are asserted equal in their verdicts.

Shapes: highway 1024 x 64 (4 lane centres of 2 vertices, one shared set), intersection 2048 x 32 (12 paths of 9 - 14 vertices,
one shared set), the metric scene (mixed 4096 x 64) with the 33-vertex traces of its own rollout, and the same with 128-vertex
traces.  A B A B ... `--reps` windows each of back-to-back launches, device events around work that ends in a synchronise;
`record_kernel` (DeviceTrajectory.record, the pool's streaming yardstick) is timed in the same run at 4096 x 64.

--a-only: 50 launches of A per shape, for a `rocprofv3 --kernel-trace --stats` run of its own.
One JSON object on stdout (and in --out)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tactics2d_amd import layout as L, scenarios as S
from tactics2d_amd.history import DeviceTrajectory
from tactics2d_amd.pool import ParticipantPool

INNER_A = 200
LANES_Y = [-5.625, -1.875, 1.875, 5.625]


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def series(us):
    return dict(us=[round(t, 2) for t in us], mean_us=round(float(np.mean(us)), 2), median_us=round(float(np.median(us)), 2),
                min_us=round(min(us), 2), max_us=round(max(us), 2))


def intersection_paths(half=70.0):
    """12 paths: each arm's inbound lane centre sampled every 8 m, then the outbound lane of one of the three other arms"""
    arms = [(1, 0), (-1, 0), (0, 1), (0, -1)]
    inb = lambda m, d: (arms[m][0] * d, -arms[m][0] * 1.875) if arms[m][0] else (arms[m][1] * 1.875, arms[m][1] * d)
    outb = lambda m, d: (arms[m][0] * d, arms[m][0] * 1.875) if arms[m][0] else (-arms[m][1] * 1.875, arms[m][1] * d)
    routes = []
    for m in range(4):
        for k, ex in enumerate([e for e in range(4) if e != m]):
            pts = [inb(m, d) for d in np.arange(half, 5.9, -8.0)] + [outb(ex, d) for d in np.arange(6.0, half + 0.1, 16.0 + 8 * k)]
            routes.append(np.float32(pts))
    return routes


def torch_expression(x, y, VX, VY, nvert, thr, active):
    """the detector's arithmetic as one broadcast expression: x, y f32 [N]; VX, VY f64 [N, S]; nvert i32 [N]"""
    px, py = x.double()[:, None], y.double()[:, None]
    ax, ay, bx, by = VX[:, :-1], VY[:, :-1], VX[:, 1:], VY[:, 1:]
    ux, uy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L2 = ux * ux + uy * uy
    t = wx * ux + wy * uy
    vx, vy = px - bx, py - by
    c = wx * uy - wy * ux
    d2 = torch.where(t <= 0, wx * wx + wy * wy, torch.where(t >= L2, vx * vx + vy * vy, (c * c) / L2))
    seg = torch.arange(VX.shape[1] - 1, device=VX.device)[None, :]
    d2 = torch.where(seg + 1 < nvert[:, None], d2, torch.full_like(d2, float("inf")))
    d = torch.sqrt(d2.min(1).values)
    live = active & (nvert >= 2) & torch.isfinite(x) & torch.isfinite(y)
    off = live & (d > thr.double())
    return torch.where(live, d, torch.full_like(d, float("nan"))).float(), off


def measure(name, pool, VX, VY, nvert, thr, reps, stream, a_only, bytes_per_participant):
    dev = "cuda"
    x, y = (torch.as_tensor(pool.device_array(f), device=dev) for f in (L.F_X, L.F_Y))
    n = pool.n
    run_a = lambda: [pool.off_route(None, None, stream) for _ in range(INNER_A)]
    if a_only:
        for _ in range(50):
            pool.off_route(None, None, stream)
        torch.cuda.synchronize()
        return dict(shape=name, launches=50)
    thr_t = torch.as_tensor(thr, device=dev)
    nv_t = torch.as_tensor(nvert.astype(np.int32), device=dev)
    active = torch.as_tensor(((pool.download(L.F_IDS) >> 16) & 0xff) != 0, device=dev)
    b = lambda: torch_expression(x, y, VX, VY, nv_t, thr_t, active)
    inner_b = 20 if VX.shape[1] <= 16 else 5
    run_b = lambda: [b() for _ in range(inner_b)]
    for _ in range(2):
        run_a(); run_b()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        ta.append(timed(run_a) / INNER_A * 1e3)
        tb.append(timed(run_b) / inner_b * 1e3)
    d_a, off_a = pool.off_route_host()
    d_b, off_b = b()
    off_b, d_b = off_b.cpu().numpy().reshape(off_a.shape), d_b.cpu().numpy().reshape(d_a.shape)
    assert (off_a == off_b).all(), (name, int((off_a != off_b).sum()))
    same_bits = bool((d_a.view(np.uint32) == d_b.view(np.uint32)).all())
    a, bb = series(ta), series(tb)
    spread = max(a["max_us"] - a["min_us"], bb["max_us"] - bb["min_us"])
    assert bb["mean_us"] - a["mean_us"] > spread, (name, a, bb)
    gbs = bytes_per_participant * n / (a["mean_us"] * 1e-6) / 1e9
    return dict(shape=name, participants=n, vertices_per_route=int(nvert.max()), A_off_route=a, B_torch_expression=bb,
                launches_per_window=dict(A=INNER_A, B=inner_b), speedup=round(bb["mean_us"] / a["mean_us"], 1),
                verdicts_equal=True, distance_bits_equal=same_bits, off_route_share=round(float(off_a.mean()), 4),
                bytes_per_participant=bytes_per_participant, GB_per_s=round(gbs, 1))


def set_shape(name, sc, routes, route_of, thr, reps, stream, a_only):
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    thr = np.full(sc.n, thr, np.float32)
    pool.set_routes([routes], None, route_of, thr)
    S_ = max(len(r) for r in routes)
    R = np.zeros((len(routes), S_, 2))
    for k, r in enumerate(routes):
        R[k, :len(r)] = r
    nv = np.array([len(r) for r in routes])
    sel = np.maximum(route_of, 0)
    V = torch.as_tensor(R[sel], device="cuda")
    nvert = np.where(route_of < 0, 0, nv[sel])
    # x, y, ids, route_of, threshold read + distance and verdict written; the set's vertices come out of LDS
    out = measure(name, pool, V[..., 0].contiguous(), V[..., 1].contiguous(), nvert, thr, reps, stream, a_only, 4 * 5 + 4 + 1)
    pool.close()
    return out


def trace_shapes(reps, stream, a_only):
    sc = S.mixed(4096, 64, seed=3)
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    pool.set_actions(*sc.sample_actions(np.random.default_rng(0)))
    traj = DeviceTrajectory(pool, 0, capacity=128)
    traj.record(pool, 0, stream)
    for k in range(1, 128):
        pool.step(100, stream)
        traj.record(pool, k * 100, stream)
    pool.set_actions(*sc.sample_actions(np.random.default_rng(1)))   # (then off the recording: other actions for five steps)
    for _ in range(5):
        pool.step(100, stream)
    pool.sync()
    out = []
    cols = [torch.as_tensor(traj.column(c), device="cuda") for c in ("x", "y")]     # [128, N]
    thr = np.full(sc.n, 0.5, np.float32)
    for n_slots in (33, 128):
        last = np.full(sc.n, n_slots - 1, np.int32)
        pool.set_routes_from(traj, windows=(np.zeros(sc.n, np.int32), last), threshold=thr)
        VX, VY = (c[:n_slots].double().t().contiguous() for c in cols)
        out.append(measure(f"metric scene 4096 x 64, {n_slots}-vertex traces", pool, VX, VY, last + 1, thr, reps, stream, a_only,
                           8 * n_slots + 4 * 5 + 4 + 1))
    rec = None
    if not a_only:   # the pool's streaming yardstick in the same run
        buf = traj._buf
        run = lambda: [buf.record(127, stream) for _ in range(INNER_A)]
        run(); torch.cuda.synchronize()
        rec = series([timed(run) / INNER_A * 1e3 for _ in range(reps)])
    pool.clear_routes()
    traj.close()
    pool.close()
    return out, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--a-only", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows = []
    hw = S.highway(1024, 64, seed=1)
    lane = np.abs(hw.y.astype(np.float64)[:, None] - np.float64(LANES_Y)[None, :]).argmin(1).astype(np.int32)
    rows.append(set_shape("highway 1024 x 64, 4 routes x 2 vertices", hw, [np.float32([[-210, ly], [210, ly]]) for ly in LANES_Y], lane,
                          0.2, args.reps, stream, args.a_only))
    ix = S.intersection(2048, 32, seed=2)
    k = np.arange(ix.n) % ix.A
    rows.append(set_shape("intersection 2048 x 32, 12 paths", ix, intersection_paths(), ((k % 4) * 3 + (k // 4) % 3).astype(np.int32),
                          0.15, args.reps, stream, args.a_only))
    traces, rec = trace_shapes(args.reps, stream, args.a_only)
    res = dict(script="scripts/time_off_route.py", device=torch.cuda.get_device_name(0), shapes=rows + traces,
               record_kernel_4096x64=rec, not_measured=["replay_kernel in the same run (needs a pool of replayed rows)"])
    print(json.dumps(res), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
