"""The lidar scan of every participant: one t2d_lidar_scan_all (A) against what there was before it (B).

    python scripts/time_lidar_all.py [--reps 5] [--out profiles/lidar_all.json] [--b-only] [--a-only] [--small]

A = one `pool.lidar_scan_all(out)`.
B = for j in range(max_agents): `pool.set_status_config(ego_index=j)`; `pool.lidar_scan(out_b[j])` -- max_agents launches and
    as many synchronising configuration calls, through entry points this library shares with its predecessors.

Per shape (highway 1024 x 64, intersection 2048 x 32, the metric scene mixed 4096 x 64; participants as obstacles; 120 and 360
beams at 20 m): both warmed up, then A, B, A, B, ... `--reps` times, each timed with device events around work that ends in a
synchronise; A and B must give the same bits, and A must be faster than B by more than the spread (max - min) of A's plus B's
own repeats -- the script exits non-zero otherwise.  Also timed: one fused `pool.step(100)` at the same shape, for scale.

--b-only: B alone (for a library built from older sources: `T2D_LIB_NAME=<that .so> T2D_ALLOW_MISSING_SYMBOLS=1`), to confirm
that B on this build is the older build's code path.  --a-only: 20 scans per shape and nothing else, for a
`rocprofv3 --kernel-trace --stats` run of its own (kernel name: lidar_all_kernel).  One JSON line per shape on stdout."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tactics2d_amd import scenarios as S
from tactics2d_amd.pool import ParticipantPool

HBM_COPY_TBS = 6.29   # measured copy bandwidth of the MI355X (spec 8.0 TB/s)
A_INNER = 10          # scans per timed window of A


def shapes(small):
    if small:
        return [("highway 64 x 64", lambda: S.highway(64, 64)), ("intersection 64 x 32", lambda: S.intersection(64, 32))]
    return [("highway 1024 x 64", lambda: S.highway(1024, 64)), ("intersection 2048 x 32", lambda: S.intersection(2048, 32)),
            ("metric mixed 4096 x 64", lambda: S.mixed(4096, 64, seed=3))]


def timed(fn):
    """milliseconds of fn() between two device events, ending in a synchronise"""
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--b-only", action="store_true")
    ap.add_argument("--a-only", action="store_true")
    ap.add_argument("--small", action="store_true")
    args = ap.parse_args()
    stream = torch.cuda.current_stream().cuda_stream
    rows, ok = [], True
    for name, make in shapes(args.small):
        sc = make()
        E, A = sc.n_env, sc.A
        pool = ParticipantPool(E, A)
        sc.load(pool)
        status = dict(sc.status)
        for beams in (120, 360):
            pool.lidar_config(beams, 20.0, True)
            out_a = torch.zeros((E, A, beams), dtype=torch.float32, device="cuda")
            out_b = torch.zeros((A, E, beams), dtype=torch.float32, device="cuda")
            slice_bytes = E * beams * 4

            def run_a():
                for _ in range(A_INNER):
                    pool.lidar_scan_all(out_a.data_ptr(), stream)

            def run_b():
                for j in range(A):
                    pool.set_status_config(**dict(status, ego_index=j))
                    pool.lidar_scan(out_b.data_ptr() + j * slice_bytes, stream)

            row = dict(shape=name, n_env=E, max_agents=A, beams=beams, out_bytes=E * A * beams * 4)
            if args.a_only:
                for _ in range(2):
                    run_a()
                torch.cuda.synchronize()
                rows.append(row)
                continue
            for _ in range(2):   # warm-up of every timed form at this shape (and the clocks: > 50 ms of work)
                if not args.b_only:
                    run_a()
                run_b()
            torch.cuda.synchronize()
            ta, tb = [], []
            for _ in range(max(5, args.reps)):
                if not args.b_only:
                    ta.append(timed(run_a) / A_INNER * 1e3)
                tb.append(timed(run_b) * 1e3)
            pool.set_status_config(**status)
            row.update(B_us=[round(t, 1) for t in tb], B_mean_us=round(float(np.mean(tb)), 1),
                       B_spread_us=round(max(tb) - min(tb), 1))
            if not args.b_only:
                same = bool(torch.equal(out_a.view(torch.int32), out_b.permute(1, 0, 2).contiguous().view(torch.int32)))
                finite = float(torch.isfinite(out_a).float().mean())
                spread = (max(ta) - min(ta)) + (max(tb) - min(tb))
                faster = float(np.mean(tb)) - float(np.mean(ta)) > spread
                row.update(A_us=[round(t, 1) for t in ta], A_mean_us=round(float(np.mean(ta)), 1),
                           A_spread_us=round(max(ta) - min(ta), 1), speedup=round(float(np.mean(tb) / np.mean(ta)), 2),
                           same_bits=same, finite_share=round(finite, 4), A_faster_by_more_than_the_spread=bool(faster),
                           A_out_TBs=round(row["out_bytes"] / (float(np.mean(ta)) * 1e-6) / 1e12, 3),
                           A_out_share_of_measured_hbm_copy=round(row["out_bytes"] / (float(np.mean(ta)) * 1e-6) / 1e12 / HBM_COPY_TBS, 3))
                ok = ok and same and faster and 0.0 < finite < 1.0
            rows.append(row)
            del out_a, out_b
        if not args.a_only:   # one fused step at the same shape, for scale (after the scans: it moves the poses)
            pool.set_actions(*sc.sample_actions(np.random.default_rng(0)))
            for _ in range(20):
                pool.step(100, stream)
            torch.cuda.synchronize()
            ts = [timed(lambda: [pool.step(100, stream) for _ in range(20)]) / 20 * 1e3 for _ in range(5)]
            for r in rows:
                if r["shape"] == name:
                    r["step_us"] = round(float(np.mean(ts)), 1)
        pool.close()
    for r in rows:
        print(json.dumps(r), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(dict(script="scripts/time_lidar_all.py", mode="b-only" if args.b_only else "a-only" if args.a_only else "ab",
                           library=os.environ.get("T2D_LIB_NAME", "libt2d_hip.so"), rows=rows), f, indent=1)
    if not ok:
        sys.exit("A is not faster than B by more than the spread, or A and B differ (see the rows above)")


if __name__ == "__main__":
    main()
