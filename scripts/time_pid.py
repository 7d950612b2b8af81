"""Time of the lane-keeping PID launch: A = one t2d_pid_actions (cross-track + the IDM law) against B = t2d_idm_actions followed
by t2d_off_route, the two existing launches whose work it combines (one leader sweep, one route sweep).

    python scripts/time_pid.py [--reps 7] [--limit 300] [--out profiles/pid.json]

The parent process never touches the GPU: it starts the measurement as a child under `timeout -k 10 <limit>` and passes its
exit status on, so a hang ends the probe instead of holding the device.

Child: the metric scene (mixed: highway / roundabout / intersection envs) at 1024 x 64 and 4096 x 64 with the shared route set
of tests/route_scenes.py (the routes the off-route tests use).  One pool per shape; a participant is PID-controlled or
IDM-controlled, never both, so the pool is re-installed between windows (outside the timing): A -- every participant with a
route PID-controlled (cross-track error, longitudinal = the IDM law, IDM rows installed with nobody assigned); B -- the same
participants IDM-controlled.  A ramp of 3000 launches, then A B A B ... `--reps` windows each of 200 launches between device
events, every window behind 100 untimed launches of its own kind.  One JSON line per shape on stdout, all of them in --out: the
raw windows (us per launch) with mean, min and max.  Asserts nothing.  Kernel names for a `rocprofv3 --kernel-trace --stats` run
of its own: pid_kernel, idm_kernel, off_route_set_kernel."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INNER = 200


def child(args):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch

    import route_scenes as RS
    from tactics2d_amd import layout as L, scenarios as S
    from tactics2d_amd.controller import IDMController, PIDController
    from tactics2d_amd.pool import ParticipantPool

    def window(fn, ramp=100):
        for _ in range(ramp):
            fn()
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(INNER):
            fn()
        t1.record()
        t1.synchronize()
        return t0.elapsed_time(t1) * 1e3 / INNER

    def series(us):
        return dict(us=[round(t, 2) for t in us], mean_us=round(float(np.mean(us)), 2), min_us=round(min(us), 2), max_us=round(max(us), 2))

    rows = []
    for n_env in (1024, 4096):
        sc = S.mixed(n_env, 64, seed=6)
        route_sets, set_of_env, route_of, thr = RS.build(sc, "shared")
        pool = ParticipantPool(sc.n_env, sc.A)
        sc.load(pool)
        pool.set_routes(route_sets, set_of_env, route_of, thr)
        routed = route_of >= 0
        idm_rows = IDMController().row()[None]
        idm_on, idm_off = np.where(routed, 0, L.IDM_NONE).astype(np.uint8), np.full(sc.n, L.IDM_NONE, np.uint8)
        pid_row = PIDController(dt=0.1, longitudinal="idm").row()[None]
        pid_on = np.where(routed, 0, L.PID_NONE).astype(np.uint8)
        act = torch.zeros((sc.n, 2), dtype=torch.float32, device="cuda")
        rec = torch.zeros((sc.n, L.PID_RECORD_BYTES // 8), dtype=torch.float64, device="cuda")
        dist = torch.zeros(sc.n, dtype=torch.float32, device="cuda")
        off = torch.zeros(sc.n, dtype=torch.uint8, device="cuda")

        def install(kind):
            if kind == "A":
                pool.set_idm(idm_rows, idm_off)
                pool.set_pid(pid_row, pid_on, sc.speed)
            else:
                pool.set_pid(None)
                pool.set_idm(idm_rows, idm_on)

        run_a = lambda: pool.pid_actions(None, act.data_ptr(), rec.data_ptr())

        def run_b():
            pool.idm_actions()
            pool.off_route(dist.data_ptr(), off.data_ptr())

        install("A")
        for _ in range(3000):
            run_a()
        torch.cuda.synchronize()
        a, b = [], []
        for _ in range(args.reps):
            install("A")
            a.append(window(run_a))
            install("B")
            b.append(window(run_b))
        rows.append(dict(what="pid_actions vs idm_actions + off_route", scene="mixed", n_env=n_env, max_agents=64,
                         controlled=int(routed.sum()), launches_per_window=INNER, A_pid_actions=series(a), B_idm_plus_off_route=series(b)))
        print(json.dumps(rows[-1]), flush=True)
        pool.close()
    if args.out:
        with open(args.out, "w") as f:
            json.dump(rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds the GPU child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    cmd += ["--out", args.out] if args.out else []
    return subprocess.run(cmd).returncode


if __name__ == "__main__":
    sys.exit(main())
