"""Time of the scripted launches that stage an env's route set: C = one t2d_pursuit_actions with pure pursuit + cruise, D = the
same with ACC (the leader rule and the extra LDS staging), P = one t2d_pid_actions (cross-track error + the IDM law, the case
of scripts/time_pid.py) and O = one set-route t2d_off_route, all on the same pool -- and, with --parent-lib, the same four
through a library built from the parent commit, with a SHA-256 per kind over what one launch directly after a fresh install
wrote (action rows and records; distances and verdicts for O), outside the timing.

    python scripts/time_pursuit.py [--reps 7] [--limit 300] [--out profiles/scripted_shared.json]
                                   [--parent-lib libt2d_hip_parent.so [--parent-first]]

--parent-lib names a library file beside libt2d_hip.so in tactics2d_amd/ (build the parent commit's tree with
T2D_LIB_NAME=libt2d_hip_parent.so and copy the file over); it is loaded by a child process of its own, after the first
(--parent-first: before it).  With both in --out the parent process appends the comparison: per shape and kind whether the
digests are equal, and the product's mean against the parent library's mean and spread (max - min of its windows).

The parent process never touches the GPU: it starts each measurement as a child under `timeout -k 10 <limit>` and passes the
first non-zero exit status on; a failing child ends the probe.

Child: the metric scene (mixed: highway / roundabout / intersection envs) at 1024 x 64 and 4096 x 64 with the shared route set
of tests/route_scenes.py.  One pool per shape; a participant has one controller, so the pool is re-installed between windows
(outside the timing), every participant with a route controlled.  A ramp of 3000 launches, then C D P O C D P O ... `--reps`
windows each of 200 launches between device events, every window behind 100 untimed launches of its own kind.  One JSON line
per shape on stdout, all of them in --out: the raw windows (us per launch) with mean, min and max.  Asserts nothing.  Kernel
names for a `rocprofv3 --kernel-trace --stats` run of its own: pursuit_kernel, pid_kernel, off_route_set_kernel."""
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
    import hashlib

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
        idm_off = np.full(sc.n, L.IDM_NONE, np.uint8)
        pid_row = PIDController(dt=0.1, longitudinal="idm").row()[None]
        on = np.where(routed, 0, 255).astype(np.uint8)
        act = torch.zeros((sc.n, 2), dtype=torch.float32, device="cuda")
        rec = torch.zeros((sc.n, 16), dtype=torch.float64, device="cuda")   # (room for either kind of record)
        dist = torch.zeros(sc.n, dtype=torch.float32, device="cuda")
        off = torch.zeros(sc.n, dtype=torch.uint8, device="cuda")
        pool.set_idm(idm_rows, idm_off)

        def install(kind):
            if kind == "P":
                pool.set_pursuit(None)
                pool.set_pid(pid_row, on, sc.speed)
            elif kind != "O":
                from tactics2d_amd.controller import PurePursuitController
                pool.set_pid(None)
                pool.set_pursuit(PurePursuitController(5.0).row("cruise" if kind == "C" else "acc")[None], on, np.abs(sc.speed))

        run_p = lambda: pool.pid_actions(None, act.data_ptr(), rec.data_ptr())
        run_c = lambda: pool.pursuit_actions(None, act.data_ptr(), rec.data_ptr())
        run_o = lambda: pool.off_route(dist.data_ptr(), off.data_ptr())
        kinds = [("C", run_c), ("D", run_c), ("P", run_p), ("O", run_o)]
        digest = {}
        for k, fn in kinds:   # one launch directly after a fresh install (PID's state starts from zero), outside the timing
            install(k)
            for t in (act, rec, dist, off):
                t.zero_()
            fn()
            torch.cuda.synchronize()
            digest[k] = hashlib.sha256(b"".join(t.cpu().numpy().tobytes() for t in ((dist, off) if k == "O" else (act, rec)))).hexdigest()
        install(kinds[0][0])
        for _ in range(3000):
            kinds[0][1]()
        torch.cuda.synchronize()
        us = {k: [] for k, _ in kinds}
        for _ in range(args.reps):
            for k, fn in kinds:
                install(k)
                us[k].append(window(fn))
        names = dict(C="C_pursuit_cruise", D="D_pursuit_acc", P="P_pid_actions", O="O_off_route_sets")
        row = dict(what="pursuit_actions (cruise, ACC) beside pid_actions", library=os.environ.get("T2D_LIB_NAME", "libt2d_hip.so"),
                   scene="mixed", n_env=n_env, max_agents=64, controlled=int(routed.sum()), launches_per_window=INNER)
        # what the controlled participants met in this scene: one more ACC launch, into the pool's own records (72 bytes each)
        install("D")
        pool.pursuit_actions(None, act.data_ptr(), None)
        torch.cuda.synchronize()
        own = pool.pursuit_records()
        ev, lead = own["events"].cpu().numpy()[routed], own["leader"].cpu().numpy()[routed]
        row.update(acc_with_leader=int((lead >= 0).sum()), wrapped=int(((ev & L.PURSUIT_WRAPPED) != 0).sum()),
                   route_end=int(((ev & L.PURSUIT_ROUTE_END) != 0).sum()), nonfinite=int(((ev & L.PURSUIT_NONFINITE) != 0).sum()))
        row.update({names[k]: dict(series(v), sha256=digest[k]) for k, v in us.items()})
        rows.append(row)
        print(json.dumps(row), flush=True)
        pool.close()
    if args.out:
        old = []
        if args.append and os.path.exists(args.out):
            with open(args.out) as f:
                old = json.load(f)
        with open(args.out, "w") as f:
            json.dump(old + rows, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--limit", type=int, default=300, help="seconds each GPU child may take")
    ap.add_argument("--out", default=None)
    ap.add_argument("--parent-lib", default=None, help="file name of a library built from the parent commit, in tactics2d_amd/")
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--append", action="store_true", help="child: keep what --out already holds")
    ap.add_argument("--parent-first", action="store_true", help="run the parent library's child before the product's")
    args = ap.parse_args()
    if args.child:
        return child(args)
    cmd = ["timeout", "-k", "10", str(args.limit), sys.executable, os.path.abspath(__file__), "--child", "--reps", str(args.reps)]
    cmd += ["--out", args.out] if args.out else []
    envs = [dict(os.environ)] + ([dict(os.environ, T2D_LIB_NAME=args.parent_lib)] if args.parent_lib else [])
    for k, env in enumerate(envs[::-1] if args.parent_first else envs):
        rc = subprocess.run(cmd + (["--append"] if k else []), env=env).returncode   # (the second only if the first exited 0)
        if rc:
            return rc
    if args.parent_lib and args.out:
        compare(args.out, args.parent_lib)
    return 0


def compare(path, parent_lib):
    """the product's rows against the parent library's, shape by shape and kind by kind (host arithmetic on the JSON)"""
    with open(path) as f:
        rows = json.load(f)
    verdict = dict(what="product against the parent library, same run", parent_library=parent_lib, rows=[])
    for new in [r for r in rows if r.get("library") == "libt2d_hip.so"]:
        old = next(r for r in rows if r.get("library") == parent_lib and r["n_env"] == new["n_env"])
        for kind in [k for k in new if isinstance(new[k], dict) and "sha256" in new[k]]:
            spread = round(old[kind]["max_us"] - old[kind]["min_us"], 2)
            excess = round(new[kind]["mean_us"] - old[kind]["mean_us"], 2)
            verdict["rows"].append(dict(n_env=new["n_env"], kind=kind, same_sha256=new[kind]["sha256"] == old[kind]["sha256"],
                                        mean_us=new[kind]["mean_us"], parent_mean_us=old[kind]["mean_us"], parent_spread_us=spread,
                                        excess_us=excess, within_parent_spread=excess <= spread))
            print(json.dumps(verdict["rows"][-1]), flush=True)
    with open(path, "w") as f:
        json.dump(rows + [verdict], f, indent=1)


if __name__ == "__main__":
    sys.exit(main())
