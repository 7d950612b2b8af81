"""The device racing-track generator beside the host class it replaces at reset time.

    python scripts/time_track_generate.py [--out profiles/track_generate.json] [--case generate|install|regenerate]

Without --case every case runs as a child process of its own under a time limit (a case that fails or runs out of time ends
the probe: nothing more is started on the device); the rows are merged into one JSON object on stdout (and in --out).

    generate     t2d_generate_tracks at 64 / 1024 / 4096 tracks: device events around REPS launches after WARM untimed ones,
                 per launch and per track; and `RacingTrackGenerator.generate()` on this machine's CPU (HOST_TRACKS tracks,
                 np.random.seed(0 ..)), the baseline, per track
    install      set_tracks_generated at 4096 envs (host clock around the synchronous call) against the host path on the same
                 tracks downloaded first: boundary + reset + snapshot + set_tracks (the host path's GENERATION time is the
                 `generate` case's host figure times 4096, not measured again)
    regenerate   4096 envs, VecRacingEnv.step_torch with auto_reset: the step without the regenerate launch
                 (new_track_per_episode=False: the baseline), with the launch when nobody finished, and the regenerate launch
                 alone when 1 % of the envs finished (their track status is set by hand before each timed launch)

Asserts nothing.  Every figure is the mean and the spread over REPS repeats."""
import argparse
import json
import os
import subprocess
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

WARM, REPS, HOST_TRACKS = 3, 10, 20
LIMITS = {"generate": 240, "install": 240, "regenerate": 240}   # seconds per case


def series(v):
    import numpy as np
    return dict(mean=round(float(np.mean(v)), 3), median=round(float(np.median(v)), 3), min=round(float(min(v)), 3),
                max=round(float(max(v)), 3), n=len(v))


def event_ms(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def case_generate():
    import numpy as np
    import torch
    from tactics2d_amd import _ffi, layout as L
    from tactics2d_amd.generator import RacingTrackGenerator
    out = {}
    for n in (64, 1024, 4096):
        dev = "cuda:0"
        tiles = torch.zeros((n, L.MAX_TRACK_TILES, 4, 2), device=dev)
        i32 = [torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4)]
        pose, line, bound = torch.zeros((n, 3), dtype=torch.float64, device=dev), torch.zeros((n, 2, 2), device=dev), torch.zeros((n, 4), device=dev)
        s = torch.cuda.current_stream().cuda_stream
        seed = [0]

        def launch():
            seed[0] += 1
            _ffi.check(_ffi.lib().t2d_generate_tracks(0, n, seed[0], 0, 4.284, tiles.data_ptr(), i32[0].data_ptr(), i32[1].data_ptr(),
                                                      i32[2].data_ptr(), pose.data_ptr(), line.data_ptr(), bound.data_ptr(),
                                                      i32[3].data_ptr(), s))
        for _ in range(WARM):
            launch()
        torch.cuda.synchronize()
        ms = [event_ms(launch) for _ in range(REPS)]
        out[f"generate_{n}"] = dict(ms_per_launch=series(ms), us_per_track=round(1e3 * float(np.mean(ms)) / n, 3),
                                    flagged_last=int((i32[3] != 0).sum()), attempts_mean_last=round(float(i32[2].float().mean()) + 1, 2))
    gen, t = RacingTrackGenerator(), []
    for k in range(HOST_TRACKS):
        np.random.seed(k)
        t0 = time.perf_counter()
        gen.generate()
        t.append(time.perf_counter() - t0)
    out["host_class_s_per_track"] = series(t)
    return out


def _manager(E):
    from tactics2d_amd import layout as L
    from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_model
    from tactics2d_amd.traffic import BatchedScenarioManager
    length, width = VEHICLE_TEMPLATE["medium_car"][:2]
    m = BatchedScenarioManager(E, 1, 100000, 100)
    ego = vehicle_model("medium_car", "kinematics", steer_range=(-0.5, 0.5), accel_range=(-4.0, 2.0))
    m.configure(ego.param_row(L.SHAPE_OBB, length, width)[None], check_dynamic=False, check_off_lane=False, check_arrival=0,
                check_no_action=1, no_action_max_step=100, shaped_reward=0)
    return m


def case_install():
    import numpy as np
    E = 4096
    m = _manager(E)
    m.status_checklist["out_bound"].reset(np.zeros((E, 4), np.float32))
    z = np.zeros(E)
    m.reset(z, z, z, z, np.zeros(E, np.uint8))
    dev_s = []
    for k in range(WARM + REPS):
        t0 = time.perf_counter()
        m.pool.set_tracks_generated(E, k)
        dev_s.append(time.perf_counter() - t0)
    gen = m.pool.generated_tracks()
    host_s = []
    for k in range(3):
        t0 = time.perf_counter()
        m.status_checklist["out_bound"].reset(np.float32(gen["boundary"]))
        pose = gen["start_pose"]
        m.reset(pose[:, 0], pose[:, 1], pose[:, 2], z, np.zeros(E, np.uint8))
        m.pool.set_tracks(gen["tiles"], np.arange(E, dtype=np.int32), 0, "forward", 8)
        m.pool.sync()
        host_s.append(time.perf_counter() - t0)
    m.close()
    return dict(install_4096=dict(device_s=series(dev_s[WARM:]), host_path_upload_only_s=series(host_s),
                                  tiles_total=int(gen["n_tile"].sum())))


def case_regenerate():
    import numpy as np
    import torch
    from tactics2d_amd.envs import VecRacingEnv
    from tactics2d_amd.pool import _DevArray
    E, INNER = 4096, 50
    out = {}
    act = torch.zeros((E, 2), device="cuda:0")
    act[:, 1] = 1.0
    for name, per_episode in (("step_auto_reset", False), ("step_auto_reset_regenerate_nobody", True)):
        env = VecRacingEnv(E, auto_reset=True, track_source="device", new_track_per_episode=per_episode)
        env.reset()
        for _ in range(60):
            env.step_torch(act)
        torch.cuda.synchronize()
        ms = [event_ms(lambda: [env.step_torch(act) for _ in range(INNER)]) / INNER for _ in range(REPS)]
        out[name] = dict(us_per_step=series([1e3 * v for v in ms]))
        if per_episode:
            pool = env.scenario_manager.pool
            status = torch.as_tensor(_DevArray(pool.track_buffers()["status"], (E, 4), "|u1", pool), device="cuda:0")
            done = torch.zeros((E, 4), dtype=torch.uint8, device="cuda:0")
            done[:, 0] = 1; done[:, 1] = 1
            done[torch.arange(0, E, 100, device="cuda:0"), 3] = 1       # 1 % of the envs, spread over the workgroups
            keep = status.clone()
            ms = []
            for _ in range(WARM + REPS):
                status.copy_(done)
                ms.append(event_ms(lambda: pool.regenerate_tracks(torch.cuda.current_stream().cuda_stream)))
            status.copy_(keep)
            pool.sync()
            out["regenerate_launch_1_percent"] = dict(ms=series(ms[WARM:]), envs=int(done[:, 3].sum()))
            status.copy_(keep)
            ms = [event_ms(lambda: pool.regenerate_tracks(torch.cuda.current_stream().cuda_stream)) for _ in range(WARM + REPS)]
            out["regenerate_launch_nobody"] = dict(us=series([1e3 * v for v in ms[WARM:]]))
        env.close()
    return out


CASES = {"generate": case_generate, "install": case_install, "regenerate": case_regenerate}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--case", choices=sorted(CASES))
    a = ap.parse_args()
    if a.case:
        print(json.dumps(CASES[a.case]()))
        return 0
    res = {}
    for case in ("generate", "install", "regenerate"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--case", case], capture_output=True, text=True, timeout=LIMITS[case])
        except subprocess.TimeoutExpired:
            res[case] = dict(error=f"ran longer than {LIMITS[case]} s")
            break
        if r.returncode != 0:
            res[case] = dict(error=f"exit status {r.returncode}", stderr=r.stderr[-2000:])
            break
        res.update(json.loads(r.stdout.strip().splitlines()[-1]))
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if not any("error" in v for v in res.values() if isinstance(v, dict)) else 1


if __name__ == "__main__":
    sys.exit(main())
