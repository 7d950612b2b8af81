"""The occupancy-grid launch (`t2d_occupancy_grid`): the product form beside the naive form and the store floor.

    python scripts/time_occupancy.py [--envs 4096] [--reps 5] [--out profiles/occupancy.json]

--envs generated parking scenes (`pool.parking_scenes`: up to 12 quads and the ego per env), the window centred on the window the lots
share (sensor.parking_window).  Cases: 64 x 64 cells of 0.75 m and 128 x 128 cells of 0.375 m (the same 48 m window); static rings
alone and with the participants (the ego listed: exclude_slot = -1); inflate 0 and 1 m; the product form and T2D_OCC_FORMAT_NAIVE
(every cell tests every listed element).  Both outputs are written (f64 weights + u8 mask).

Each row is the mean over --reps windows of INNER back-to-back launches between two device events (launch to launch, on one stream),
after a clock ramp of RAMP untimed launches of the same work.  store floor: the bytes a launch must write (envs x H x W x 9 B) at the
HBM peak bench.py's roofline uses (8000 GB/s); `floor_frac` = floor time / measured time.  Asserts nothing; records whether the naive
grid equals the product one.  One JSON object on stdout (and in --out).  Kernel durations under rocprofv3 and hardware counters are
not measured here."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np
import torch

from tactics2d_amd import sensor
from tactics2d_amd.participant import VEHICLE_TEMPLATE, vehicle_row
from tactics2d_amd.pool import ParticipantPool

INNER, RAMP = 20, 60
HBM_PEAK_GBS = 8000.0   # bench.py's roofline
WINDOW_M = 48.0


def timed(fn):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    E = args.envs
    size = VEHICLE_TEMPLATE["medium_car"][:2]
    pool = ParticipantPool(E, 1)
    pool.set_param_table(vehicle_row("medium_car")[None])
    pool.set_status_config(max_step=100)
    pool.parking_scenes(7, 0.5, size)
    n_quads = pool.get_parking_scenes().n_quads
    stream = torch.cuda.current_stream().cuda_stream
    cases, equal = {}, True
    for side in (64, 128):
        nbytes = E * side * side * 9
        floor_us = nbytes / (HBM_PEAK_GBS * 1e9) * 1e6
        for participants in (False, True):
            for inflate in (0.0, 1.0):
                masks = {}
                for naive in (False, True):
                    grid = sensor.OccupancyGrid(pool, side, side, WINDOW_M / side, None, inflate, participants, -1, naive=naive,
                                                vehicle_size=size)
                    fn = lambda: grid.render(stream)
                    for _ in range(RAMP):
                        fn()
                    torch.cuda.synchronize()
                    us = [timed(lambda: [fn() for _ in range(INNER)]) / INNER * 1e3 for _ in range(args.reps)]
                    mean = float(np.mean(us))
                    name = f"{side}x{side}_{'participants' if participants else 'static'}_inflate{inflate:g}_{'naive' if naive else 'product'}"
                    cases[name] = dict(us=[round(t, 2) for t in us], mean_us=round(mean, 2), min_us=round(min(us), 2), max_us=round(max(us), 2),
                                       store_bytes=nbytes, store_floor_us=round(floor_us, 2), floor_frac=round(floor_us / mean, 3),
                                       occupied_frac=round(float(grid.mask.float().mean()), 4))
                    masks[naive] = grid.mask.clone()
                equal = equal and bool(torch.equal(masks[False], masks[True]))
    pool.close()
    out = dict(script="scripts/time_occupancy.py", device=torch.cuda.get_device_name(0), envs=E, window_m=WINDOW_M,
               quads_per_env=dict(mean=round(float(n_quads.mean()), 2), max=int(n_quads.max())), inner_launches=INNER, ramp_launches=RAMP,
               reps=args.reps, hbm_peak_gbs=HBM_PEAK_GBS, cases=cases, naive_grid_equals_product=equal,
               product_speedup_over_naive={k[:-8]: round(cases[k[:-8] + "_naive"]["mean_us"] / v["mean_us"], 2)
                                           for k, v in cases.items() if k.endswith("_product")},
               not_measured=["rocprofv3 kernel durations", "hardware counters", "the launch behind a step inside VecParkingEnv"])
    text = json.dumps(out, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
