#!/usr/bin/env python3
"""Golden answers for replayed participants -> replay.npz, made by RUNNING the reference's own `ParticipantBase.is_active` /
`ParticipantBase.get_state` (participant/element/participant_base.py:166-203) on its own `Trajectory` / `State` objects.

TEST INFRASTRUCTURE (generation time only).  Imports tactics2d.participant.trajectory (numpy only) from a reference tree and
loads participant/element/participant_base.py from its FILE (its package's __init__ needs shapely); the concrete participant
below only fills in the abstract members, none of which the two executed methods touch.  Stores numbers and names only:

    period    ()       grid period of every trajectory (ms); t0 = 0
    offsets   (T + 1,) trajectory t's states are entries offsets[t] .. offsets[t + 1] - 1 (none: an empty trajectory)
    stamp     (S,)     frame (ms) of each state, ascending inside a trajectory, every one on the grid, no gaps
    state     (S, 6)   x, y, heading, speed, vx, vy (fp32-rounded before the reference sees them)
    q_traj    (Q,)     trajectory a query asks
    q_frame   (Q,)     the frame it asks for
    q_kind    (Q,)     KINDS below
    q_active  (Q,)     is_active(frame): 1 / 0, or -1 where it raised
    q_active_exc (Q,)  the exception's type name ("" = none)
    q_state   (Q, 6)   get_state(frame) (NaN where it raised)
    q_state_exc (Q,)   the exception's type name ("" = none)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_replay.py --ref REFERENCE_TREE [--out DIR]

The npz is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import importlib.util
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PERIOD = 40   # highD / inD / rounD / exiD: 25 Hz

K_INSIDE, K_FIRST, K_LAST, K_BEFORE, K_AFTER, K_OFF_GRID, K_ONE_FRAME, K_EMPTY = range(8)
KINDS = ["a stamp inside the window", "the window's first stamp", "the window's last stamp", "before the window",
         "after the window", "inside the window, off the grid", "a one-frame trajectory (at, before, after, off its stamp)",
         "an empty trajectory"]


def write_npz(path, arrays):
    """np.savez_compressed with fixed time stamps (reproducible bytes)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            b = io.BytesIO()
            np.lib.format.write_array(b, np.ascontiguousarray(arrays[k]), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), b.getvalue(),
                        compress_type=zipfile.ZIP_DEFLATED)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True, help="root of a tactics2d source tree")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.ref)
    from tactics2d.participant.trajectory import State, Trajectory
    spec = importlib.util.spec_from_file_location(
        "t2d_ref_participant_base", os.path.join(args.ref, "tactics2d", "participant", "element", "participant_base.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Logged(mod.ParticipantBase):   # the abstract members only; is_active / get_state are the base class's
        geometry = None

        def bind_trajectory(self, trajectory=None):
            self.trajectory = trajectory

        def get_pose(self, frame=None):
            return None

        def get_trace(self, frame_range=None):
            return None

    rng = np.random.default_rng(4207)
    f32 = lambda a: np.float32(a).astype(np.float64)
    trajs, queries = [], []   # [(stamps, states)], [(traj, frame, kind)]

    def add_traj(first_slot, n):
        stamps = [(first_slot + k) * PERIOD for k in range(n)]
        x, y = f32(rng.uniform(-200, 200, 2))
        h, v = float(f32(rng.uniform(0, 2 * np.pi))), float(f32(rng.uniform(0, 30)))
        states = []
        for _ in stamps:
            states.append(f32([x, y, h, v, v * np.cos(h), v * np.sin(h)]))
            x, y = f32(x + v * np.cos(h) * PERIOD / 1000), f32(y + v * np.sin(h) * PERIOD / 1000)
            h = float(f32(np.mod(h + rng.uniform(-0.02, 0.02), 2 * np.pi)))
            v = float(f32(max(0.0, v + rng.uniform(-0.2, 0.2))))
        trajs.append((stamps, states))
        return len(trajs) - 1, stamps

    for _ in range(40):   # ordinary windows: late starts, every length from 3 slots up
        t, st = add_traj(int(rng.integers(0, 30)), int(rng.integers(3, 60)))
        queries += [(t, int(rng.choice(st[1:-1])), K_INSIDE), (t, st[0], K_FIRST), (t, st[-1], K_LAST),
                    (t, st[0] - PERIOD * int(rng.integers(1, 5)), K_BEFORE), (t, st[0] - 1, K_BEFORE),
                    (t, st[-1] + PERIOD * int(rng.integers(1, 5)), K_AFTER), (t, st[-1] + 1, K_AFTER),
                    (t, int(rng.choice(st[:-1])) + int(rng.integers(1, PERIOD)), K_OFF_GRID)]
    for _ in range(12):   # one-frame trajectories
        t, st = add_traj(int(rng.integers(0, 30)), 1)
        queries += [(t, st[0], K_ONE_FRAME), (t, st[0] - PERIOD, K_ONE_FRAME), (t, st[0] + PERIOD, K_ONE_FRAME),
                    (t, st[0] + int(rng.integers(1, PERIOD)), K_ONE_FRAME)]
    for _ in range(8):    # empty trajectories
        trajs.append(([], []))
        queries += [(len(trajs) - 1, int(f), K_EMPTY) for f in (0, PERIOD * int(rng.integers(1, 50)), 17)]

    parts = []
    for i, (stamps, states) in enumerate(trajs):
        tr = Trajectory(id_=i, fps=1000 / PERIOD)
        for f, s in zip(stamps, states):
            tr.add_state(State(frame=int(f), x=s[0], y=s[1], heading=s[2], speed=s[3], vx=s[4], vy=s[5]))
        parts.append(Logged(i, "car", trajectory=tr))

    q_active, q_active_exc, q_state, q_state_exc = [], [], [], []
    for t, frame, _ in queries:
        try:
            q_active.append(int(bool(parts[t].is_active(frame))))
            q_active_exc.append("")
        except Exception as e:
            q_active.append(-1)
            q_active_exc.append(type(e).__name__)
        try:
            s = parts[t].get_state(frame)
            q_state.append([s.x, s.y, s.heading, s.speed, s.vx, s.vy])
            q_state_exc.append("")
        except Exception as e:
            q_state.append([np.nan] * 6)
            q_state_exc.append(type(e).__name__)

    off = np.cumsum([0] + [len(st) for st, _ in trajs])
    arrays = dict(period=np.int32(PERIOD), offsets=off.astype(np.int32),
                  stamp=np.array([f for st, _ in trajs for f in st], np.int64),
                  state=np.array([s for _, ss in trajs for s in ss], np.float64).astype(np.float32),
                  q_traj=np.array([q[0] for q in queries], np.int32), q_frame=np.array([q[1] for q in queries], np.int64),
                  q_kind=np.array([q[2] for q in queries], np.uint8), q_active=np.array(q_active, np.int8),
                  q_active_exc=np.array(q_active_exc, "U16"), q_state=np.array(q_state, np.float64).astype(np.float32),
                  q_state_exc=np.array(q_state_exc, "U16"))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "replay.npz")
    write_npz(path, arrays)
    k = arrays["q_kind"]
    print(f"{path}: {len(trajs)} trajectories, {int(off[-1])} states, {len(queries)} queries;",
          {i: int((k == i).sum()) for i in range(len(KINDS))},
          "exceptions:", sorted(set(q_active_exc) | set(q_state_exc)))


if __name__ == "__main__":
    main()
