#!/usr/bin/env python3
"""Golden vectors for `verify_states` -> verify_states.npz, made by RUNNING the reference's own
`PhysicsModelBase.verify_states` (physics/physics_model_base.py:53-73) on its own `Trajectory` objects.

TEST INFRASTRUCTURE (generation time only).  Imports tactics2d.physics and tactics2d.participant.trajectory (numpy only) from
the read-only reference tree and the parameter-row helpers of oracle/gen_golden*.py; stores numbers only:

    rows      (12, 24) the twelve model rows of verify_state.npz (kinematics, dynamics, point mass newton / euler, drift;
                       with and without an accel range)
    type_id   (T,)     row of each trajectory
    kind      (T,)     KINDS below
    fps       (T,)     Trajectory.fps (NaN: None -- only for trajectories that are not of stable frequency)
    stable    (T,)     Trajectory.stable_freq after the last add_state
    offsets   (T + 1,) trajectory t's added states are entries offsets[t] .. offsets[t + 1] - 1
    stamp     (S,)     frame (ms) of each added state, in insertion order (a duplicated stamp overwrites)
    state     (S, 6)   x, y, heading, speed, vx, vy of each added state (fp32-rounded before the reference sees them)
    interval  (S,)     the interval the reference's verify_states passed for that stamp (0 for the first)
    valid     (T,)     model.verify_states(trajectory)
    margin    (T,)     smallest distance of any tested quantity to its threshold over all frames; trajectories closer than
                       1e-7 are dropped (libm vs deterministic trig may legitimately flip them)

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_verify_states.py [--ref /root/reference] [--out DIR]

The npz is written with fixed zip time stamps: the same inputs give the same bytes.
"""
import argparse
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ORACLE = os.path.join(HERE, "..", "..", "oracle")

# what a trajectory exercises
K_STABLE_INT, K_STABLE_FRAC, K_UNEVEN, K_DUP, K_SINGLE, K_STEPPED, K_JUMP, K_FLAG_OFF = range(8)
KINDS = ["stable fps 10 / 20 (integer interval)", "stable fps 30 / 7 (1000 / fps not an integer)", "uneven stamps",
         "duplicated stamps", "a single frame", "quirk: stepped by the model itself, checked against frame 0",
         "quirk: jumps between frames, each within one interval of frame 0", "even stamps, stable_freq=False given"]


def models(PointMass, SingleTrackDrift, SingleTrackDynamics, SingleTrackKinematics):
    """the twelve rows of verify_state.npz, in its order (oracle/gen_golden_verify.py)"""
    car = dict(lf=4.284 / 2 - 0.880, lr=4.284 / 2 - 0.767, mass=1620.0, mass_height=1.449 / 2)
    return [
        SingleTrackKinematics(lf=1.262, lr=1.375, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44),
                              accel_range=(-11.0, 3.121)),
        SingleTrackKinematics(lf=1.262, lr=1.375, steer_range=(-0.524, 0.524), speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0)),
        SingleTrackKinematics(lf=1.0, lr=1.2, steer_range=0.6, speed_range=(0.0, 20.0), accel_range=3.0),
        SingleTrackKinematics(lf=1.262, lr=1.375, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44)),
        SingleTrackDynamics(lf=1.262, lr=1.375, mass=1620.0, mass_height=0.726, steer_range=(-0.524, 0.524),
                            speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)),
        PointMass(speed_range=(0.0, 7.0), accel_range=(0.0, 1.5)),
        PointMass(speed_range=(0.0, 7.0), accel_range=(0.3, 2.0)),
        PointMass(speed_range=(0.0, 7.0)),
        PointMass(speed_range=(0.0, 7.0), accel_range=(0.0, 1.5), backend="euler"),
        PointMass(speed_range=(0.0, 7.0), backend="euler"),
        SingleTrackDrift(**car, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)),
        SingleTrackDrift(**car, steer_range=(-0.524, 0.524), speed_range=(-16.67, 69.44)),
    ]


f32 = lambda a: np.float32(a).astype(np.float64)


def is_pm(m):
    return not hasattr(m, "wheel_base")


def vehicle_reach(m, last, dt):
    wb = m.wheel_base
    beta = np.arctan(m.lr / wb * np.array(m.steer_range, float))
    hr = np.mod(last[2] + last[3] / wb * np.sin(beta) * dt, 2 * np.pi)
    sr = np.clip(last[3] + np.array(m.accel_range, float) * dt, *m.speed_range)
    xr = last[0] + sr * np.cos(last[2] + beta) * dt
    yr = last[1] + sr * np.sin(last[2] + beta) * dt
    return hr, sr, xr, yr


def margin(m, last, cand, interval):
    """distance of every compared quantity to its threshold, recomputed in fp64 (for filtering only)"""
    if interval == 0:
        return np.inf
    dt = interval / 1000
    if is_pm(m):
        if m.accel_range is None:
            return np.inf
        den = 2 / dt ** 2
        a = np.hypot((cand[0] - last[0] - last[4] * dt) * den, (cand[1] - last[1] - last[5] * dt) * den)
        return min(abs(a - m.accel_range[0]), abs(a - m.accel_range[1]))
    if None in (m.steer_range, m.speed_range, m.accel_range):
        return np.inf
    hr, sr, xr, yr = vehicle_reach(m, last, dt)
    return min(abs(hr[0] - hr[1]), abs(cand[2] - hr[0]), abs(cand[2] - hr[1]), abs(cand[3] - sr[0]), abs(cand[3] - sr[1]),
               abs(cand[0] - xr[0]), abs(cand[0] - xr[1]), abs(cand[1] - yr[0]), abs(cand[1] - yr[1]))


def first_state(rng, m):
    lx, ly = f32(rng.uniform(-200, 200, 2))
    lh = float(f32(rng.uniform(0, 2 * np.pi)))
    if is_pm(m):
        lvx, lvy = f32(rng.uniform(-4, 4, 2))
        return np.array([lx, ly, lh, f32(np.hypot(lvx, lvy)), lvx, lvy])
    lo, hi = m.speed_range
    lv = float(f32(rng.uniform(max(lo, -5), min(hi, 30))))
    return np.array([lx, ly, lh, lv, f32(lv * np.cos(lh)), f32(lv * np.sin(lh))])


def candidate(rng, m, last, interval, inside, frac=None):
    """a state one interval from `last`: inside its reach (fractions of each range) or, for inside=False, pushed out of it"""
    dt = interval / 1000
    u = (lambda: rng.uniform(0.1, 0.9)) if frac is None else (lambda: frac)
    if is_pm(m):
        lo, hi = (0.0, 2.5) if m.accel_range is None else m.accel_range
        a = lo + (hi - lo) * u() if inside else hi * rng.uniform(1.2, 3.0)
        th = rng.uniform(0, 2 * np.pi)
        x = last[0] + last[4] * dt + 0.5 * a * np.cos(th) * dt * dt
        y = last[1] + last[5] * dt + 0.5 * a * np.sin(th) * dt * dt
        vx, vy = last[4] + a * np.cos(th) * dt, last[5] + a * np.sin(th) * dt
        return f32([x, y, last[2], np.hypot(vx, vy), vx, vy])
    if None in (m.steer_range, m.speed_range, m.accel_range):
        hr, sr = np.array([last[2], last[2] + 0.1]), np.array([last[3] - 1, last[3] + 1])
        xr = last[0] + sr * np.cos(last[2]) * dt
        yr = last[1] + sr * np.sin(last[2]) * dt
    else:
        hr, sr, xr, yr = vehicle_reach(m, last, dt)
    span = lambda r: r[0] + (r[1] - r[0]) * u()
    hh = hr[1] if hr[0] <= hr[1] else hr[1] + 2 * np.pi
    h = np.mod(hr[0] + (hh - hr[0]) * u(), 2 * np.pi)
    v, x, y = span(sr), span(xr), span(yr)
    if not inside:   # one quantity out of its range
        which = rng.integers(0, 4)
        w = lambda r: max(abs(r[1] - r[0]), 1e-3) * rng.uniform(0.3, 2.0)
        if which == 0:
            x = max(xr) + w(xr)
        elif which == 1:
            y = min(yr) - w(yr)
        elif which == 2:
            v = max(sr) + w(sr)
        else:
            h = np.mod(hh + 0.3, 2 * np.pi)
    return f32([x, y, h, v, v * np.cos(h), v * np.sin(h)])


def stepped(m, st, rng, n, interval, State):
    """the model's own roll-out: n - 1 steps of `interval` from st with random in-range actions"""
    out = [st]
    s = State(frame=0, x=st[0], y=st[1], heading=st[2], speed=st[3], vx=st[4], vy=st[5])
    for k in range(1, n):
        if is_pm(m):
            s = m.step(s, (rng.uniform(-1, 1), rng.uniform(-1, 1)), interval)
        else:
            s, _, _ = m.step(s, rng.uniform(-1, 1), rng.uniform(-0.3, 0.3), interval)
        vx = s.vx if s.vx is not None else s.speed * np.cos(s.heading)
        vy = s.vy if s.vy is not None else s.speed * np.sin(s.heading)
        v = f32([s.x, s.y, s.heading, s.speed, vx, vy])
        out.append(v)
        s = State(frame=k * interval, x=v[0], y=v[1], heading=v[2], speed=v[3], vx=v[4], vy=v[5])
    return out


def make_case(rng, ms, State, kind):
    t = int(rng.integers(0, len(ms)))
    if kind == K_STEPPED:
        t = int(rng.choice([0, 1, 2, 4, 5, 6]))   # (the models whose step is the plain one: kinematics, dynamics, newton)
    m = ms[t]
    n = 1 if kind == K_SINGLE else int(min(40, 1 + rng.geometric(1 / 7))) if kind != K_STEPPED else int(rng.integers(3, 12))
    n = max(n, 2) if kind in (K_DUP, K_JUMP) else n
    fps, stable_given = None, True
    if kind in (K_STABLE_INT, K_STEPPED, K_JUMP, K_SINGLE, K_UNEVEN, K_DUP):   # (a two-frame "uneven" one stays stable)
        fps = int(rng.choice([10, 20]))
    elif kind == K_STABLE_FRAC:
        fps = int(rng.choice([30, 7]))
    elif kind == K_FLAG_OFF:
        fps, stable_given = int(rng.choice([10, 20, 30])), False
    step = {10: 100, 20: 50, 30: 33, 7: 143, None: 100}[fps]
    if kind == K_UNEVEN:
        stamps = list(np.cumsum([0] + [int(rng.choice([7, 33, 50, 100, 150, 250])) for _ in range(n - 1)]))
    else:
        stamps = [k * step for k in range(n)]
    if kind == K_DUP:
        k = int(rng.integers(0, n))
        stamps = stamps[:k + 1] + [stamps[k]] + stamps[k + 1:]   # (a repeat of the last stamp so far: overwritten, no KeyError)
    st0 = first_state(rng, m)
    if kind == K_STEPPED:
        states = stepped(m, st0, rng, n, step, State)
    else:
        want = rng.random() < 0.5
        bad = int(rng.integers(1, len(stamps))) if len(stamps) > 1 and not want else -1
        states = [st0]
        for j in range(1, len(stamps)):
            iv = 1000 / fps if kind not in (K_UNEVEN, K_DUP, K_FLAG_OFF) else stamps[j] - stamps[0]
            frac = (0.15 if j % 2 else 0.85) if kind == K_JUMP else None
            states.append(candidate(rng, m, st0, iv if iv else 100, j != bad, frac))
    tr = Trajectory(id_=0, fps=fps, stable_freq=stable_given)
    for f, v in zip(stamps, states):
        tr.add_state(State(frame=int(f), x=v[0], y=v[1], heading=v[2], speed=v[3], vx=v[4], vy=v[5]))
    ok = bool(m.verify_states(tr))
    seen = []   # the intervals the reference passes, frame by frame: the same call with a verify_state that records and accepts
    m.verify_state = lambda state, last, interval=None: seen.append(interval) or True
    try:
        m.verify_states(tr)
    finally:
        del m.verify_state
    hist = tr.history_states
    first = hist[tr.frames[0]]
    lastv = np.array([first.x, first.y, first.heading, first.speed, first.vx, first.vy], float)
    mg = np.inf
    for f, iv in zip(tr.frames[1:], seen):
        s = hist[f]
        mg = min(mg, margin(m, lastv, np.array([s.x, s.y, s.heading, s.speed]), iv))
    return dict(type_id=t, kind=kind, fps=np.nan if fps is None else fps, stable=bool(tr.stable_freq), stamps=stamps,
                states=states, interval=[0.0] + [float(v) for v in seen], valid=ok, margin=mg)


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
    ap.add_argument("--ref", default="/root/reference")
    ap.add_argument("--out", default=HERE)
    args = ap.parse_args(argv)
    sys.path.insert(0, args.ref)
    sys.path.insert(0, ORACLE)
    global Trajectory
    from tactics2d.participant.trajectory import State, Trajectory
    from tactics2d.physics import PointMass, SingleTrackDrift, SingleTrackDynamics, SingleTrackKinematics
    from gen_golden import row_from_model, KIN, DYN, PM
    from gen_golden_drift import DRIFT, drift_row
    from gen_golden_pm_euler import PM_EULER
    ms = models(PointMass, SingleTrackDrift, SingleTrackDynamics, SingleTrackKinematics)
    ids = [KIN, KIN, KIN, KIN, DYN, PM, PM, PM, PM_EULER, PM_EULER, DRIFT, DRIFT]
    rows = np.stack([drift_row(m) if mid == DRIFT else row_from_model(m, mid) for m, mid in zip(ms, ids)])
    rng = np.random.default_rng(2031)
    plan = [K_STABLE_INT] * 700 + [K_STABLE_FRAC] * 600 + [K_UNEVEN] * 450 + [K_DUP] * 250 + [K_SINGLE] * 60 + \
           [K_STEPPED] * 150 + [K_JUMP] * 100 + [K_FLAG_OFF] * 120
    cases = [c for c in (make_case(rng, ms, State, k) for k in plan) if c["margin"] >= 1e-7]
    off = np.cumsum([0] + [len(c["stamps"]) for c in cases])
    arrays = dict(rows=rows, type_id=np.array([c["type_id"] for c in cases], np.uint8),
                  kind=np.array([c["kind"] for c in cases], np.uint8), fps=np.array([c["fps"] for c in cases], np.float64),
                  stable=np.array([c["stable"] for c in cases], np.uint8), offsets=off.astype(np.int32),
                  stamp=np.concatenate([c["stamps"] for c in cases]).astype(np.int64),
                  state=np.concatenate([np.array(c["states"], np.float64) for c in cases]).astype(np.float32),
                  interval=np.concatenate([c["interval"] for c in cases]).astype(np.float64),
                  valid=np.array([c["valid"] for c in cases], np.uint8),
                  margin=np.array([c["margin"] for c in cases], np.float64))
    os.makedirs(args.out, exist_ok=True)
    path = os.path.join(args.out, "verify_states.npz")
    write_npz(path, arrays)
    v, k = arrays["valid"], arrays["kind"]
    print(f"{path}: {len(cases)} trajectories, {int(off[-1])} states, {int(v.sum())} valid;",
          {i: (int(v[k == i].sum()), int((k == i).sum())) for i in range(len(KINDS))})


if __name__ == "__main__":
    main()
