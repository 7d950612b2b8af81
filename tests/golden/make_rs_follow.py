#!/usr/bin/env python3
"""Golden data for the Reeds-Shepp path follower -> rs_follow.npz, made by EXECUTING the parking tutorial's own definitions.

TEST INFRASTRUCTURE (generation time only; nothing of the reference's text is kept: the file holds numbers).  From a reference
tree this script parses docs/tutorial/train_parking_demo.ipynb and executes, taken from the parsed cells, the definitions
PIDController, rear_center_coord and RSAgent and the body of ParkingWrapper._preprocess_action (pure numpy); loads
tactics2d/interpolator/reeds_shepp.py from its file as make_rs.py does; and imports the reference's SingleTrackKinematics.

The file holds SEQUENCES of follower calls.  Sequence q is the calls off[q] .. off[q + 1] - 1; per call
  state f32 [M, 4]   x, y, heading, speed of the ego as the call sees them (fp32: what a pool holds)
  ended u8 [M]       the episode ended in the step before (the notebook's loop then calls agent.reset())
  plan i32 [M]       row of the plan table whose record reads FOUND in this call, -1: no plan
  action f64 [M, 2]  RSAgent.get_action's return (NaN: the agent did not act, the policy's action goes through)
  row f32 [M, 2]     _preprocess_action(action) for ParkingEnv's Box(+-0.524, +-2.0) (NaN likewise)
  head i32 [M]       index of the head segment within the adopted plan after the call, -1 without a path
  left i32 [M]       segments left after the call
  events u8 [M]      1 adopted, 2 popped by the reach rule, 4 popped by the rising rule, 8 finished, 16 reset
and per sequence gains i32 [Q] (row of gain_table f64 [2, 9]: Kp, Ki, Kd of the velocity, acceleration and steer controller),
the plan table plan_steer i32 [P, 5], plan_distance f64 [P, 5] (as RSAgent.calculate_target_points computes them),
plan_n i32 [P], and for the closed loops end_pose f64 [24, 3]: the path's end, a rear-axle pose.
  (a) sequences 0 .. 23: closed loops of the reference alone.  medium_car, start pose in +-5 m, goal within +-5 m of the rear
      axle, path = get_path.  (No closed loop runs a five-segment slot: slots 44-47 of the reference's get_all_path were a path
      for none of 20 000 random goals within 15 m, as for none of make_rs.py's; part (b) drives five segments.)  Each step get_action -> wrapper ->
      SingleTrackKinematics.step(..., 100); x, y, heading, speed are rounded to fp32 before they go back into agent and model.
      Candidates are taken in the order of the seeded stream; one that does not finish within 1000 steps or has a decision
      margin below 1e-6 is passed over.
  (b) sequences 24 ..: states from a crude integrator of this script's own with prescribed disturbances, three of each:
      a pop by the rising rule; a first segment shorter than 0.02 m; an agent.reset() in the middle of a path (with and without a
      new plan in the same call); a second path adopted after the first finished, with non-zero Ki and Kd (gains row 1).
Every call is also run through tests/rs_follow_ref.py in lockstep: the script fails unless the restatement agrees (1e-12, decisions
exactly), every pop rule and every (letter, sign) pair occurs, and no call has a decision margin below 1e-7.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_rs_follow.py --ref REFERENCE_TREE [--out DIR]
"""
import argparse
import ast
import json
import math
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
from make_rs import load_reference, write_npz   # noqa: E402
import rs_follow_ref as F                       # noqa: E402

SEED = 20261018
LENGTH, WHEEL_BASE, FRONT_OVERHANG, REAR_OVERHANG = 4.284, 2.637, 0.880, 0.767   # medium_car
STEER_HI = 0.524
GAINS = np.array([[0.8, 0.0, 0.0, 2.0, 0.0, 0.0, 5.0, 0.0, 0.0], [0.8, 0.01, 0.1, 2.0, 0.02, 0.2, 5.0, 0.05, 0.5]])
LETTER = {"L": 1, "R": -1, "S": 0}
CAP = 1000
N_LOOPS = 24


def notebook_definitions(ref):
    """the follower's definitions, executed from the parsed cells"""
    nb = json.load(open(os.path.join(ref, "docs", "tutorial", "train_parking_demo.ipynb")))
    want, body, wrapper = {"PIDController", "rear_center_coord", "RSAgent"}, [], None
    for cell in nb["cells"]:
        if cell["cell_type"] != "code":
            continue
        src = "".join(ln for ln in "".join(cell["source"]).splitlines(True) if not ln.lstrip().startswith(("%", "!")))
        try:
            tree = ast.parse(src)
        except SyntaxError:
            continue
        for node in tree.body:
            if isinstance(node, (ast.ClassDef, ast.FunctionDef)) and node.name in want:
                body.append(node)
                want.discard(node.name)
            if isinstance(node, ast.ClassDef) and node.name == "ParkingWrapper":
                wrapper = next(n for n in node.body if isinstance(n, ast.FunctionDef) and n.name == "_preprocess_action")
    assert not want and wrapper is not None, (want, wrapper)
    body.append(wrapper)
    ns = {"np": np, "STEER_RATIO": 0.98}
    exec(compile(ast.Module(body=body, type_ignores=[]), "<tutorial>", "exec"), ns)
    box = types.SimpleNamespace(high=np.array([STEER_HI, 2.0], np.float32), low=np.array([-STEER_HI, -2.0], np.float32))
    owner = types.SimpleNamespace(env=types.SimpleNamespace(action_space=box))
    ns["wrap"] = lambda action: ns["_preprocess_action"](owner, action)
    return ns


class Recorder:
    """one sequence: the notebook's agent and the restatement side by side"""

    def __init__(self, ns, gains, radius, dr, plans):
        self.ns, self.plans = ns, plans
        self.agent = ns["RSAgent"](None, radius, dr)
        g = GAINS[gains]
        for c, k in ((self.agent.velocity_controller, 0), (self.agent.accelerate_controller, 3), (self.agent.steer_controller, 6)):
            c.Kp, c.Ki, c.Kd = g[k:k + 3]
        self.ref = F.Follower(F.Params(radius, dr, kp_v=g[0], ki_v=g[1], kd_v=g[2], kp_a=g[3], ki_a=g[4], kd_a=g[5], kp_s=g[6],
                                       ki_s=g[7], kd_s=g[8]))
        self.rows = []
        self.margin = math.inf
        self.n_adopted = 0

    def add_plan(self, path):
        """a plan table row from an object with actions / signs / segments; its distances are read off the agent"""
        probe = self.ns["RSAgent"](None, self.agent.execute_radius, self.agent.dr)
        probe.calculate_target_points(path, [0.0, 0.0, 0.0])
        seg = probe.path_info["segments"]
        self.plans.append(([s for s, _ in seg], [float(d) for _, d in seg], path))
        return len(self.plans) - 1

    def call(self, state, ended=False, plan=-1):
        agent, st = self.agent, types.SimpleNamespace(x=float(state[0]), y=float(state[1]), heading=float(state[2]), speed=float(state[3]))
        events = 0
        if ended:
            agent.reset()
            events |= F.EV_RESET
        n_total = getattr(self, "_n_total", 0)
        action = None
        if not agent.executing_rs and plan >= 0:
            agent.calculate_target_points(self.plans[plan][2], [st.x, st.y, st.heading])
            assert [list(s) for s in agent.path_info["segments"]] == [list(s) for s in zip(*self.plans[plan][:2])]
            n_total = self._n_total = len(agent.path_info["segments"])
            events |= F.EV_ADOPTED
            self.n_adopted += 1
        if agent.executing_rs:
            before = len(agent.path_info["segments"])
            tx, ty = agent.path_info["target_points"][0][:2]
            rx, ry, _ = self.ns["rear_center_coord"](st.x, st.y, st.heading, agent.dr)
            d = np.sqrt((rx - tx) ** 2 + (ry - ty) ** 2)
            action = agent.get_action(st)
            left = len(agent.path_info["segments"])
            if left < before:
                events |= F.EV_POP_REACHED if d < 0.02 else F.EV_POP_RISING
            if left == 0:
                events |= F.EV_FINISHED
        left = len(agent.path_info["segments"])
        head = n_total - left if left else -1
        act = np.full(2, np.nan) if action is None else np.asarray(action, np.float64)
        row = np.full(2, np.nan, np.float32) if action is None else self.ns["wrap"](action)
        assert row.dtype == np.float32
        p = self.plans[plan] if plan >= 0 else None
        r = self.ref.call(state, ended, True, None if p is None else (p[0], p[1]))
        assert (r.executing, r.segment, r.events) == (left, head, events), (len(self.rows), r, left, head, events)
        if action is None:
            assert np.isnan(r.action[0])
        else:
            assert np.abs(np.array(r.action) - act).max() <= 1e-12 and r.row.tobytes() == row.tobytes(), (r, act, row)
        self.margin = min(self.margin, r.margin)
        self.rows.append((np.float32(state), int(ended), int(plan), act, row, head, left, events))
        return action, row


def crude_step(state, row, lf, lr):
    """this script's own integrator for part (b): one 100 ms Euler step of a bicycle about its centre"""
    x, y, h, v = (float(s) for s in state)
    steer, accel = float(row[0]), float(row[1])
    v = min(max(v + accel * 0.1, -0.5), 0.5)
    beta = math.atan(lr / (lf + lr) * math.tan(steer))
    return np.float32([x + v * math.cos(h + beta) * 0.1, y + v * math.sin(h + beta) * 0.1, h + v / lr * math.sin(beta) * 0.1, v])


def fake_path(radius, steer, distance):
    letter = {1: "L", -1: "R", 0: "S"}
    return types.SimpleNamespace(actions=[letter[s] for s in steer], signs=np.sign(distance).astype(int),
                                 segments=np.abs(np.asarray(distance, float)) / radius)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ref", required=True)
    ap.add_argument("--out", default=HERE)
    a = ap.parse_args()
    sys.dont_write_bytecode = True
    ns = notebook_definitions(a.ref)
    rs_mod = load_reference(a.ref)
    sys.path.insert(0, a.ref)
    from tactics2d.participant.trajectory import State
    from tactics2d.physics import SingleTrackKinematics
    lf, lr = LENGTH / 2 - FRONT_OVERHANG, LENGTH / 2 - REAR_OVERHANG
    model = SingleTrackKinematics(lf=lf, lr=lr, steer_range=(-STEER_HI, STEER_HI), speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0),
                                  interval=100)
    radius = WHEEL_BASE / np.tan(STEER_HI * 0.98)
    dr = 0.5 * LENGTH - REAR_OVERHANG
    rs = rs_mod.ReedsShepp(radius)
    rng = np.random.default_rng(SEED)
    plans, seqs, gains, end_pose = [], [], [], []

    # ---- (a) closed loops ------------------------------------------------------------------------------------------------
    def closed_loop(five):
        start = np.float32(np.concatenate([rng.uniform(-5, 5, 2), rng.uniform(-np.pi, np.pi, 1), [0.0]]))
        rear = np.array([start[0] - dr * np.cos(float(start[2])), start[1] - dr * np.sin(float(start[2]))], float)
        span = 15 if five else 5   # (no five-segment slot is a path for a goal within 5 m at this radius)
        goal = np.concatenate([rear + rng.uniform(-span, span, 2), rng.uniform(-np.pi, np.pi, 1)])
        if five:
            cands = [p for p in rs.get_all_path(rear, float(start[2]), goal[:2], goal[2])[44:48] if p is not None]
            if not cands:
                return None
            path = min(cands, key=lambda p: p.length)
        else:
            path = rs.get_path(rear, float(start[2]), goal[:2], goal[2])
        rec = Recorder(ns, 0, radius, dr, list(plans))
        k = rec.add_plan(path)
        state = start
        for step in range(CAP):
            action, row = rec.call(state, False, k if step == 0 else -1)
            if not rec.agent.executing_rs:
                break
            s, _, _ = model.step(State(0, x=float(state[0]), y=float(state[1]), heading=float(state[2]), speed=float(state[3])),
                                 float(row[1]), float(row[0]), 100)
            state = np.float32([s.x, s.y, s.heading, s.speed])
        else:
            return None
        if rec.margin < 1e-6:
            return None
        return rec, goal

    passed_over = 0
    for five in [False] * N_LOOPS:
        for _ in range(20000):
            got = closed_loop(five)
            if got is not None:
                break
            passed_over += 1
        else:
            raise SystemExit("no candidate episode in 20000 draws")
        rec, goal = got
        plans.append(rec.plans[-1])
        seqs.append(rec)
        gains.append(0)
        end_pose.append(goal)

    # ---- (b) synthetic sequences -------------------------------------------------------------------------------------------
    def synthetic(kind, variant):
        g = 1 if kind == "second" else 0
        rec = Recorder(ns, g, radius, dr, list(plans))
        start = np.float32([1.5 - variant, -2.0 + 1.5 * variant, 0.7 * variant - 0.4, 0.0])
        state = start
        drive = lambda row: crude_step(state, row if np.isfinite(row).all() else np.float32([0.1, -0.3]), lf, lr)   # (no path: a policy's row)
        if kind == "rising":
            steer, dist = [(0, 1), (1, 0), (-1, 0)][variant], [(0.6, 1.0), (-0.5, 0.8), (0.55, -0.9)][variant]
            k = rec.add_plan(fake_path(radius, steer, dist))
            n0, rising = len(steer), lambda: any(r[7] & F.EV_POP_RISING for r in rec.rows)

            def to_go(st):
                tx, ty = rec.agent.path_info["target_points"][0][:2]
                rx, ry, _ = ns["rear_center_coord"](float(st[0]), float(st[1]), float(st[2]), dr)
                return rx - tx, ry - ty
            after = 0
            for step in range(300):
                _, row = rec.call(state, False, k if step == 0 else -1)
                after += rising()
                if after > 40:
                    break
                nxt = drive(row)
                if not rising() and rec.rows[-1][6] == n0 and math.hypot(*to_go(nxt)) < 0.07:
                    state = nxt
                    _, row = rec.call(state, False, -1)      # d still falls ...
                    ux, uy = to_go(nxt)                      # ... the disturbance: 12 mm away from the target, d rises below 0.1
                    n = math.hypot(ux, uy)
                    nxt = np.float32([nxt[0] + 0.012 * ux / n, nxt[1] + 0.012 * uy / n, nxt[2], nxt[3]])
                state = nxt
            popped = rising()
            assert popped, (kind, variant)
        elif kind == "short":
            steer, dist = [(0, 1, 0), (1, 0), (-1, 0, 1)][variant], [(0.01, 0.5, 0.4), (0.015, -0.5), (-0.012, -0.4, 0.3)][variant]
            k = rec.add_plan(fake_path(radius, steer, dist))
            for step in range(25):
                _, row = rec.call(state, False, k if step == 0 else -1)
                state = drive(row)
            assert rec.rows[0][7] == F.EV_ADOPTED | F.EV_POP_REACHED, rec.rows[0]
        elif kind == "five":
            sg = (1, -1, 1)[variant]
            k = rec.add_plan(fake_path(radius, (sg, -sg, 0, sg, -sg), [(0.5, -0.4, 0.6, -0.3, 0.4), (-0.5, 0.4, -0.6, 0.3, -0.4),
                                                                      (0.3, 0.4, 0.5, -0.4, -0.3)][variant]))
            for step in range(CAP):
                _, row = rec.call(state, False, k if step == 0 else -1)
                if not rec.agent.executing_rs:
                    break
                state = drive(row)
            assert rec.rows[-1][7] & F.EV_FINISHED and max(r[5] for r in rec.rows) == 4, (kind, variant)
        elif kind == "reset":
            k1 = rec.add_plan(fake_path(radius, (1, 0, -1), (0.7, 0.5, 0.6)))
            k2 = rec.add_plan(fake_path(radius, (-1, 0), (-0.6, -0.7)))
            for step in range(45):
                ended = step == 12 + variant
                plan = k1 if step == 0 else k2 if (ended and variant != 1) or (variant == 1 and step == 20) else -1
                _, row = rec.call(state, ended, plan)
                state = drive(row if np.isfinite(row).all() else np.float32([0.1, -0.3]))
            ev = [r[7] for r in rec.rows]
            assert any(e & F.EV_RESET for e in ev) and rec.n_adopted == 2
        else:
            k1 = rec.add_plan(fake_path(radius, [(0,), (1,), (-1,)][variant], [(0.3,), (-0.3,), (0.35,)][variant]))
            k2 = rec.add_plan(fake_path(radius, (0, 1), (-0.4, 0.5)))
            first_done = None
            for step in range(400):
                plan = k1 if step == 0 else k2 if first_done is not None and step == first_done + 2 else -1
                _, row = rec.call(state, False, plan)
                if first_done is None and rec.rows[-1][7] & F.EV_FINISHED:
                    first_done = step
                if first_done is not None and step > first_done + 30:
                    break
                state = drive(row if np.isfinite(row).all() else np.float32([0.0, 0.0]))
            assert first_done is not None and rec.n_adopted == 2, (kind, variant, first_done)
            assert rec.agent.steer_controller.integral != 0
        return rec

    for kind in ("rising", "short", "reset", "second", "five"):
        for variant in range(3):
            rec = synthetic(kind, variant)
            for k in range(len(plans), len(rec.plans)):
                plans.append(rec.plans[k])
            seqs.append(rec)
            gains.append(1 if kind == "second" else 0)

    # ---- the conditions on the file ------------------------------------------------------------------------------------------
    rows = [r for rec in seqs for r in rec.rows]
    events = np.array([r[7] for r in rows], np.uint8)
    n_a = sum(len(rec.rows) for rec in seqs[:N_LOOPS])
    pairs = set()
    for rec in seqs[:N_LOOPS]:
        s, d, _ = rec.plans[-1]
        pairs |= {(int(si), int(np.sign(di))) for si, di in zip(s, d)}
    margin = min(rec.margin for rec in seqs)
    counts = {n: int((events & b != 0).sum()) for n, b in (("adopted", 1), ("reach", 2), ("rising", 4), ("finished", 8), ("reset", 16))}
    print(f"(a): {n_a} calls in {N_LOOPS} closed loops, {passed_over} candidates passed over; segment counts "
          f"{sorted({len(rec.plans[-1][0]) for rec in seqs[:N_LOOPS]})}; (letter, sign) pairs {sorted(pairs)}")
    print(f"all: {len(rows)} calls in {len(seqs)} sequences, events {counts}, smallest decision margin {margin:.3e}")
    worst_d, worst_yaw = 0.0, 0.0
    for rec, goal in zip(seqs[:N_LOOPS], end_pose):
        x, y, h = (float(v) for v in rec.rows[-1][0][:3])
        worst_d = max(worst_d, math.hypot(x - dr * math.cos(h) - goal[0], y - dr * math.sin(h) - goal[1]))
        worst_yaw = max(worst_yaw, abs((h - goal[2] + np.pi) % (2 * np.pi) - np.pi))
    print(f"(a): final rear-axle error <= {worst_d:.4f} m, <= {worst_yaw:.4f} rad")
    assert pairs == {(s, g) for s in (1, 0, -1) for g in (1, -1)}, "change the seed"
    assert counts["reach"] >= 3 and counts["rising"] >= 3 and counts["reset"] >= 3, counts
    assert all(rec.rows[-1][7] & F.EV_FINISHED for rec in seqs[:N_LOOPS])
    assert margin >= 1e-7, "change the seed or the disturbances"

    P = len(plans)
    plan_steer, plan_distance = np.zeros((P, 5), np.int32), np.zeros((P, 5))
    for k, (s, d, _) in enumerate(plans):
        plan_steer[k, :len(s)], plan_distance[k, :len(d)] = s, d
    out = dict(off=np.cumsum([0] + [len(rec.rows) for rec in seqs]).astype(np.int32), gains=np.array(gains, np.int32), gain_table=GAINS,
               state=np.array([r[0] for r in rows], np.float32), ended=np.array([r[1] for r in rows], np.uint8),
               plan=np.array([r[2] for r in rows], np.int32), action=np.array([r[3] for r in rows]),
               row=np.array([r[4] for r in rows], np.float32), head=np.array([r[5] for r in rows], np.int32),
               left=np.array([r[6] for r in rows], np.int32), events=events, plan_steer=plan_steer, plan_distance=plan_distance,
               plan_n=np.array([len(s) for s, _, _ in plans], np.int32), end_pose=np.array(end_pose),
               radius=np.array(radius), dr=np.array(dr))
    path = os.path.join(a.out, "rs_follow.npz")
    write_npz(path, out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
