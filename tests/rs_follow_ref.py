"""The Reeds-Shepp path follower for ONE env, in plain Python floats: the specification of t2d_rs_follow (include/t2d.h,
DESIGN.md 4.15a).  What it restates is the parking tutorial's RSAgent with its three PID controllers
(docs/tutorial/train_parking_demo.ipynb cells 14 and 17) and the wrapper's action scaling (cell 7); the fixture
tests/golden/rs_follow.npz, made by executing those cells, pins it (tests/test_rs_follow.py).

    f = Follower(Params())
    r = f.call(state, ended, active, plan, policy_row)      # one t2d_rs_follow for this env

state = (x, y, heading, speed) as the pool holds them (fp32 values, widened); plan = None (no record with status FOUND) or
(steer[n], distance[n]); policy_row = the caller's float32 pair.  r is a Result; r.margin is the distance of this call's
decisions from their thresholds (margin()).
"""
import math
from collections import namedtuple

import numpy as np

EV_ADOPTED, EV_POP_REACHED, EV_POP_RISING, EV_FINISHED, EV_RESET, EV_DROPPED = 1, 2, 4, 8, 16, 32
MAX_SEGMENTS = 5

_FIELDS = ("radius", "dr", "steer_ratio", "max_speed", "max_acceleration", "kp_v", "ki_v", "kd_v", "kp_a", "ki_a", "kd_a",
           "kp_s", "ki_s", "kd_s", "yaw_weight", "reach_radius", "rising_radius", "steer_bound", "accel_bound")
_MEDIUM_CAR = (2.637 / math.tan(0.524 * 0.98), 0.5 * 4.284 - 0.767)   # the tutorial's radius and rear-axle shift


class Params(namedtuple("Params", _FIELDS)):
    """t2d_rs_follow_params, field for field, with the notebook's defaults for a medium_car in ParkingEnv"""


Params.__new__.__defaults__ = _MEDIUM_CAR + (0.98, 0.5, 2.0, 0.8, 0.0, 0.0, 2.0, 0.0, 0.0, 5.0, 0.0, 0.0, 0.5, 0.02, 0.1, 0.524, 2.0)

Result = namedtuple("Result", "executing segment events steps action row distance_to_go total_error margin")


def sign(v):
    return 1.0 if v > 0 else -1.0 if v < 0 else 0.0


def clip(v, lo, hi):
    """np.clip for a scalar: a NaN stays a NaN"""
    return lo if v < lo else hi if v > hi else v


class PID:
    def __init__(self, kp, ki, kd):
        self.kp, self.ki, self.kd = kp, ki, kd
        self.target = self.prev_error = self.integral = 0.0

    def update(self, value, target):
        """returns (output, the state after it): the caller commits the state only if the whole action is finite"""
        error = target - value
        integral = self.integral + error
        out = self.kp * error + self.ki * integral + self.kd * (error - self.prev_error)
        return out, (target, error, integral)

    def commit(self, state):
        self.target, self.prev_error, self.integral = state

    def reset(self):   # (the target stays: the notebook's reset() is called without one)
        self.prev_error = self.integral = 0.0


def wrap_action(action, steer_bound=0.524, accel_bound=2.0):
    """the wrapper's scaling in fp32, in its order: round, clip to [-1, 1], * (high - low) / 2 + (high + low) / 2"""
    a = np.clip(np.array(action, dtype=np.float32), np.float32(-1), np.float32(1))
    high = np.array([steer_bound, accel_bound], np.float32)
    low = -high
    return a * (high - low) / np.float32(2) + (high + low) / np.float32(2)


def target_points(p, pose, steer, distance):
    """the chain of segment end points from the ego pose: per segment (tx, ty, tyaw, cx, cy, sx, sy); cx = None on a line"""
    x, y, yaw = pose
    x, y = x - p.dr * math.cos(yaw), y - p.dr * math.sin(yaw)
    out, r = [], p.radius
    for s, d in zip(steer, distance):
        if s == 0:
            cx = cy = None
            tx, ty, tyaw = x + d * math.cos(yaw), y + d * math.sin(yaw), yaw
        elif s > 0:
            cx, cy = x - r * math.sin(yaw), y + r * math.cos(yaw)
            da = d / r
            tx, ty, tyaw = cx + r * math.sin(yaw + da), cy - r * math.cos(yaw + da), yaw + da
        else:
            cx, cy = x + r * math.sin(yaw), y - r * math.cos(yaw)
            da = d / r
            tx, ty, tyaw = cx + r * math.sin(-yaw + da), cy + r * math.cos(-yaw + da), yaw - da
        out.append((tx, ty, tyaw, cx, cy, x, y))
        x, y, yaw = tx, ty, tyaw
    return out


class Follower:
    def __init__(self, params=None):
        self.p = params or Params()
        p = self.p
        self.pid_v, self.pid_a, self.pid_s = PID(p.kp_v, p.ki_v, p.kd_v), PID(p.kp_a, p.ki_a, p.kd_a), PID(p.kp_s, p.ki_s, p.kd_s)
        self.drop()

    def drop(self):
        self.steer, self.distance, self.points = [], [], []
        self.head, self.steps, self.last = -1, 0, math.inf

    @property
    def left(self):
        return len(self.steer) - self.head if self.head >= 0 else 0

    def reset(self):
        self.drop()
        for c in (self.pid_v, self.pid_a, self.pid_s):
            c.reset()

    def call(self, state, ended=False, active=True, plan=None, policy_row=(0.0, 0.0)):
        p = self.p
        x, y, yaw, v = (float(s) for s in state)
        events, margin = 0, math.inf
        passed = lambda: Result(self.left, self.head if self.left else -1, events, self.steps, (math.nan, math.nan),
                                np.array(policy_row, np.float32), math.nan, math.nan, margin)
        if ended:
            self.reset()
            events |= EV_RESET
        if not active:
            return passed()
        if not all(math.isfinite(s) for s in (x, y, yaw, v)):
            self.drop()
            events |= EV_DROPPED
            return passed()
        if not self.left and plan is not None and 1 <= len(plan[0]) <= MAX_SEGMENTS:
            self.steer, self.distance = [int(s) for s in plan[0]], [float(d) for d in plan[1]]
            self.points = target_points(p, (x, y, yaw), self.steer, self.distance)
            self.head, self.steps = 0, 0
            events |= EV_ADOPTED
        if not self.left:
            return passed()
        self.steps += 1
        rx, ry = x - p.dr * math.cos(yaw), y - p.dr * math.sin(yaw)
        tx, ty = self.points[self.head][:2]
        d = math.sqrt((rx - tx) ** 2 + (ry - ty) ** 2)
        margin = min(abs(d - p.reach_radius), abs(d - p.rising_radius))
        if d < p.rising_radius:
            margin = min(margin, abs(d - self.last))
        if d < p.reach_radius or (self.last < d and d < p.rising_radius):
            events |= EV_POP_REACHED if d < p.reach_radius else EV_POP_RISING
            self.last = math.inf
            self.head += 1
        else:
            self.last = d
        if not self.left:
            steps = self.steps
            self.drop()
            events |= EV_FINISHED
            return Result(0, -1, events, steps, (0.0, 0.0), wrap_action((0.0, 0.0), p.steer_bound, p.accel_bound), d,
                          math.nan, margin)
        s, dist = self.steer[self.head], self.distance[self.head]
        tx, ty, tyaw, cx, cy, sx, sy = self.points[self.head]
        d = math.sqrt((rx - tx) ** 2 + (ry - ty) ** 2)
        out_v, st_v = self.pid_v.update(-d * sign(dist), 0.0)
        target_v = clip(out_v, -p.max_speed, p.max_speed)
        out_a, st_a = self.pid_a.update(v, target_v)
        target_a = clip(out_a, -p.max_acceleration, p.max_acceleration)
        if cx is not None:
            err = (math.sqrt((rx - cx) ** 2 + (ry - cy) ** 2) - p.radius) * sign(s)
            want_yaw = math.atan2(ry - cy, rx - cx) + math.pi / 2 * sign(s)
        else:
            line_yaw = math.atan2(ty - sy, tx - sx)
            along = math.cos(line_yaw - yaw)
            margin = min(margin, abs(along))
            err = (ty - sy) * rx - (tx - sx) * ry + tx * sy - ty * sx
            norm = math.sqrt((ty - sy) ** 2 + (tx - sx) ** 2)
            err = (err / norm if norm != 0.0 else math.nan) * (1.0 if along > 0 else -1.0)   # (0 / 0 in numpy: NaN)
            want_yaw = tyaw
        err_yaw = -(want_yaw - yaw)
        err_yaw = math.atan2(math.sin(err_yaw), math.cos(err_yaw))
        margin = min(margin, math.pi - abs(err_yaw))
        total = err + p.yaw_weight * err_yaw
        out_s, st_s = self.pid_s.update(-total, 0.0)
        action = (clip(s * p.steer_ratio + out_s, -1.0, 1.0), target_a / p.max_acceleration)
        if not all(math.isfinite(a) for a in action):
            self.drop()
            events |= EV_DROPPED
            return passed()
        self.pid_v.commit(st_v)
        self.pid_a.commit(st_a)
        self.pid_s.commit(st_s)
        return Result(self.left, self.head, events, self.steps, action, wrap_action(action, p.steer_bound, p.accel_bound), d, total,
                      margin)


def margin(result):
    """how far the call's decisions were from flipping: min of |d - reach|, |d - rising|, |d - last| (below rising),
    |cos(line yaw - heading)| on a line and pi - |error_yaw|; +inf for a call that decided nothing"""
    return result.margin
