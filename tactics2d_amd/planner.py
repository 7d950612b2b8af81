"""The parking tutorial's Reeds-Shepp planner for every env of a pool (docs/tutorial/train_parking_demo.ipynb cell 9).

RSPlanner.plan() is RSPlanner.get_rs_path of the notebook for the ego of every env in one launch of t2d_rs_plan
(include/t2d.h): candidates from the ego's rear axle to the target pose, obstacle edges from the lidar scan, the first
candidate in ascending (length, slot) whose swept box crosses no edge.  RSFollower.follow() is the notebook's RSAgent (cells 14
and 17) for the ego of every env in one launch of t2d_rs_follow: it adopts a found plan, and while a path is being executed it
replaces the env's action row by the PID follower's.  There is no CPU path.
"""
import numpy as np

from . import layout as L
from .controller import _ActionWriter
from .participant import MAX_STEER, VEHICLE_TEMPLATE

STATUS_NAMES = ("no_target", "far", "found", "none_free", "unchecked")   # layout.RS_NO_TARGET ...


def rs_params(vehicle="medium_car", steer_ratio=0.98, lidar_range=20.0, steer_hi=MAX_STEER, distance_tolerance=0.05,
              sample_step=0.1, length_ratio=2.0, edge_tolerance=1e-4):
    """The configuration RSPlanner.__init__ (cell 9 :7-21) derives from `scenario_manager.agent`: radius = wheel_base /
    tan(steer_ratio * steer_hi), center_shift = length / 2 - rear_overhang, threshold_distance = lidar_range - 5.  `vehicle`: a
    template name or (length, width, wheel_base, rear_overhang)."""
    if isinstance(vehicle, str):
        t = VEHICLE_TEMPLATE[vehicle]
        length, width, wheel_base, rear_overhang = t[0], t[1], t[3], t[5]
    else:
        length, width, wheel_base, rear_overhang = (float(v) for v in vehicle)
    return dict(radius=wheel_base / np.tan(steer_hi * steer_ratio), center_shift=0.5 * length - rear_overhang,
                half_length=0.5 * length, half_width=0.5 * width, distance_tolerance=distance_tolerance,
                threshold_distance=lidar_range - 5.0, sample_step=sample_step, length_ratio=length_ratio,
                edge_tolerance=edge_tolerance)


class RSPlanner:
    """pool: a ParticipantPool with target areas, target headings and a configured lidar (lidar_config with max_range =
    lidar_range).  plan() returns zero-copy torch views of the plan records (ParticipantPool.rs_plan_views)."""

    def __init__(self, pool, vehicle="medium_car", steer_ratio=0.98, lidar_range=20.0, steer_hi=MAX_STEER, vehicle_base=None,
                 **overrides):
        self.pool = pool
        self.params = rs_params(vehicle, steer_ratio, lidar_range, steer_hi)
        unknown = set(overrides) - set(self.params)
        if unknown:
            raise TypeError(f"unknown planner options {sorted(unknown)}")
        self.params.update(overrides)
        self.vehicle_base = vehicle_base
        self._out = self._views = None
        self.configure()

    def configure(self):
        """(again) after the pool's lidar was reconfigured"""
        self.pool.rs_config(vehicle_base=self.vehicle_base, **self.params)

    def plan(self, lidar=None, stream=None):
        """lidar: float32 CUDA tensor [n_env, n_beams] (None: the pool's own scan buffer, i.e. the last lidar_scan()); stream: a
        torch stream (None: the current one).  Asynchronous: enqueued behind a step and a scan on the same stream it plans from
        that step.  Returns dict(status, slot, n_seg, n_visited, steer, distance, length, shortest), valid until the next plan()."""
        import torch
        pool = self.pool
        dev = torch.device("cuda", pool.device_id)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        if lidar is not None:
            if lidar.dtype != torch.float32 or tuple(lidar.shape) != (pool.n_env, pool.n_beams) or not lidar.is_contiguous():
                raise ValueError(f"lidar must be a contiguous float32 [{pool.n_env}, {pool.n_beams}] tensor")
        if self._out is None:
            self._out = torch.zeros((pool.n_env, L.RS_RECORD_BYTES // 8), dtype=torch.float64, device=dev)
            self._views = pool.rs_plan_views(self._out.data_ptr(), owner=self._out)
        pool.rs_plan(None if lidar is None else lidar.data_ptr(), self._out.data_ptr(), st.cuda_stream)
        return self._views

    def write_routes(self, route=0, step_size=0.01, plan=None, stream=None):
        """The current plans as routes (ParticipantPool.curve_routes): the path of every FOUND env, sampled as
        ReedsSheppPath.get_curve_line samples it (reeds_shepp.py:46-139; step_size: its default) from the ego's rear-axle pose,
        goes into route `route` of that env's own route set; every other env gives a word of 0 segments, so its route stays.
        The words are made of the plan records on the device -- steer is the letter, distance / radius the segment --, the start
        of the state views; nothing crosses to the host.  plan: the dict plan() returned (None: its last one).  Needs
        pool.set_routes with one set per env, whose route `route` has the capacity in vertices.  Returns the int32 CUDA tensor
        [n_env] of the curves' point counts (0: no plan, more than the capacity: truncated).  Asynchronous on `stream`."""
        import torch
        from .interpolator import pack_words
        pool = self.pool
        plan = plan if plan is not None else self._views
        if plan is None:
            raise RuntimeError("write_routes needs a plan: call plan() first")
        dev = torch.device("cuda", pool.device_id)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
        with torch.cuda.stream(st):
            found = plan["status"] == L.RS_FOUND
            radius, shift = float(self.params["radius"]), float(self.params["center_shift"])
            ego = pool.status_config.ego_index if hasattr(pool, "status_config") else 0
            cols = [torch.as_tensor(pool.device_array(f), device=dev).view(pool.n_env, pool.max_agents)[:, ego].double()
                    for f in (L.F_X, L.F_Y, L.F_HEADING)]
            starts = torch.stack([cols[0] - shift * torch.cos(cols[2]), cols[1] - shift * torch.sin(cols[2]), cols[2]], 1).contiguous()
            words = pack_words(plan["distance"] / radius, plan["steer"], plan["n_seg"].masked_fill(~found, 0))
            return pool.curve_routes(words, starts, radius, step_size, L.CURVE_RS, route, stream=st.cuda_stream)


FOLLOW_EVENTS = ("adopted", "pop_reached", "pop_rising", "finished", "reset", "dropped")   # bit k: layout.RS_FOLLOW_*


def rs_follow_params(planner_params, steer_ratio=0.98, max_speed=0.5, max_acceleration=2.0, steer_bound=0.524, accel_bound=2.0):
    """The configuration of the notebook's RSAgent (cell 17 and cell 20: execute_radius = the planner's radius, dr = its
    center_shift), its three PIDController gains, its thresholds, and the action box of the wrapper (cell 7)."""
    return dict(radius=planner_params["radius"], dr=planner_params["center_shift"], steer_ratio=steer_ratio, max_speed=max_speed,
                max_acceleration=max_acceleration, kp_v=0.8, ki_v=0.0, kd_v=0.0, kp_a=2.0, ki_a=0.0, kd_a=0.0, kp_s=5.0, ki_s=0.0,
                kd_s=0.0, yaw_weight=0.5, reach_radius=0.02, rising_radius=0.1, steer_bound=steer_bound, accel_bound=accel_bound)


class RSFollower(_ActionWriter):
    """pool: the ParticipantPool of `planner` (an RSPlanner, whose radius and center_shift it takes).  follow() returns zero-copy
    torch views of the follower's records (ParticipantPool.rs_follow_views) beside the action rows it wrote."""

    _record_bytes, _records, _n_rows = L.RS_FOLLOW_RECORD_BYTES, "rs_follow_views", "n_env"

    def __init__(self, pool, planner, **overrides):
        super().__init__(pool)
        self.planner = planner
        self.params = rs_follow_params(planner.params)
        unknown = set(overrides) - set(self.params)
        if unknown:
            raise TypeError(f"unknown follower options {sorted(unknown)}")
        self.params.update(overrides)
        pool.rs_follow_config(**self.params)

    def follow(self, actions, plan=None, out=None, stream=None):
        """actions: float32 CUDA tensor [n_env, 2] (steering, accel), the policy's rows (None: zeros), never written unless it is
        also `out`; plan: the dict RSPlanner.plan() returned (None: its last one, or the pool's own records if it never planned);
        out: float32 [n_env, 2] tensor for the rows to step (None: a buffer of the follower's own).  Asynchronous on `stream`.
        Returns dict(action_rows, executing, segment, events, steps, action, distance_to_go, total_error), valid until the
        next follow()."""
        if plan is not None:
            plan_ptr = plan["status"].data_ptr()   # (the record's first word)
        else:
            plan_ptr = self.planner._out.data_ptr() if self.planner._out is not None else None
        return self._write(lambda act_in, act_out, rec, st: self.pool.rs_follow(act_in, act_out, plan_ptr, rec, st), actions, out, stream)

    def reset(self, mask=None, stream=None):
        """agent.reset() for the envs where `mask` (a uint8 / bool CUDA tensor [n_env]) is non-zero; None: every env"""
        self._reset(self.pool.rs_follow_reset, mask, stream)
