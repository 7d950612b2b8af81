"""The parking tutorial's Reeds-Shepp planner for every env of a pool (docs/tutorial/train_parking_demo.ipynb cell 9).

RSPlanner.plan() is RSPlanner.get_rs_path of the notebook for the ego of every env in one launch of t2d_rs_plan
(include/t2d.h): candidates from the ego's rear axle to the target pose, obstacle edges from the lidar scan, the first
candidate in ascending (length, slot) whose swept box crosses no edge.  Following the chosen path (the notebook's RSAgent) is
not part of it.  There is no CPU path.
"""
import numpy as np

from . import layout as L
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
