"""Batched counterparts of tactics2d.traffic: status enums, event detectors, ScenarioManager.

Mirrors (tactics2d v0.1.9rc3):
    ScenarioStatus / TrafficStatus          traffic/status.py:10-61
    EventBase.update / reset                traffic/event_detection/event_base.py:10-19
    StaticCollision / DynamicCollision      traffic/event_detection/collision.py:12-46
    OutBound                                traffic/event_detection/out_bound.py:12-65
    OffLane                                 traffic/event_detection/off_lane.py:10-20
    OffRoute                                traffic/event_detection/off_route.py:12-51
    TimeExceed                              traffic/event_detection/time_exceed.py:10-36
    ScenarioManager                         traffic/scenario_manager.py:13-98
    _ParkingScenarioManager.update/check_status/reset   envs/parking.py:352-441

One `BatchedScenarioManager` owns one ParticipantPool = n_env independent scenes.  `update()` is one
t2d_integrate launch for every participant of every scene, `check_status()` one t2d_collide launch
(flags + the ordered status logic); `step()` runs both (t2d_step).  The detectors are views on the
flags of the last launch -- there is no per-participant Python loop and no CPU path.
"""
from enum import IntEnum

import numpy as np

from . import layout as L
from .pool import ParticipantPool


class ScenarioStatus(IntEnum):
    """traffic/status.py:10-30"""
    NORMAL = 1
    COMPLETED = 2
    TIME_EXCEEDED = 3
    OUT_BOUND = 4
    NO_ACTION = 5
    FAILED = 6


class TrafficStatus(IntEnum):
    """traffic/status.py:33-61"""
    NORMAL = 1
    UNKNOWN = 2
    COLLISION_STATIC = 3
    COLLISION_DYNAMIC = 4
    OFF_ROUTE = 5
    OFF_LANE = 6
    VIOLATION_RETROGRADE = 7
    VIOLATION_NON_DRIVABLE = 8
    VIOLATION_TRAFFIC_LIGHT = 9
    VIOLATION_TRAFFIC_SIGN = 10


def polygons_to_csr(per_env_polygons):
    """[[poly(n,2), ...] per env] -> (env_offsets, vertex_offsets, verts_xy) for the C ABI."""
    eo, vo, xy = [0], [0], []
    for polys in per_env_polygons:
        for q in polys:
            q = np.asarray(q, np.float32).reshape(-1, 2)
            xy.append(q); vo.append(vo[-1] + len(q))
        eo.append(eo[-1] + len(polys))
    xy = np.concatenate(xy) if xy else np.zeros((0, 2), np.float32)
    return np.array(eo, np.int32), np.array(vo, np.int32), xy


def as_polyline(route):
    """OffRoute.reset's acceptance rule (off_route.py:45-49): a LineString (anything with `.coords`) or what LineString(...)
    accepts -- a sequence of at least two points of two (or three: z is dropped) numbers each -- as float32 (n, 2); TypeError
    otherwise, as the reference raises for whatever LineString refuses."""
    try:
        pts = np.asarray(list(route.coords) if hasattr(route, "coords") else route, np.float64)
        if pts.ndim != 2 or pts.shape[0] < 2 or pts.shape[1] not in (2, 3):
            raise ValueError(pts.shape)
    except Exception:
        raise TypeError("The route should be a LineString or a list of points.") from None
    return np.ascontiguousarray(pts[:, :2], np.float32)


def routes_to_csr(route_sets):
    """[[polyline, ...] per route set] -> (set_route_offsets, route_vert_offsets, verts_xy) for t2d_set_routes; every polyline
    goes through as_polyline (TypeError for what cannot become a polyline of >= 2 points)."""
    so, vo, xy = [0], [0], []
    for routes in route_sets:
        for r in routes:
            q = as_polyline(r)
            xy.append(q); vo.append(vo[-1] + len(q))
        so.append(so[-1] + len(routes))
    xy = np.concatenate(xy) if xy else np.zeros((0, 2), np.float32)
    return np.array(so, np.int32), np.array(vo, np.int32), xy


class _FlagDetector:
    """EventBase over one bit of the pool's event flags (evaluated by the collide kernel)."""
    bit = 0

    def __init__(self, manager=None):
        self._m = manager

    def bind(self, manager):
        self._m = manager

    def update(self, ego_only=True):
        """Reference: update(agent_pose) -> bool.  Batched: bool[n_env] for the ego of every scene
        (ego_only) or bool[n_env, max_agents] for every participant."""
        f = self._m.flags()
        hit = (f & self.bit) != 0
        return hit[:, self._m.ego_index] if ego_only else hit


class StaticCollision(_FlagDetector):
    bit = L.FLAG_COLLISION_STATIC

    def __init__(self, static_objects=None, manager=None):
        super().__init__(manager)
        self.static_objects = static_objects

    def reset(self, static_objects=None):
        """static_objects: per-env lists of convex polygons (array (n, 2), 3..8 vertices)."""
        self.static_objects = static_objects
        if self._m is not None:
            self._m._static = None if static_objects is None else polygons_to_csr(static_objects)
            self._m._push_geometry()


class DynamicCollision(_FlagDetector):
    bit = L.FLAG_COLLISION_DYNAMIC

    def reset(self):
        return


class OutBound(_FlagDetector):
    bit = L.FLAG_OUT_BOUND

    def __init__(self, boundary=None, manager=None):
        super().__init__(manager)
        self.map_boundary = boundary

    def reset(self, boundary=None):
        """boundary: (n_env, 4) xmin, xmax, ymin, ymax (out_bound.py:20-35) or None (= never out)."""
        self.map_boundary = boundary
        if self._m is not None:
            self._m._boundary = None if boundary is None else np.asarray(boundary, np.float32).reshape(-1, 4)
            self._m._push_geometry()


class OffLane(_FlagDetector):
    """The reference detector is a stub that returns False (off_lane.py:16-17).  Here it becomes real once lanes
    are supplied: `not union(lane polygons).contains(pose)` -- the predicate of OutBound (out_bound.py:37-48) applied
    to the lanes (build-defined; lanes that abut must share their vertices exactly or overlap)."""
    bit = L.FLAG_OFF_LANE

    def __init__(self, manager=None):
        super().__init__(manager)
        self.lanes = None

    def reset(self, lanes):
        self.lanes = lanes
        if self._m is not None:
            self._m._lanes = None if lanes is None else polygons_to_csr(lanes)
            self._m.pool.set_lane_geometry(self._m._lanes)


class OffRoute:
    """OffRoute (off_route.py:12-51) for every participant of every scene: `route.distance(centre) > threshold`, evaluated by
    one launch of its own (t2d_off_route) -- no flag bit, status or reward is involved.

    reset(route): the reference's form -- ONE polyline (a LineString, or a list of >= 2 points; TypeError otherwise) that
    every participant of every scene follows.  The batched forms, by keyword:
        reset(route_sets=[[polyline, ...] per set], set_of_env=int[n_env] | None, route_of=int[n_env, max_agents] | int)
            per-scene sets of routes (None: set 0 serves every scene), per-participant route inside the scene's set (-1: none)
        reset(source=DeviceTrajectory | ReplaySource, route_of=None, src_env=None, windows=None)
            the recorded trace of a participant as its route (route_of None: its own), read on the device
    threshold: a scalar or float[n_env, max_agents].  Participants without a route, inactive ones and non-finite positions
    give False / NaN (build-defined)."""

    def __init__(self, threshold, manager=None):
        self.threshold = threshold
        self.route = None
        self._m = None
        if manager is not None:
            self.bind(manager)

    def bind(self, manager):
        self._m = manager
        manager.off_route = self

    @property
    def installed(self):
        return self.route is not None

    def reset(self, route=None, *, route_sets=None, set_of_env=None, route_of=None, source=None, src_env=None, windows=None):
        if sum(v is not None for v in (route, route_sets, source)) != 1:
            raise TypeError("The route should be a LineString or a list of points.")
        if route is not None:
            route_sets, set_of_env, route_of = [[as_polyline(route)]], None, 0
        if route_sets is not None:
            csr = route_sets if isinstance(route_sets, tuple) else routes_to_csr(route_sets)
            if self._m is not None:
                self._m.pool.set_routes(csr, set_of_env, 0 if route_of is None else route_of, self.threshold)
            self.route = csr
        else:
            if self._m is None:
                raise ValueError("trace routes live on a pool's device: bind the detector to a manager first")
            self._m.pool.set_routes_from(source, src_env, windows, route_of, self.threshold)
            self.route = source
        if self._m is not None:
            self._m._off_route_fresh = False

    def _result(self):
        if self.route is None:
            raise ValueError("The route should be set before the event detection.")
        m = self._m
        if not m._off_route_fresh:   # (step() / check_status() launch it behind the step; otherwise: now)
            m.pool.off_route()
            m._off_route_fresh = True
        return m.pool.off_route_all()

    def update(self, ego_only=True):
        """Reference: update(location) -> bool.  Batched: bool[n_env] for the ego of every scene (ego_only) or
        bool[n_env, max_agents]; ValueError before reset."""
        off = self._result()[1]
        return off[:, self._m.ego_index] if ego_only else off

    def distance(self, ego_only=True):
        """float32 distance to the route behind the last verdict (NaN: not evaluated)."""
        d = self._result()[0]
        return d[:, self._m.ego_index] if ego_only else d


class TimeExceed:
    """time_exceed.py:10-36; the counter lives in the pool (cnt_step per scene)."""

    def __init__(self, max_step, manager=None):
        self.max_step = max_step
        self._m = manager

    def bind(self, manager):
        self._m = manager

    def update(self):
        return self._m.pool.download(L.F_CNT_STEP) > self.max_step

    def reset(self):
        return


class BatchedScenarioManager:
    """ScenarioManager (traffic/scenario_manager.py:13-98) for n_env scenes at once."""

    def __init__(self, n_env, max_agents=1, max_step=None, step_size=None, render_fps=60, off_screen=True,
                 device_id=0):
        self.render_fps = render_fps
        self.off_screen = off_screen
        self.max_step = max_step
        self.step_size = int(step_size) if step_size is not None else int(1000 / render_fps)
        self.n_env, self.max_agents = n_env, max_agents
        self.ego_index = 0
        self.pool = ParticipantPool(n_env, max_agents, device_id)
        self.render_manager = None
        self._static = self._lanes = self._boundary = None
        self.status_checklist = {
            "time_exceed": TimeExceed(max_step, self),
            "out_bound": OutBound(manager=self),
            "collision": StaticCollision(manager=self),
            "dynamic_collision": DynamicCollision(self),
            "off_lane": OffLane(self),
        }
        self._flags_cache = None
        self.off_route = None          # an OffRoute detector bound to this manager (OffRoute(threshold, manager)), optional
        self._off_route_fresh = False  # the pool's off-route buffers hold the verdict of the current state

    def _after_step(self, stream):
        """behind a step: the flags are new, and -- only when a route is installed -- one t2d_off_route launch on the same stream"""
        self._flags_cache = None
        self._off_route_fresh = False
        if self.off_route is not None and self.off_route.installed:
            self.pool.off_route(None, None, stream)
            self._off_route_fresh = True

    # -- state views ----------------------------------------------------------------------------
    @property
    def cnt_step(self):
        return self.pool.download(L.F_CNT_STEP)

    @property
    def scenario_status(self):
        return self.pool.download(L.F_STATUS)[:, 0]

    @property
    def traffic_status(self):
        return self.pool.download(L.F_STATUS)[:, 1]

    def flags(self):
        if self._flags_cache is None:
            self._flags_cache = self.pool.download(L.F_FLAGS).reshape(self.n_env, self.max_agents)
        return self._flags_cache

    def _push_geometry(self):
        self.pool.set_static_geometry(self._static, self._boundary)

    # -- ScenarioManager interface -----------------------------------------------------------------
    def configure(self, rows, check_dynamic=False, check_off_lane=False, **options):
        self.pool.set_param_table(rows)
        self.pool.set_status_config(max_step=self.max_step if self.max_step is not None else 0,
                                    ego_index=self.ego_index, check_dynamic=int(check_dynamic),
                                    check_off_lane=int(check_off_lane), **options)

    def reset(self, x, y, heading, speed, type_id, active=None, env_mask=None):
        """Load the start states (Trajectory reset + detector resets, envs/parking.py:397-441)."""
        self.pool.reset(x, y, heading, speed, type_id, active, env_mask=env_mask)
        self.pool.snapshot()
        self._flags_cache = None
        self._off_route_fresh = False
        self._ego_velocity_derived = None   # (an env's ego model is fixed until the next reset: see get_observation)

    def update(self, act0, act1, stream=None):
        """Physics step of every participant (parking.py:352-359: `physics_model.step` + add_state)."""
        self.pool.set_actions(act0, act1)
        self.pool.integrate(self.step_size, stream)
        self._flags_cache = None
        self._off_route_fresh = False

    def check_status(self, stream=None):
        """Ordered event checks (parking.py:361-392) -> (scenario_status[E], traffic_status[E])."""
        self.pool.check_status(self.step_size, stream)
        self._after_step(stream)
        st = self.pool.download(L.F_STATUS)
        return st[:, 0], st[:, 1]

    def step(self, act0=None, act1=None, stream=None):
        """update + check_status in one t2d_step (two launches, stream ordered)."""
        if act0 is not None:
            self.pool.set_actions(act0, act1)
        self.pool.step(self.step_size, stream)
        self._after_step(stream)

    def step_host(self, actions, lidar=False, fresh=True):
        """update + check_status for every scene, host to host, in ONE library call (t2d_step_host): `actions` float32
        [n_env * max_agents, 2] in the reference's action layout (steering, accel) -- (ay, ax) for a point mass -- in, a
        pool.HostFrame out: the ego's state, reward, status bytes, IoU, frame, counters (and the 360-beam scan with lidar=True,
        after lidar_config) of every scene as numpy views of one pinned frame, instead of one blocking copy per field."""
        want = (bool(lidar),)
        if getattr(self, "_frame_cfg", None) != want:
            self.pool.frame_config(lidar=bool(lidar))
            self._frame_cfg = want
        a = np.ascontiguousarray(actions, np.float32).reshape(self.n_env * self.max_agents, 2)
        self._flags_cache = None
        self._off_route_fresh = False
        return self.pool.step_host(a, self.step_size, fresh=fresh)

    def render(self):
        raise NotImplementedError("rendering is outside the accelerated path (DESIGN.md section 9)")

    def get_active_participants(self, frame=None):
        """Per scene, the indices of the active participants (scenario_manager.py:83-94).  frame None: the participants active
        on the device now.  With a frame (ms of env time) on a pool with a bound replay source (pool.replay_bind): replayed
        participants answer by their recording's window at that env time -- `p.is_active(frame)`, without a device call;
        `replayed` (bool [n_env, max_agents], default: every participant) says which participants are replayed ones, the
        others count as active."""
        if frame is None or getattr(self.pool, "replay_source", None) is None:
            ids = self.pool.download(L.F_IDS).reshape(self.n_env, self.max_agents)
            act = (ids >> 16) & 0xff
            return [np.nonzero(a)[0].tolist() for a in act]
        src = self.pool.replay_source
        act = src.active_mask(np.asarray(frame) + self.pool.replay_offset_ms, self.pool.replay_src_env)
        replayed = getattr(self, "replayed", None)
        if replayed is not None:
            act = act | ~np.asarray(replayed, bool).reshape(self.n_env, self.max_agents)
        return [np.nonzero(a)[0].tolist() for a in act]

    def get_observation(self):
        """State observation of the ego of every scene: float32 [n_env, 6] = x, y, heading, speed, vx, vy
        (the reference returns a rendered camera image, scenario_manager.py:96-98: not on this path)."""
        cols = [self.pool.download(f).reshape(self.n_env, self.max_agents)[:, self.ego_index]
                for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY)]
        # SingleTrackDynamics / SingleTrackDrift return a State without vx, vy (single_track_dynamics.py:220-227) and
        # the pool's VX / VY fields are not written by those models (include/t2d.h): State.velocity then DERIVES
        # (speed cos(heading), speed sin(heading)) (state.py:152-169) -- done here the same way, lazily
        # (the mask is read once per reset, not per call: an ego's model does not change in between)
        if getattr(self, "_ego_velocity_derived", None) is None:
            model = self.pool.download(L.F_IDS).reshape(self.n_env, self.max_agents)[:, self.ego_index] & 0xff
            self._ego_velocity_derived = (model == L.MODEL_DYNAMICS) | (model == L.MODEL_DRIFT)
        derived = self._ego_velocity_derived
        if derived.any():
            h, v = cols[2].astype(np.float64), cols[3].astype(np.float64)
            cols[4] = np.where(derived, (v * np.cos(h)).astype(np.float32), cols[4])
            cols[5] = np.where(derived, (v * np.sin(h)).astype(np.float32), cols[5])
        return np.stack(cols, 1)

    def get_lidar_observation(self, out=None, stream=None):
        """Lidar observation of EVERY participant of every scene (SingleLineLidar bound to each of them, sensor/lidar.py:29;
        after pool.lidar_config): float32 [n_env, max_agents, n_beams], +inf = no return, one launch.
        out: a contiguous float32 CUDA tensor of that shape -- the scan is written straight into it, asynchronously on
        `stream` (a torch stream; default the tensor's device's current stream), and `out` is returned; None: a numpy array."""
        pool = self.pool
        if out is None:
            pool.lidar_scan_all(None, None if stream is None else stream.cuda_stream)
            return pool.lidar_all()
        import torch
        shape = (self.n_env, self.max_agents, pool.n_beams)
        if not isinstance(out, torch.Tensor) or not out.is_cuda or out.dtype != torch.float32 or tuple(out.shape) != shape or \
                not out.is_contiguous() or out.device.index != pool.device_id:
            raise ValueError(f"out must be a contiguous float32 tensor {list(shape)} on cuda:{pool.device_id}")
        st = stream if stream is not None else torch.cuda.current_stream(out.device)
        pool.lidar_scan_all(out.data_ptr(), st.cuda_stream)
        return out

    def close(self):
        self.pool.close()
