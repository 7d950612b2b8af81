"""Gym-style environments on top of the batched hot path.

Mirrors (tactics2d v0.1.9rc3) `ParkingEnv` -- envs/parking.py:44-444 -- and `RacingEnv` -- envs/racing.py:40-384 (VecRacingEnv
below) -- for the part that is on
the accelerated path: `step()` = physics update of the ego (`_ParkingScenarioManager.update`, :352-359)
+ ordered status checks (`check_status`, :361-392) + terminated / truncated / reward (:243-250,
:148-166).  `Arrival` (IoU >= 0.95 with the target bay -> COMPLETED, +5, terminated), `NoAction` (IoU with the
previous pose > 0.999 on more than 100 checks, including the reference's quirk of reporting it in
`traffic_status`) and the IoU / distance reward shaping are evaluated in the same launch.  `info["lidar"]` is the 360-beam / 20 m
SingleLineLidar scan of the same poses (t2d_lidar_scan).  observation="state" (the default) returns the ego state vector;
observation="camera" returns the reference's declared observation, the (200, 200, 3) uint8 top-down image of the camera
bound to the agent (tactics2d_amd.sensor.BEVCamera, one launch behind the step).  Windows, matplotlib and
the WebGL viewer (`render()`) stay outside the accelerated path.

gymnasium is not a dependency: `Box` below is the minimal stand-in for `spaces.Box`.
"""
import ctypes as C

import numpy as np

from . import layout as L, scenarios
from ._ffi import ERR_ACTION, T2DError
from .traffic import BatchedScenarioManager, ScenarioStatus, TrafficStatus

_SCENARIO = {int(v): v for v in ScenarioStatus}
_TRAFFIC = {int(v): v for v in TrafficStatus}
MAX_STEER = 0.524  # envs/parking.py:30
MAX_ACCEL = 2.0    # envs/parking.py:31


class InvalidAction(Exception):
    """Same role as gymnasium.error.InvalidAction in envs/parking.py:235-236."""


class Box:
    def __init__(self, low, high, dtype=np.float32):
        self.low = np.asarray(low, dtype)
        self.high = np.asarray(high, dtype)
        self.shape = self.low.shape
        self.dtype = np.dtype(dtype)

    def contains(self, a):
        a = np.asarray(a)
        return a.shape[-len(self.shape):] == self.shape and bool(np.all(a >= self.low) and np.all(a <= self.high))

    def sample(self, rng, n=None):
        size = self.shape if n is None else (n,) + self.shape
        return rng.uniform(self.low, self.high, size).astype(self.dtype)


CAMERA_WINDOW = (200, 200)   # Box(0, 255, (200, 200, 3), uint8): envs/racing.py:102, envs/parking.py:130


def _camera_space():
    return Box(np.zeros(CAMERA_WINDOW[::-1] + (3,)), np.full(CAMERA_WINDOW[::-1] + (3,), 255), np.uint8)


def _check_observation(observation):
    if observation not in ("state", "camera"):
        raise ValueError(f"unknown observation {observation!r}")
    return observation


class VecParkingEnv:
    """n_envs independent ParkingEnv scenes stepped by one t2d_step per call.

    step(actions[n_envs, 2]) -> (obs[n_envs, 6], reward[n_envs], terminated[n_envs], truncated[n_envs], infos)
    The action layout is the reference's: (steering, accel) (envs/parking.py:239)."""

    _max_steer = MAX_STEER
    _max_accel = MAX_ACCEL
    _discrete_actions = {1: (0, 0), 2: (-0.5, 0), 3: (0.5, 0), 4: (0, 1), 5: (0, -1)}  # parking.py:95

    def __init__(self, n_envs, max_step=int(2e4), continuous=True, auto_reset=False, seed=0, device_id=0,
                 scene_source="layout", type_proportion=0.5, info_lidar=True, copy=True, zero_copy=None, lidar_beams=360,
                 observation="state", rs_planner=False, rs_follow=False, occupancy=None):
        """scene_source: "generator" = the device-side ParkingLotGenerator (tactics2d_amd.generator; bay and
        parallel scenes with the reference's rejection sampler, `type_proportion` as in envs/parking.py:331-333),
        "layout" = the fixed bay layout of scenarios.parking (BASELINE config 2).
        The host path (`step`) is ONE library call per step (t2d_step_host): actions up, step + 360-beam scan + pack, one
        frame back (pool.HostFrame).  info_lidar=False leaves the scan out of the host path (info["lidar"] is None: at 4096
        envs the 360 floats per env are 5.9 MB per step over PCIe).  The arrays handed out are views of pinned host frames:
        copy=True (default) fills a frame nobody holds a view of any more -- as good as fresh arrays, without a memcpy (a
        caller that keeps many steps' results by reference gets real copies once the four frames are held); copy=False
        takes the frames in turn (valid for three further steps); copy="always" hands out arrays that OWN their memory (one
        memcpy of the frame per step: nothing the caller holds is ever touched again, whatever it keeps and however).
        lidar_beams: beams of the scan in info["lidar"] / step_torch()["lidar"], a divisor of the reference's 360
        (envs/parking.py:303-304): the scan is then exactly `full_scan[:, ::360 // lidar_beams]` -- the tutorial policy keeps
        every third beam (docs/tutorial/train_parking_demo.ipynb), i.e. lidar_beams=120 moves a third of the bytes.  zero_copy: the kernels read the actions from / write
        the frame to mapped host memory instead of copy commands (None = for pools of at most 16384 envs; beyond, the
        8 B per env of the actions would cross PCIe inside the step kernel).
        observation: "state" = the ego's 6-vector; "camera" = the reference's observation, the uint8 [200, 200, 3] image of a
        BEVCamera with perception_range (20, 20, 20, 20) bound to the agent (envs/parking.py:130, :306-308): reset() and step()
        return [n_envs, 200, 200, 3] arrays (downloaded: 120 KB per env), step_torch() adds `image` / `image_class`.
        rs_planner: step_torch() adds `rs_plan`, the tutorial's Reeds-Shepp plan of every env (planner.RSPlanner: dict of views
        of the plan records), one launch behind the scan on the same stream.
        rs_follow (needs rs_planner): the tutorial's hybrid policy.  step_torch() puts the path follower (planner.RSFollower, the
        notebook's RSAgent) in front of the step: an env that holds a path, or whose last plan was found, is stepped with the
        follower's action, the others with the caller's; `actions` itself is never written.  The result gains `action` (float32
        [n, 2]: what was stepped) and `rs_follow` (the follower's record views); reset() clears the follower and ends with a scan
        and a plan of the reset state, so the first step has a record to adopt.
        occupancy: None, or the keywords of sensor.OccupancyGrid behind the pool (H, W, cell_size, origin, inflate, ...): reset()
        and step_torch() launch the occupancy grid of every env behind the step (and the scan) on the same stream;
        step_torch() adds `occupancy` (float64 [n, H, W]: the weights search.HybridAStar.plan_batch / Dijkstra.plan_batch read
        in place, with `self.occupancy_grid.planner_kwargs()`) and `occupancy_mask` (u8 [n, H, W])."""
        self.observation = _check_observation(observation)
        self.occupancy = None if occupancy is None else dict(occupancy)
        self.occupancy_grid = None
        self.rs_planner = bool(rs_planner)
        self.rs_follow = bool(rs_follow)
        if self.rs_follow and not self.rs_planner:
            raise ValueError("rs_follow=True needs rs_planner=True")
        self.planner = self.follower = None
        if scene_source not in ("layout", "generator"):
            raise ValueError(f"unknown scene_source {scene_source!r}")
        self.scene_source = scene_source
        self.type_proportion = type_proportion
        self.device_id = device_id
        self.n_envs = int(n_envs)
        self.max_step = max_step
        self.continuous = continuous
        self.auto_reset = auto_reset
        self.info_lidar = bool(info_lidar)
        if copy not in (True, False, "always"):
            raise ValueError('copy must be True, False or "always"')
        self.copy = copy is True
        self.copy_always = copy == "always"
        self.lidar_beams = int(lidar_beams)
        if self.lidar_beams < 1 or 360 % self.lidar_beams:
            raise ValueError("lidar_beams must divide 360 (a regular subset of the reference's scan)")
        self.zero_copy = self.n_envs <= 16384 if zero_copy is None else bool(zero_copy)
        self.observation_space = _camera_space() if self.observation == "camera" else Box(np.full(6, -np.inf), np.full(6, np.inf))
        self.camera = None
        self.action_space = Box([-self._max_steer, -self._max_accel], [self._max_steer, self._max_accel])
        lo, hi = self.action_space.low, self.action_space.high
        self._action_box = np.float32([lo[0], hi[0], lo[1], hi[1]]) if continuous else None
        # ScenarioManager(max_step, step_size=100, ...)  envs/parking.py:144-146
        self.scenario_manager = BatchedScenarioManager(self.n_envs, 1, max_step, 100, device_id=device_id)
        self._seed = seed
        self._scene = None

    # ------------------------------------------------------------------ reset
    def reset(self, seed=None, options=None):
        """New scenes for every env (envs/parking.py:397-405: map_.reset(), map_generator.generate(map_),
        agent.reset(start_state))."""
        if seed is not None:
            self._seed = int(seed)
        m = self.scenario_manager
        if self.scene_source == "generator":
            # generate + install in one launch on the device; with auto_reset every finished episode continues in a
            # NEW scene (the reference's reset() per episode), not in a copy of the first one
            from .participant import VEHICLE_TEMPLATE, vehicle_model
            size = VEHICLE_TEMPLATE["medium_car"][:2]
            ego = vehicle_model("medium_car", "kinematics", speed_range=(-0.5, 0.5), accel_range=(-2.0, 2.0),
                                steer_range=(-0.524, 0.524))
            rows = ego.param_row(L.SHAPE_OBB, *size)[None]
            m.configure(rows, check_dynamic=False, check_off_lane=False, check_arrival=1, check_no_action=1,
                        no_action_max_step=100, shaped_reward=1)
            m.pool.parking_scenes(self._seed, self.type_proportion, size, regenerate=self.auto_reset)
            self._generated = m.pool.get_parking_scenes()
            bad = self._generated.info & 0x1e
            if bad.any():
                raise RuntimeError(f"{int((bad != 0).sum())} generated scenes are flagged; use another seed")
            self._scene = self._generated.scene(max_step=self.max_step)
        else:
            sc = scenarios.parking(self.n_envs, seed0=self._seed * self.n_envs)
            self._scene = sc
            m.pool.set_target_areas(sc.target)
            m.pool.set_target_headings(sc.target_heading)
            m.configure(sc.rows, check_dynamic=False, check_off_lane=False, check_arrival=1, check_no_action=1,
                        no_action_max_step=100, shaped_reward=1)
            m.status_checklist["collision"].reset(_csr_to_lists(sc.static))
            m.status_checklist["out_bound"].reset(sc.boundary)
            m.reset(sc.x, sc.y, sc.heading, sc.speed, sc.type_id, sc.active)
        m.pool.bind_actions(None, None)   # a step_torch binding does not outlive the episode set-up
        m.pool.set_auto_reset(self.auto_reset)
        # SingleLineLidar(perception_range=20, freq_detect=360 * 10)  envs/parking.py:303-304,422-431
        m.pool.lidar_config(self.lidar_beams, 20.0, include_participants=False, subsample_of=360)
        # the target area changes under the caller only when scenes are regenerated on the device: the frame carries it then
        self._moving_targets = self.scene_source == "generator" and self.auto_reset
        m.pool.frame_config(lidar=self.info_lidar, target=self._moving_targets, zero_copy=self.zero_copy)
        self._target_area, self._target_heading = self._scene.target, self._scene.target_heading
        if self.rs_planner:
            from .planner import RSPlanner
            # RSPlanner(scenario_manager.agent, lidar_num, lidar_range)  tutorial cell 9; the ego is a medium_car with steer_range 0.524
            self.planner = RSPlanner(m.pool, "medium_car", lidar_range=20.0, steer_hi=0.524)
        if self.rs_follow:
            # agent.reset(); choose_action(info0, ...)  tutorial cell 18: a cleared follower and a plan of the reset state
            import torch
            from .planner import RSFollower
            self.follower = RSFollower(m.pool, self.planner)
            dev = torch.device("cuda", self.device_id)
            self._t_lidar = torch.empty((self.n_envs, self.lidar_beams), dtype=torch.float32, device=dev)
            self._t_views = None
            st = torch.cuda.current_stream(dev)
            m.pool.lidar_scan(self._t_lidar.data_ptr(), st.cuda_stream)
            self.planner.plan(self._t_lidar, st)
        fr = m.pool.frame_fetch(fresh=self.copy)
        fr = self._last = fr.copy() if self.copy_always else fr
        if self.occupancy is not None:   # the grid of the new lots, on torch's current stream
            from .sensor import OccupancyGrid
            if self.occupancy_grid is None:
                self.occupancy_grid = OccupancyGrid(m.pool, **self.occupancy)
            self.occupancy_grid.render()
        if self.observation == "camera":
            from .sensor import BEVCamera
            # BEVCamera(perception_range=(20, 20, 20, 20)) bound to the agent  envs/parking.py:306-308
            self.camera = BEVCamera(m.pool, (20, 20, 20, 20), CAMERA_WINDOW, 0, True, ("static", "target", "participants", "arrows"))
            return self.camera.render_numpy()["image"], self._infos(fr)
        return fr.obs, self._infos(fr)

    @property
    def generated(self):
        """The generated scenes the envs are in NOW (a generator.ParkingScenes + .episode): fetched from the device on demand
        when scenes are regenerated there (nothing on the step path reads it: the frame carries the target areas)."""
        if getattr(self, "_moving_targets", False):
            self._generated = self.scenario_manager.pool.get_parking_scenes()
        return self._generated

    # ------------------------------------------------------------------ step
    def _to_continuous(self, actions):
        if self.continuous:
            # (`action_space.contains` runs inside t2d_step_host, in the pass that stages the actions: 50 us of numpy at 4096 envs)
            try:
                return np.ascontiguousarray(actions, np.float32).reshape(self.n_envs, 2)
            except (ValueError, TypeError):
                raise InvalidAction(f"Action {actions} is not in the action space.") from None
        idx = np.asarray(actions).reshape(self.n_envs)
        if not np.all(np.isin(idx, list(self._discrete_actions))):
            raise InvalidAction(f"Action {actions} is not in the action space.")
        return np.array([self._discrete_actions[int(i)] for i in idx], np.float32)

    def step(self, actions):
        """(obs[n, 6], reward[n], terminated[n], truncated[n], infos) -- envs/parking.py:219-256 for every env: one
        t2d_step_host call (physics_model.step(state, accel, steering) parking.py:355 + check_status + scan + pack)."""
        if self._scene is None:
            raise RuntimeError("call reset() first")
        a = self._to_continuous(actions)
        try:
            fr = self.scenario_manager.pool.step_host(a, 100, action_box=self._action_box, fresh=self.copy)
            fr = self._last = fr.copy() if self.copy_always else fr
        except T2DError as exc:
            if exc.code == ERR_ACTION:
                raise InvalidAction(f"Action {actions} is not in the action space.") from None
            raise
        self.scenario_manager._flags_cache = None
        obs = self.camera.render_numpy()["image"] if self.observation == "camera" else fr.obs
        return obs, fr.reward, fr.terminated, fr.truncated, self._infos(fr)

    def step_torch(self, actions, stream=None):
        """The device-resident step: `actions` is a float32 CUDA tensor [n_envs, 2] in the reference's layout (steering,
        accel); nothing is copied to the host and nothing synchronises.  Returns a dict of torch tensors that are
        ZERO-COPY VIEWS of the pool (valid until the next step): state [6 x n_envs] columns (vx, vy as written by the ego's
        SingleTrackKinematics -- a dynamics / drift ego leaves those two fields alone, include/t2d.h), reward, status (u8 [n, 4]:
        scenario, traffic, terminated, truncated), iou, and `lidar` [n_envs, lidar_beams] written by the scan kernel straight
        into a tensor owned by this env -- the observation buffer handed back to the policy.  With observation="camera":
        `image` u8 [n, 200, 200, 3] and `image_class` u8 [n, 200, 200], rendered on the same stream behind the step.
        Out-of-range actions are the caller's responsibility here (the numpy `step` raises InvalidAction like the reference)."""
        import torch
        if self._scene is None:
            raise RuntimeError("call reset() first")
        pool = self.scenario_manager.pool
        dev = actions.device
        cur = torch.cuda.current_stream(dev)
        st = stream if stream is not None else cur
        if st != cur:
            st.wait_stream(cur)   # `actions` was produced on the caller's current stream; the step reads it in place
        with torch.cuda.stream(st):
            # the [n, 2] (steering, accel) tensor is read in place: accel = column 1, steering = column 0, stride 2
            # (two copy kernels per step otherwise: 4.7 us of a 36 us vector step); kept alive until the next step
            if actions.dtype != torch.float32 or tuple(actions.shape) != (self.n_envs, 2):
                raise ValueError(f"actions must be float32 [{self.n_envs}, 2]")
            self._act = actions if actions.is_contiguous() else actions.contiguous()
            follow = self.follower.follow(self._act, stream=st) if self.follower is not None else None
            base = self._act.data_ptr() if follow is None else follow["action_rows"].data_ptr()
            pool.bind_actions(base + 4, base, stride=2)
            pool.step(100, st.cuda_stream)
            if getattr(self, "_t_lidar", None) is None or self._t_lidar.device != dev or getattr(self, "_t_views", None) is None:
                if getattr(self, "_t_lidar", None) is None or self._t_lidar.device != dev:
                    self._t_lidar = torch.empty((self.n_envs, self.lidar_beams), dtype=torch.float32, device=dev)
                view = lambda f: torch.as_tensor(pool.device_array(f), device=dev)
                self._t_views = dict(x=view(L.F_X), y=view(L.F_Y), heading=view(L.F_HEADING), speed=view(L.F_SPEED),
                                     vx=view(L.F_VX), vy=view(L.F_VY), reward=view(L.F_REWARD), status=view(L.F_STATUS),
                                     iou=view(L.F_IOU))
            pool.lidar_scan(self._t_lidar.data_ptr(), st.cuda_stream)
            cam = self.camera.render(st.cuda_stream) if self.observation == "camera" else {}
            plan = self.planner.plan(self._t_lidar, st) if self.planner is not None else None
            occ = self.occupancy_grid.render(st.cuda_stream) if self.occupancy_grid is not None else None
        out = dict(self._t_views)
        out["lidar"] = self._t_lidar
        if occ is not None:
            out["occupancy"], out["occupancy_mask"] = occ["occupancy"], occ["occupancy_mask"]
        if plan is not None:
            out["rs_plan"] = plan
        if follow is not None:
            out["action"] = follow.pop("action_rows")
            out["rs_follow"] = follow
        out.update(cam)   # image, image_class: the poses (and, with regenerated scenes, the lots) the returned state shows
        return out

    def _infos(self, fr):
        """_get_infos (envs/parking.py:203-217) for every env, as views of the frame."""
        obs, st = fr.obs, fr.status
        ta, th = (fr.target, fr.target_heading) if self._moving_targets else (self._target_area, self._target_heading)
        return dict(state=dict(x=obs[:, 0], y=obs[:, 1], heading=obs[:, 2], speed=obs[:, 3], vx=obs[:, 4], vy=obs[:, 5],
                               frame=fr.frame_ms),
                    scenario_status=st[:, 0], traffic_status=st[:, 1],
                    target_area=ta, target_heading=th,
                    diff_position=fr.rel[:, 0], diff_angle=fr.rel[:, 1], diff_heading=fr.rel[:, 2],
                    iou=fr.iou, lidar=fr.lidar, episode=fr.episode)

    def _targets(self):
        """Target areas / headings of the scenes the envs are in NOW (as of the last step / reset)."""
        if self._moving_targets:   # (the env keeps the HostFrame object, not views of it: the frame stays free to be refilled)
            return self._last.target.copy(), self._last.target_heading.copy()
        return self._target_area, self._target_heading

    def render(self):
        raise NotImplementedError("rendering is outside the accelerated path")

    def close(self):
        """Frees the pool -- and with it the pinned frames: arrays handed out by reset() / step() are views of that memory
        (DESIGN.md 5a), so copy what has to outlive the env before closing it."""
        self.scenario_manager.close()


class VecRacingEnv:
    """n_envs independent RacingEnv scenes (envs/racing.py:40-384): a `medium_car` on SingleTrackKinematics (interval 100 ms)
    on a generated Bezier track of some hundred lane tiles, stepped by one t2d_step and one t2d_track_progress per call.

    step(actions[n_envs, 2]) -> (obs[n_envs, 6], reward[n_envs], terminated[n_envs], truncated[n_envs], infos); the action
    layout is the reference's: (steering in +-0.5, accel in -4 .. 2), or an index into its 11 x 13 discrete table
    (racing.py:111-115).  observation="state" (the default): the ego state vector, as in VecParkingEnv; observation="camera":
    the reference's observation, the uint8 [200, 200, 3] image of a BEVCamera with perception_range (30, 30, 50, 10) bound to
    the agent (racing.py:102, :234-236) -- obs is then [n_envs, 200, 200, 3] (downloaded by reset() / step(); step_torch() hands
    out `image` / `image_class` as views, rendered behind the progress / restore launches, so after an auto-reset the image
    shows the start pose the returned state shows).  infos carries tile_visiting, num_visited_tile and num_tile beside the state and the two statuses.

    n_tracks distinct tracks are generated per reset() (tactics2d_amd.generator.RacingTrackGenerator, numpy's global random
    stream as in the reference; seeded with `seed` at the first reset and whenever reset(seed=...) names one); env e drives
    on track e % n_tracks.  Tracks are shifted to the centre of their bounding box before they are rounded to fp32.

    progress_rule: "reference" is the reference's _locate_agent bit for bit -- including its degenerate case: when the car
    touches only the tile it was last seen on, EVERY tile is marked visited, so an episode ends COMPLETED within a handful of
    steps of driving off the start line.  "forward" (the default, build-defined) is the same touch test and the same march
    with two changes: only tile_visiting and its first max_advance successors are looked at (0 = the whole ring), and only
    the tiles strictly between tile_visiting and the touched run are filled in -- a lap is complete when the car has driven
    it.  max_advance only applies to the forward rule; the default, 8 tiles, covers the car's own length, short closing
    tiles and a few steps without contact at the template's top speed (6.9 m per step, less than one 10 m tile) and is far
    below half of any generated ring, so a car that backs onto the tile behind it is not credited with a lap.
    check_off_road=True installs the tiles as lane geometry and ends an episode when the car leaves them (traffic status
    OFF_LANE, reward -5; build-defined); False is the reference, whose off-road detector never fires.

    track_source="device": the tracks come from the device generator instead (t2d_set_tracks_generated, include/t2d.h): reset()
    installs ONE TRACK PER ENV in one launch -- env e drives on the track of the counter stream (seed, e), first_track = 0;
    reset(seed=...) re-keys -- and nothing but the tile counts crosses to the host (n_tracks is not used, `self.tracks` stays
    empty; pool.generated_tracks() downloads them).  The stream is the build's own: these are not the tracks the host class
    makes from numpy's stream.  new_track_per_episode=True (needs track_source="device" and auto_reset=True) is the
    reference's RacingEnv.reset (racing.py:374-383): step() / step_torch() put one regenerate launch between the progress and
    the restore launch, and a finished episode continues on a NEW track -- episode k of env e on the track of stream
    (seed, e + k n_envs) -- at its start pose; infos["num_tile"] / step_torch's `num_tile` are then the device's own counts.
    check_off_road=True needs the host's lane geometry and raises ValueError with track_source="device"."""

    _max_steer, _max_accel, _min_accel = 0.5, 2.0, -4.0   # envs/racing.py:24-26

    def __init__(self, n_envs, max_step=int(1e5), continuous=True, auto_reset=False, seed=0, n_tracks=1,
                 progress_rule="forward", max_advance=8, check_off_road=False, device_id=0, observation="state",
                 track_source="host", new_track_per_episode=False):
        self.observation = _check_observation(observation)
        if track_source not in ("host", "device"):
            raise ValueError(f"unknown track_source {track_source!r}")
        if track_source == "device" and check_off_road:
            raise ValueError("check_off_road is not supported with track_source='device' (the lane geometry is built on the host)")
        if new_track_per_episode and not (track_source == "device" and auto_reset):
            raise ValueError("new_track_per_episode needs track_source='device' and auto_reset=True")
        self.track_source, self.new_track_per_episode = track_source, bool(new_track_per_episode)
        self.camera = None
        if progress_rule not in ("forward", "reference"):
            raise ValueError(f"unknown progress_rule {progress_rule!r}")
        if not 1 <= int(n_tracks) <= int(n_envs):
            raise ValueError("n_tracks must be in 1 .. n_envs")
        self.n_envs, self.max_step, self.continuous, self.auto_reset = int(n_envs), max_step, continuous, bool(auto_reset)
        self.n_tracks, self.progress_rule, self.max_advance = int(n_tracks), progress_rule, int(max_advance)
        self.check_off_road = bool(check_off_road)
        self.device_id = device_id
        self.observation_space = _camera_space() if self.observation == "camera" else Box(np.full(6, -np.inf), np.full(6, np.inf))
        self.action_space = Box([-self._max_steer, self._min_accel], [self._max_steer, self._max_accel])
        xx, yy = np.meshgrid(np.linspace(-self._max_steer, self._max_steer, 11), np.linspace(self._min_accel, self._max_accel, 13))
        self._discrete_action = np.vstack([xx.ravel(), yy.ravel()]).T     # racing.py:111-115
        # ScenarioManager(max_step, step_size=100, ...)  envs/racing.py:117-119
        self.scenario_manager = BatchedScenarioManager(self.n_envs, 1, max_step, 100, device_id=device_id)
        self._seed, self._seeded = int(seed), False
        self.tracks = None

    # ------------------------------------------------------------------ reset
    def reset(self, seed=None, options=None):
        """New tracks (racing.py:374-383: _reset_map, _reset_agent): every env at its track's start pose, only tile 0 visited."""
        from . import mapgeom
        from .generator import RacingTrackGenerator
        from .participant import VEHICLE_TEMPLATE, vehicle_model
        if seed is not None:
            self._seed, self._seeded = int(seed), False
        if not self._seeded:
            np.random.seed(self._seed)
            self._seeded = True
        if self.track_source == "device":
            return self._reset_device()
        gen = RacingTrackGenerator()
        length, width = VEHICLE_TEMPLATE["medium_car"][:2]
        tiles, poses, bounds = [], [], []
        self.generated = []
        for _ in range(self.n_tracks):
            t = gen.generate()
            pts = t.tiles.reshape(-1, 2)
            origin = (pts.min(axis=0) + pts.max(axis=0)) / 2
            t.tiles = t.tiles - origin; t.start_line = t.start_line - origin; t.end_line = t.end_line - origin
            t.center_line = t.center_line - origin; t.start_point = t.start_point - origin
            t32 = np.float32(t.tiles)
            self.generated.append(t)
            tiles.append(t32)
            poses.append(t.start_pose(length))
            bounds.append(mapgeom.map_boundary(t32.reshape(-1, 2), np.float32(t.center_line)))   # Map.boundary: lanes + road lines
        self.tracks = tiles
        E = self.n_envs
        self.track_of_env = (np.arange(E) % self.n_tracks).astype(np.int32)
        pose = np.array(poses)[self.track_of_env]
        m = self.scenario_manager
        ego = vehicle_model("medium_car", "kinematics", steer_range=(-self._max_steer, self._max_steer),
                            accel_range=(self._min_accel, self._max_accel))
        m.configure(ego.param_row(L.SHAPE_OBB, length, width)[None], check_dynamic=False, check_off_lane=False, check_arrival=0,
                    check_no_action=1, no_action_max_step=100, shaped_reward=0)
        m.status_checklist["out_bound"].reset(np.float32(bounds)[self.track_of_env])
        if self.check_off_road:
            # (the CSR is made once per track and repeated per env: 4096 envs share n_tracks lists of some 450 polygons)
            per_track = [[q for tile in t for q in mapgeom.ring_to_convex(tile, 4)] for t in tiles]
            counts = [np.array([len(q) for q in polys]) for polys in per_track]
            verts = [np.concatenate(polys).astype(np.float32) for polys in per_track]
            soe = self.track_of_env
            eo = np.concatenate([[0], np.cumsum([len(counts[s]) for s in soe])]).astype(np.int32)
            vo = np.concatenate([[0], np.cumsum(np.concatenate([counts[s] for s in soe]))]).astype(np.int32)
            m.status_checklist["off_lane"].lanes = [per_track[s] for s in soe]   # (per env, as OffLane.reset keeps them; the lists are shared)
            m._lanes = (eo, vo, np.concatenate([verts[s] for s in soe]))
        else:
            m.status_checklist["off_lane"].lanes = None
            m._lanes = None
        m.pool.set_lane_geometry(m._lanes)
        m.reset(pose[:, 0], pose[:, 1], np.mod(pose[:, 2], 2 * np.pi), np.zeros(E), np.zeros(E, np.uint8))
        m.pool.bind_actions(None, None)
        m.pool.set_auto_reset(False)    # (finished racing episodes go back through t2d_restore behind the progress launch)
        m.pool.set_tracks(tiles, self.track_of_env, 0, self.progress_rule, self.max_advance, self.check_off_road)
        self._t_views = None
        self.num_tile = m.pool.track_n_tile
        obs = m.get_observation()
        st = np.tile(np.uint8([1, 1, 0, 0]), (E, 1))
        infos = self._infos(obs, st, np.zeros(E, np.int32), np.ones(E, np.int32))
        if self.observation == "camera":
            from .sensor import BEVCamera
            # BEVCamera(perception_range=(30, 30, 50, 10)) bound to the agent  envs/racing.py:234-236
            self.camera = BEVCamera(m.pool, (30, 30, 50, 10), CAMERA_WINDOW, 0, True, ("tracks", "participants", "arrows"))
            obs = self.camera.render_numpy()["image"]
        return obs, infos

    def _reset_device(self):
        """reset() with track_source="device": the pool is set up with placeholder poses and boundaries, then one generator
        launch and one install launch put every env's track, boundary, start pose and snapshot in place on the device"""
        from .participant import VEHICLE_TEMPLATE, vehicle_model
        length, width = VEHICLE_TEMPLATE["medium_car"][:2]
        E = self.n_envs
        m = self.scenario_manager
        ego = vehicle_model("medium_car", "kinematics", steer_range=(-self._max_steer, self._max_steer),
                            accel_range=(self._min_accel, self._max_accel))
        m.configure(ego.param_row(L.SHAPE_OBB, length, width)[None], check_dynamic=False, check_off_lane=False, check_arrival=0,
                    check_no_action=1, no_action_max_step=100, shaped_reward=0)
        m.status_checklist["out_bound"].reset(np.zeros((E, 4), np.float32))
        m.status_checklist["off_lane"].lanes = None
        m._lanes = None
        m.pool.set_lane_geometry(None)
        z = np.zeros(E)
        m.reset(z, z, z, z, np.zeros(E, np.uint8))
        m.pool.bind_actions(None, None)
        m.pool.set_auto_reset(False)
        m.pool.set_tracks_generated(E, self._seed, 0, E, None, 0, self.progress_rule, self.max_advance,
                                    regenerate=self.new_track_per_episode, car_length=length)
        self.tracks, self.generated = [], []
        self.track_of_env = np.arange(E, dtype=np.int32)
        self._t_views = None
        self.num_tile = m.pool.track_n_tile
        obs = m.get_observation()
        st = np.tile(np.uint8([1, 1, 0, 0]), (E, 1))
        infos = self._infos(obs, st, np.zeros(E, np.int32), np.ones(E, np.int32))
        if self.observation == "camera":
            from .sensor import BEVCamera
            self.camera = BEVCamera(m.pool, (30, 30, 50, 10), CAMERA_WINDOW, 0, True, ("tracks", "participants", "arrows"))
            obs = self.camera.render_numpy()["image"]
        return obs, infos

    def _infos(self, obs, st, visiting, n_visited):
        return dict(state=dict(x=obs[:, 0], y=obs[:, 1], heading=obs[:, 2], speed=obs[:, 3], vx=obs[:, 4], vy=obs[:, 5]),
                    scenario_status=st[:, 0], traffic_status=st[:, 1], tile_visiting=visiting, num_visited_tile=n_visited,
                    num_tile=self.num_tile)

    # ------------------------------------------------------------------ step
    def _to_continuous(self, actions):
        if self.continuous:
            try:
                a = np.ascontiguousarray(actions, np.float32).reshape(self.n_envs, 2)
            except (ValueError, TypeError):
                raise InvalidAction(f"Action {actions} is not in the action space.") from None
            if not self.action_space.contains(a):
                raise InvalidAction(f"Action {actions} is not in the action space.")
            return a
        try:
            idx = np.asarray(actions).reshape(self.n_envs)
            ok = np.issubdtype(idx.dtype, np.integer) and np.all((idx >= 0) & (idx < len(self._discrete_action)))
        except (ValueError, TypeError):
            ok = False
        if not ok:
            raise InvalidAction(f"Action {actions} is not in the action space.")
        return np.float32(self._discrete_action[idx])

    def step(self, actions):
        """racing.py:145-184 for every env: the physics step, _locate_agent, check_status and _get_rewards -- the step launch and
        the progress launch -- then the results are downloaded.  With auto_reset, finished episodes are back at their start
        pose in the observation returned (their reward and statuses are the terminal step's)."""
        if self.tracks is None:
            raise RuntimeError("call reset() first")
        a = self._to_continuous(actions)
        m = self.scenario_manager
        m.pool.bind_actions(None, None)   # (a step_torch binding ends here; uploading the actions would end it as well)
        m.pool.set_actions(a[:, 1], a[:, 0])
        m.pool.step(100)
        m.pool.track_progress(True)
        if self.new_track_per_episode:
            m.pool.regenerate_tracks()
        if self.auto_reset:
            m.pool.restore(done_only=True)
        m._flags_cache = None
        ts = m.pool.track_state()
        if self.new_track_per_episode:
            self.num_tile = ts["num_tile"]
        obs = m.get_observation()
        st = ts["status"]
        infos = self._infos(obs, st, ts["tile_visiting"], ts["num_visited"])
        if self.observation == "camera":
            obs = self.camera.render_numpy()["image"]
        return obs, ts["reward"], st[:, 2].astype(bool), st[:, 3].astype(bool), infos

    def step_torch(self, actions, stream=None):
        """The device-resident step: `actions` is a float32 CUDA tensor [n_envs, 2] (steering, accel), read in place; step
        launch -> progress launch (-> t2d_restore of finished episodes with auto_reset), nothing is copied to the host and
        nothing synchronises.  Returns a dict of torch tensors that are ZERO-COPY VIEWS (valid until the next step / reset):
        x, y, heading, speed, vx, vy, reward, status (u8 [n, 4]: scenario, traffic, terminated, truncated), tile_visiting,
        num_visited, num_tile -- and with observation="camera" image (u8 [n, 200, 200, 3]) and image_class (u8 [n, 200, 200]).  Out-of-range actions are the caller's responsibility here."""
        import torch
        if self.tracks is None:
            raise RuntimeError("call reset() first")
        pool = self.scenario_manager.pool
        dev = actions.device
        cur = torch.cuda.current_stream(dev)
        st = stream if stream is not None else cur
        if st != cur:
            st.wait_stream(cur)
        with torch.cuda.stream(st):
            if actions.dtype != torch.float32 or tuple(actions.shape) != (self.n_envs, 2):
                raise ValueError(f"actions must be float32 [{self.n_envs}, 2]")
            self._act = actions if actions.is_contiguous() else actions.contiguous()
            base = self._act.data_ptr()
            pool.bind_actions(base + 4, base, stride=2)
            pool.step(100, st.cuda_stream)
            pool.track_progress(True, st.cuda_stream)
            if self.new_track_per_episode:
                pool.regenerate_tracks(st.cuda_stream)
            if self.auto_reset:
                pool.restore(done_only=True, stream=st.cuda_stream)
            if self._t_views is None:
                view = lambda f: torch.as_tensor(pool.device_array(f), device=dev)
                tv = pool.track_views()
                self._t_views = dict(x=view(L.F_X), y=view(L.F_Y), heading=view(L.F_HEADING), speed=view(L.F_SPEED),
                                     vx=view(L.F_VX), vy=view(L.F_VY), reward=tv["reward"], status=tv["status"],
                                     tile_visiting=tv["tile_visiting"], num_visited=tv["num_visited"], num_tile=tv["num_tile"])
            cam = self.camera.render(st.cuda_stream) if self.observation == "camera" else {}
        self.scenario_manager._flags_cache = None
        out = dict(self._t_views)
        out.update(cam)
        return out

    def render(self):
        raise NotImplementedError("rendering is outside the accelerated path")

    def close(self):
        self.scenario_manager.close()


class ParkingEnv:
    """Single-scene adapter with the reference's 5-tuple (envs/parking.py:256)."""

    def __init__(self, type_proportion=0.5, render_mode="rgb_array", render_fps=60, max_step=int(2e4),
                 continuous=True, seed=0, scene_source="layout", info_lidar=True, zero_copy=True):
        if render_mode not in ("human", "rgb_array"):
            raise NotImplementedError(f"Render mode {render_mode} is not supported.")  # parking.py:119-120
        self.max_step = max_step
        self.continuous = continuous
        self._vec = VecParkingEnv(1, max_step, continuous, seed=seed, scene_source=scene_source,
                                  type_proportion=type_proportion, info_lidar=info_lidar, copy=False, zero_copy=zero_copy)
        self.observation_space = self._vec.observation_space
        self.action_space = self._vec.action_space
        self.scenario_manager = self._vec.scenario_manager

    def reset(self, seed=None, options=None):
        obs, infos = self._vec.reset(seed, options)
        self._abuf = np.zeros((1, 2), np.float32)
        infos = _first(infos)
        infos["scenario_status"] = ScenarioStatus(int(infos["scenario_status"]))
        infos["traffic_status"] = TrafficStatus(int(infos["traffic_status"]))
        # (what reset hands out must not alias the pinned frame the steps fill: copies, like the step's own results)
        obs = obs.copy()
        infos = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in infos.items()}
        # the step's fast path: everything a step needs of the library and of frame 0, looked up once (one env: the results
        # are copied out of the frame anyway, so every step fills the same pinned frame)
        pool = self.scenario_manager.pool
        fr = pool._frames[0]                  # (built by the reset's frame_fetch: the first frame handed out)
        self._vec._last = fr
        self._fast = (pool._lib.t2d_step_host, pool._h, self._abuf.ctypes.data,
                      None if self._vec._action_box is None else self._vec._action_box.ctypes.data, C.byref(pool._frame_ptr), pool,
                      fr, fr.obs[0], fr.status[0], fr.rel[0], None if fr.lidar is None else fr.lidar[0])
        return obs[0], infos

    def step(self, action):
        """envs/parking.py:219-256: (observation, reward, terminated, truncated, infos) as host values -- one library call
        (t2d_step_host on a zero-copy frame: the kernels read the action from and write the results to mapped host memory).
        `infos["state"]` holds Python floats (the stored fp32 values, exactly), the statuses are the reference's enums."""
        v = self._vec
        if v._scene is None:
            raise RuntimeError("call reset() first")
        a = self._abuf
        if self.continuous:
            try:
                a[0, 0], a[0, 1] = action   # (exactly two scalars: Box.contains checks the shape as well)
            except (ValueError, TypeError):
                raise InvalidAction(f"Action {action} is not in the action space.") from None
        else:
            try:
                a[0] = v._discrete_actions[int(action)]
            except (KeyError, ValueError, TypeError):
                raise InvalidAction(f"Action {action} is not in the action space.") from None
        step_host, h, a_ptr, box_ptr, frame_ref, pool, fr, obs_row, st_row, rel_row, lidar_row = self._fast
        # (`action_space.contains`: checked by the library while it stages the action -- a NaN is outside, like Box.contains)
        rc = step_host(h, a_ptr, box_ptr, 100, None, 0, frame_ref)
        if rc:
            if rc == ERR_ACTION:
                raise InvalidAction(f"Action {action} is not in the action space.")
            pool._ck(rc)
        v.scenario_manager._flags_cache = None
        o = obs_row.copy()
        x, y, heading, speed, vx, vy = o.tolist()
        s0, s1, s2, s3 = st_row.tolist()
        d0, d1, d2 = rel_row.tolist()
        ta, th = (fr.target[0].copy(), float(fr.target_heading[0])) if v._moving_targets else (v._target_area[0], v._target_heading[0])
        infos = {"state": {"x": x, "y": y, "heading": heading, "speed": speed, "vx": vx, "vy": vy, "frame": int(fr.frame_ms[0])},
                 "scenario_status": _SCENARIO[s0], "traffic_status": _TRAFFIC[s1], "target_area": ta, "target_heading": th,
                 "diff_position": d0, "diff_angle": d1, "diff_heading": d2, "iou": float(fr.iou[0]),
                 "lidar": None if lidar_row is None else lidar_row.copy(), "episode": int(fr.episode[0])}
        return o, float(fr.reward[0]), s2 != 0, s3 != 0, infos

    def close(self):
        self._vec.close()


def _first(infos):
    out = {}
    for k, v in infos.items():
        if isinstance(v, dict):
            out[k] = {kk: (vv[0] if vv is not None else None) for kk, vv in v.items()}
        else:
            out[k] = v[0] if isinstance(v, np.ndarray) else v
    return out


def _csr_to_lists(csr):
    eo, vo, xy = csr
    return [[xy[vo[p]:vo[p + 1]] for p in range(eo[e], eo[e + 1])] for e in range(len(eo) - 1)]
