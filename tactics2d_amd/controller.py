"""Host-side mirrors of the reference's IDM, PID, pure-pursuit and acceleration controllers for the batched device path (scope row f3).

Reference: `tactics2d.controller.IDMController` (controller/idm_controller.py:15-157): same
constructor arguments and defaults, `configure(**kwargs)` with the same AttributeError, and `step`
returning `(steering, acceleration)` with steering always 0.0.  Here one controller object is one
parameter set; `install(pool, controllers, ctrl_id)` hands the sets to the device, after which
`pool.step()` computes the controlled participants' accelerations on the GPU before integrating.
There is no CPU path: `step` runs the HIP kernel on a scratch pool.
"""
import numpy as np

from . import layout as L

_PARAMS = ("desired_speed", "time_headway", "min_spacing", "max_acceleration", "comfortable_deceleration", "delta")


class IDMController:
    def __init__(self, desired_speed=10.0, time_headway=1.5, min_spacing=2.0, max_acceleration=1.0,
                 comfortable_deceleration=3.0, delta=4.0, lane_half_width=1.875, horizon=np.inf):
        # reference ctor: idm_controller.py:33-57.  lane_half_width / horizon belong to the
        # build-defined leader rule (include/t2d.h, t2d_set_idm); the reference has no such rule.
        self.desired_speed = desired_speed
        self.time_headway = time_headway
        self.min_spacing = min_spacing
        self.max_acceleration = max_acceleration
        self.comfortable_deceleration = comfortable_deceleration
        self.delta = delta
        self.lane_half_width = lane_half_width
        self.horizon = horizon

    def configure(self, **kwargs):
        """idm_controller.py:143-157; re-install on the pool afterwards."""
        for key, value in kwargs.items():
            if hasattr(self, key):
                setattr(self, key, value)
            else:
                raise AttributeError(f"IDMController has no parameter '{key}'")

    def row(self):
        r = np.zeros(L.IDM_COLS)
        for k, name in enumerate(_PARAMS):
            r[k] = float(getattr(self, name))
        r[L.IDM_LANE_HALF_WIDTH] = float(self.lane_half_width)
        r[L.IDM_HORIZON] = float(self.horizon)
        return r

    def step(self, ego_state, leading_state=None, **kwargs):
        """Batched `IDMController.step(ego_state, leading_state)`: states are `physics.BatchedState`s of
        equal length (leading_state=None: free flow).  Returns (steering[n] zeros, acceleration[n])."""
        from .pool import ParticipantPool
        n = len(np.atleast_1d(ego_state.x))
        two = leading_state is not None
        A = 2 if two else 1
        z = np.zeros(n, np.float32)

        def col(name):
            e = np.asarray(getattr(ego_state, name), np.float32).reshape(n)
            if not two:
                return e
            l = np.asarray(getattr(leading_state, name), np.float32).reshape(n)
            return np.stack([e, l], 1).reshape(-1)

        pool = ParticipantPool(n, A)
        try:
            row = np.zeros((1, L.PARAM_COLS)); row[0, L.P_DELTA_T_MS] = 5.0  # a kinematic dummy type: never integrated
            row[0, L.P_LF] = row[0, L.P_LR] = 1.0; row[0, L.P_WB] = 2.0; row[0, L.P_LENGTH] = 4.0; row[0, L.P_WIDTH] = 2.0
            pool.set_param_table(row)
            hd = col("heading") if getattr(ego_state, "heading", None) is not None else np.zeros(n * A, np.float32)
            pool.reset(col("x"), col("y"), hd, col("speed"), np.zeros(n * A, np.uint8))
            cid = np.full(n * A, L.IDM_NONE, np.uint8); cid[::A] = 0
            pool.set_idm(self.row()[None], cid)
            forced = np.full(n * A, L.IDM_LEADER_FREE, np.int32)
            if two:
                forced[::A] = 1
            pool.upload(L.F_LEADER, forced)           # reuse the field as the device-side leader list
            ptr, _ = pool.field_ptr(L.F_LEADER)
            pool.idm_actions(ptr)
            acc = pool.download(L.F_ACT0)[::A].astype(np.float64)
        finally:
            pool.close()
        return z.astype(np.float64), acc


def install(pool, controllers, ctrl_id):
    """controllers: sequence of IDMController; ctrl_id[n]: index into it or layout.IDM_NONE."""
    rows = np.stack([c.row() for c in controllers]) if len(controllers) else None
    pool.set_idm(rows, ctrl_id)


# ---------------------------------------------------------------------------------------------------- PID (lane keeping)
_PID_PARAMS = ("dt", "kp_lat", "ki_lat", "kd_lat", "max_steering", "kp_lon", "ki_lon", "kd_lon", "max_accel", "min_accel")
_PID_MODES = ("combined", "lateral", "longitudinal")
# update_driving_style: parameter -> (value at style -1, value at style +1), pid_controller.py:120-124
_PID_STYLE = {"kp_lat": (1.0, 2.0), "kp_lon": (1.5, 2.5), "max_steering": (0.4, 0.6), "max_accel": (2.5, 3.5), "min_accel": (-4.0, -6.0)}
_LATERAL = {"cross_track": L.PID_LAT_CROSS_TRACK, "heading": L.PID_LAT_HEADING}
_LONGITUDINAL = {"pid": L.PID_LON_SPEED, "idm": L.PID_LON_IDM, "caller": L.PID_LON_CALLER}


def _pid_check(dt=None, control_mode=None, max_steering=None, max_accel=None, min_accel=None, derivative_filter_alpha=None):
    """the constructor's refusals (pid_controller.py:82-102), comparison by comparison; None = not given"""
    if control_mode is not None and control_mode not in _PID_MODES:
        raise ValueError(f"control_mode: one of {_PID_MODES} expected, not {control_mode!r}")
    if dt is not None and dt <= 0:
        raise ValueError(f"dt = {dt}: a positive time step expected")
    if max_steering is not None and max_steering <= 0:
        raise ValueError(f"max_steering = {max_steering}: a positive angle expected")
    if max_accel is not None and max_accel <= 0:
        raise ValueError(f"max_accel = {max_accel}: a positive acceleration expected")
    if min_accel is not None and min_accel >= 0:
        raise ValueError(f"min_accel = {min_accel}: a negative acceleration (a deceleration) expected")
    if max_accel is not None and min_accel is not None and max_accel <= min_accel:
        raise ValueError(f"max_accel = {max_accel} does not exceed min_accel = {min_accel}")
    if derivative_filter_alpha is not None and (derivative_filter_alpha <= 0 or derivative_filter_alpha > 1):
        raise ValueError(f"derivative_filter_alpha = {derivative_filter_alpha} outside (0, 1]")


def pid_term(error, state, kp, ki, kd, dt, alpha, limits=None):
    """`PIDController._compute_pid` (pid_controller.py:159-234) on float64 scalars, one rounding per operation: returns
    (output, (integral, prev_error, prev_derivative), saturated).  state = (integral, prev_error, prev_derivative)."""
    f = np.float64
    error, (integral, prev_error, prev_der) = f(error), (f(v) for v in state)
    kp, ki, kd, dt, alpha = f(kp), f(ki), f(kd), f(dt), f(alpha)
    with np.errstate(all="ignore"):
        raw = (error - prev_error) / dt if dt > 0 else f(0.0)
        der = alpha * raw + (f(1.0) - alpha) * prev_der
        out = kp * error + kd * der
        saturated = False
        if limits is not None:
            lo, hi = f(limits[0]), f(limits[1])
            if out > hi:
                saturated, out = True, hi
            elif out < lo:
                saturated, out = True, lo
        integral = integral * f(0.99) if saturated else integral + error * dt
        out = out + ki * integral
        if limits is not None:
            out = np.clip(out, lo, hi)
    return f(out), (f(integral), error, f(der)), saturated


class PIDController:
    """`tactics2d.controller.PIDController` (controller/pid_controller.py:15-470): the same constructor arguments, defaults and
    refusals, `step`, `reset`, `configure` and `update_driving_style`.  One object is one parameter set of the device path
    (`row()`, `install_pid`); its own `step` evaluates the restated law in numpy on the host, one participant at a time, with
    the reference's calling convention (the caller supplies target_heading / cross_track_error / target_speed / wheel_base).

    Build columns of the device row (include/t2d.h, t2d_set_pid): `lateral` = "cross_track" or "heading" says which error the
    kernel measures against the installed route when the control mode has a lateral side; `longitudinal` = "pid" (the
    reference's), "idm" (the IDM law with the leader rule of t2d_idm_actions) or "caller" (the acceleration of the caller's
    row); `wheel_base` = the kwarg of `step` (None: lf + lr of the participant's type)."""

    def __init__(self, dt=0.05, control_mode="combined", kp_lat=1.5, ki_lat=0.2, kd_lat=0.5, max_steering=0.5, kp_lon=2.0,
                 ki_lon=0.3, kd_lon=0.4, max_accel=3.0, min_accel=-5.0, derivative_filter_alpha=0.1, lateral="cross_track",
                 longitudinal="pid", wheel_base=None):
        _pid_check(dt, control_mode, max_steering, max_accel, min_accel, derivative_filter_alpha)
        if lateral not in _LATERAL or longitudinal not in _LONGITUDINAL:
            raise ValueError(f"lateral: one of {sorted(_LATERAL)}, longitudinal: one of {sorted(_LONGITUDINAL)}")
        self.dt, self.control_mode = dt, control_mode
        self.kp_lat, self.ki_lat, self.kd_lat, self.max_steering = kp_lat, ki_lat, kd_lat, max_steering
        self.kp_lon, self.ki_lon, self.kd_lon, self.max_accel, self.min_accel = kp_lon, ki_lon, kd_lon, max_accel, min_accel
        self._derivative_filter_alpha = derivative_filter_alpha
        self.lateral, self.longitudinal, self.wheel_base = lateral, longitudinal, wheel_base
        self.reset()

    def reset(self):
        self._lat = (np.float64(0.0),) * 3   # integral, prev_error, prev_derivative
        self._lon = (np.float64(0.0),) * 3

    @property
    def state(self):
        """the six state words in the order of t2d_pid_state"""
        return np.array(self._lat + self._lon, np.float64)

    @state.setter
    def state(self, words):
        w = [np.float64(v) for v in words]
        self._lat, self._lon = tuple(w[:3]), tuple(w[3:6])

    def update_driving_style(self, style_id):
        """pid_controller.py:136-157: kp_lat, kp_lon, max_steering, max_accel and min_accel by the reference's interpolator --
        linear between style -1 and +1, the end values beyond (controller_base.py:69-91).  Re-install on the pool afterwards."""
        if not isinstance(style_id, (int, float)):
            raise TypeError("style_id: an int or a float expected")
        s = np.float64(style_id)
        for name, (left, right) in _PID_STYLE.items():
            left, right = np.float64(left), np.float64(right)
            if s < -1.0:
                v = left
            elif s > 1.0:
                v = right
            else:   # (slope * (x - x_left) + y_left: the order of scipy's linear interp1d)
                v = (right - left) / np.float64(2.0) * (s - np.float64(-1.0)) + left
            setattr(self, name, float(v))

    def configure(self, **kwargs):
        """pid_controller.py:420-470: every value is checked before any is applied; re-install on the pool afterwards."""
        names = set(_PID_PARAMS) | {"control_mode", "derivative_filter_alpha"}
        for key in kwargs:
            if key not in names:
                raise AttributeError(f"PIDController has no parameter '{key}'")
        _pid_check(**{k: kwargs[k] for k in ("dt", "control_mode", "max_steering", "max_accel", "min_accel",
                                              "derivative_filter_alpha") if k in kwargs})
        for key, value in kwargs.items():
            setattr(self, "_derivative_filter_alpha" if key == "derivative_filter_alpha" else key, value)

    def modes(self):
        """(lat_mode, lon_mode) of the device row"""
        lat = _LATERAL[self.lateral] if self.control_mode in ("combined", "lateral") else L.PID_LAT_NONE
        lon = _LONGITUDINAL[self.longitudinal] if self.control_mode in ("combined", "longitudinal") else L.PID_LON_ZERO
        return lat, lon

    def row(self):
        r = np.zeros(L.PID_COLS)
        for k, name in enumerate(_PID_PARAMS):
            r[k] = float(getattr(self, name))
        r[L.PID_ALPHA] = float(self._derivative_filter_alpha)
        r[L.PID_LAT_MODE], r[L.PID_LON_MODE] = self.modes()
        r[L.PID_WHEEL_BASE] = np.nan if self.wheel_base is None else float(self.wheel_base)
        return r

    def step(self, ego_state, **kwargs):
        """`PIDController.step(ego_state, **kwargs)` (:309-406) for one participant on the host: (steering, acceleration)."""
        num = (int, float)
        steering = acceleration = 0.0
        if self.control_mode in ("combined", "lateral"):
            try:
                if "target_heading" in kwargs:
                    if not isinstance(kwargs["target_heading"], num):
                        raise TypeError("target_heading: a number expected")
                    e = np.float64(kwargs["target_heading"]) - np.float64(ego_state.heading)
                    err = np.float64(np.arctan2(np.sin(e), np.cos(e)))
                elif "cross_track_error" in kwargs:
                    if not isinstance(kwargs["cross_track_error"], num):
                        raise TypeError("cross_track_error: a number expected")
                    err = np.float64(kwargs["cross_track_error"])
                else:
                    raise ValueError("the lateral side needs target_heading or cross_track_error")
                out, self._lat, _ = pid_term(err, self._lat, self.kp_lat, self.ki_lat, self.kd_lat, self.dt,
                                             self._derivative_filter_alpha)
                if "cross_track_error" in kwargs:
                    wb = kwargs.get("wheel_base", 2.637)
                    if wb <= 0:
                        raise ValueError(f"wheel_base = {wb}: a positive length expected")
                    out = out * (np.float64(2.0) / np.float64(wb))
                steering = np.clip(out, -np.float64(self.max_steering), np.float64(self.max_steering))
            except (ValueError, TypeError):
                if self.control_mode == "lateral":
                    raise
                steering = 0.0
        if self.control_mode in ("combined", "longitudinal"):
            try:
                if "target_speed" not in kwargs:
                    raise ValueError("the longitudinal side needs target_speed")
                if not isinstance(kwargs["target_speed"], num):
                    raise TypeError("target_speed: a number expected")
                speed = ego_state.speed if ego_state.speed is not None else 0.0
                lim = (self.min_accel, self.max_accel)
                out, self._lon, _ = pid_term(np.float64(kwargs["target_speed"]) - np.float64(speed), self._lon, self.kp_lon,
                                             self.ki_lon, self.kd_lon, self.dt, self._derivative_filter_alpha, lim)
                acceleration = np.clip(out, np.float64(lim[0]), np.float64(lim[1]))
            except (ValueError, TypeError):
                if self.control_mode == "longitudinal":
                    raise
                acceleration = 0.0
        return steering, acceleration


def install_pid(pool, controllers, ctrl_id, target_speed=0.0, idm=None):
    """controllers: sequence of PIDController; ctrl_id[n]: index into it or layout.PID_NONE; target_speed[n] (a scalar
    broadcasts); idm[n]: for participants whose controller has longitudinal="idm", the row of the IDM parameter sets installed
    with `install` / pool.set_idm (None: row 0).  An empty sequence uninstalls."""
    rows = np.stack([c.row() for c in controllers]) if len(controllers) else None
    pool.set_pid(rows, ctrl_id, target_speed, idm)


PID_EVENTS = ("route_end", "nonfinite", "reset", "no_route", "bad_wheel_base", "saturated")   # bit k: layout.PID_*


class _ActionWriter:
    """What LaneKeeper, PathFollower and planner.RSFollower share: one launch per call that writes one (steering, accel) row and
    one record per row of the action tensor, into lazily made buffers of the object's own unless the caller brings the rows.
    A subclass names its records (their size in bytes, the ParticipantPool method that views them, whether there is one row
    per participant or per env) and passes its launch to _write / _reset."""
    _record_bytes = _records = None
    _n_rows = "n"   # the pool attribute that counts the rows: "n" (participants) or "n_env"

    def __init__(self, pool):
        self.pool = pool
        self._rec = self._views = self._act = None

    def _stream(self, stream):
        import torch
        return stream if stream is not None else torch.cuda.current_stream(torch.device("cuda", self.pool.device_id))

    def _write(self, launch, actions, out, stream):
        """launch(act_in_ptr, act_out_ptr, record_ptr, stream handle) -> dict(the record views, action_rows=the rows written)"""
        import torch
        n, st = getattr(self.pool, self._n_rows), self._stream(stream)
        for t in (actions, out):
            if t is not None and (t.dtype != torch.float32 or tuple(t.shape) != (n, 2) or not t.is_contiguous()):
                raise ValueError(f"action rows must be a contiguous float32 [{n}, 2] tensor")
        if self._rec is None:
            self._rec = torch.zeros((n, self._record_bytes // 8), dtype=torch.float64, device=st.device)
            self._views = getattr(self.pool, self._records)(self._rec.data_ptr(), owner=self._rec)
            self._act = torch.zeros((n, 2), dtype=torch.float32, device=st.device)
        rows = self._act if out is None else out
        launch(None if actions is None else actions.data_ptr(), rows.data_ptr(), self._rec.data_ptr(), st.cuda_stream)
        return dict(self._views, action_rows=rows)

    def _reset(self, launch, mask, stream):
        """launch(mask_ptr, stream handle) with `mask` as uint8 [n_env] (None: every env)"""
        import torch
        st = self._stream(stream)
        if mask is not None:
            mask = mask.to(torch.uint8).contiguous()
            if tuple(mask.shape) != (self.pool.n_env,):
                raise ValueError(f"mask must have {self.pool.n_env} elements")
            self._mask = mask   # (kept alive until the launch has run)
        launch(None if mask is None else mask.data_ptr(), st.cuda_stream)


class LaneKeeper(_ActionWriter):
    """The controllers installed on `pool` (install_pid) in a step_torch-style loop: follow() writes the action rows to step
    with -- bind them with pool.bind_actions(rows + 4 bytes, rows, stride=2) -- and returns zero-copy torch views of the
    records (ParticipantPool.pid_records) beside them."""

    _record_bytes, _records = L.PID_RECORD_BYTES, "pid_records"

    def follow(self, actions=None, out=None, stream=None):
        """actions: float32 CUDA tensor [n, 2] (steering, accel), the rows of whoever else acts (None: zeros), never written
        unless it is also `out`; out: float32 [n, 2] tensor for the rows to step (None: a buffer of the keeper's own).
        Asynchronous on `stream`.  Returns dict(action_rows, cross_track, lat_error, segment, leader, events, action), valid until
        the next follow()."""
        return self._write(self.pool.pid_actions, actions, out, stream)

    def reset(self, mask=None, stream=None):
        """controller.reset() for the envs where `mask` (a uint8 / bool CUDA tensor [n_env]) is non-zero; None: every env"""
        self._reset(self.pool.pid_reset, mask, stream)


# ---------------------------------------------------------------------------------------------------- pure pursuit, cruise / ACC
_PURSUIT_LON = {"cruise": L.PURSUIT_LON_CRUISE, "acc": L.PURSUIT_LON_ACC, "caller": L.PURSUIT_LON_CALLER}
# update_driving_style: parameter -> (value at style -1, value at style +1), acceleration_controller.py:50-55
_ACCEL_STYLE = {"kp": (4.5, 2.5), "speed_factor": (0.8, 1.2), "accel_change_rate": (3.0, 6.0), "max_accel": (1.5, 2.5),
                "min_accel": (-3.0, -5.0), "interval": (3.5, 1.5)}


def _style_value(style_id, left, right):
    """the reference's style interpolator (controller_base.py:69-91): linear between style -1 and +1, the end values beyond"""
    s, left, right = np.float64(style_id), np.float64(left), np.float64(right)
    if s < -1.0:
        return float(left)
    if s > 1.0:
        return float(right)
    return float((right - left) / np.float64(2.0) * (s - np.float64(-1.0)) + left)   # (the order of scipy's linear interp1d)


def _configure(obj, kwargs):
    """ControllerBase.configure (controller_base.py:52-67)"""
    for key, value in kwargs.items():
        if hasattr(obj, key):
            setattr(obj, key, value)
        else:
            raise AttributeError(f"Controller {type(obj).__name__} has no parameter '{key}'")


def interpolate(line, distance):
    """The point `distance` along a polyline from its START, float64 (x, y): what `LineString.interpolate` is asked for by the
    reference (pure_pursuit_controller.py:94), computed as the device's walk computes it (include/t2d.h) -- per segment
    L = sqrt(vx * vx + vy * vy), the target is cur + v * (distance_left / L) on the first segment with distance_left <= L and
    L > 0, the last vertex beyond the line's end.  `line`: anything traffic.as_polyline accepts."""
    from .traffic import as_polyline
    pts = as_polyline(line).astype(np.float64)
    rem = np.float64(distance)
    cur = pts[0]
    with np.errstate(all="ignore"):
        for k in range(1, len(pts)):
            v = pts[k] - cur
            seg = np.sqrt(v[0] * v[0] + v[1] * v[1])
            if rem <= seg and seg > 0.0:
                return cur + v * (rem / seg)
            rem = rem - seg
            cur = pts[k]
    return cur


class AccelerationController:
    """`tactics2d.controller.AccelerationController` (controller/acceleration_controller.py:14-145): the same constructor,
    attributes, class defaults and refusals, `update_driving_style`, `configure` and `step` (cruise, or adaptive cruise behind
    `front_state`); `step` evaluates the law in numpy on the host.  One object is one parameter set of the device path (`row()`,
    `install_pursuit`).  `lane_half_width` and `horizon` are the build's leader rule for longitudinal="acc" (t2d_set_idm's)."""
    kp = 3.5
    speed_factor = 1.0   # set by update_driving_style and never read, as in the reference
    accel_change_rate = 3.0
    max_accel = 1.5
    min_accel = -4.0
    interval = 2.0
    delta_t = 0.05
    lane_half_width = 1.875
    horizon = np.inf
    DEFAULT_SAFETY_DISTANCE = 5.0
    MIN_TARGET_DISTANCE = 7.0
    MAX_TARGET_DISTANCE = 80.0

    def __init__(self, target_speed=5.0):
        if target_speed < 0:
            raise ValueError("target_speed must be non-negative")
        self.target_speed = target_speed

    def update_driving_style(self, style_id):
        if not isinstance(style_id, (int, float)):
            raise TypeError("style_id must be int or float")
        for name, (left, right) in _ACCEL_STYLE.items():
            setattr(self, name, _style_value(style_id, left, right))

    def configure(self, **kwargs):
        _configure(self, kwargs)

    def _clips(self, accel, accel_last):
        f = np.float64
        step = f(self.accel_change_rate) * f(self.delta_t)
        accel = np.clip(accel, f(accel_last) - step, f(accel_last) + step)
        return np.clip(accel, f(self.min_accel), f(self.max_accel))

    def _cruise_control(self, ego_state):
        f = np.float64
        with np.errstate(all="ignore"):
            return self._clips((f(self.target_speed) - f(ego_state.speed)) / f(self.kp), ego_state.accel)

    def _adaptive_cruise_control(self, ego_state, front_state):
        f = np.float64
        with np.errstate(all="ignore"):
            distance_front = np.hypot(f(ego_state.x) - f(front_state.x), f(ego_state.y) - f(front_state.y))
            distance_target = np.clip(f(ego_state.speed) * f(self.interval) + f(self.DEFAULT_SAFETY_DISTANCE),
                                      f(self.MIN_TARGET_DISTANCE), f(self.MAX_TARGET_DISTANCE))
            relative_speed = f(front_state.speed) - f(ego_state.speed)
            relative_target_speed = (distance_target - distance_front) / f(self.kp)
            relative_accel = (relative_target_speed - relative_speed) / f(self.kp)
            return self._clips(f(front_state.accel) - relative_accel, ego_state.accel)

    def step(self, ego_state, **kwargs):
        """(0.0, acceleration): adaptive cruise behind kwargs["front_state"] when given, cruise otherwise (:126-145).  The
        reference raises TypeError for a front_state that is no `State`; this package has no State class, so the refusal is for
        whatever lacks a state's x, y, speed and accel."""
        front_state = kwargs.get("front_state")
        if front_state is not None:
            if not all(hasattr(front_state, k) for k in ("x", "y", "speed", "accel")):
                raise TypeError("front_state must be a state with x, y, speed and accel")
            return 0.0, self._adaptive_cruise_control(ego_state, front_state)
        return 0.0, self._cruise_control(ego_state)

    def row(self, longitudinal="cruise"):
        r = np.zeros(L.PURSUIT_COLS)
        r[L.PURSUIT_MIN_PRE_AIMING], r[L.PURSUIT_INTERVAL_LAT] = 10.0, 1.0   # (unread with lat_mode 0)
        self._fill(r, longitudinal)
        r[L.PURSUIT_WHEEL_BASE] = np.nan
        return r

    def _fill(self, r, longitudinal):
        if longitudinal not in _PURSUIT_LON:
            raise ValueError(f"longitudinal: one of {sorted(_PURSUIT_LON)}")
        for col, name in ((L.PURSUIT_KP, "kp"), (L.PURSUIT_ACCEL_CHANGE_RATE, "accel_change_rate"), (L.PURSUIT_MAX_ACCEL, "max_accel"),
                          (L.PURSUIT_MIN_ACCEL, "min_accel"), (L.PURSUIT_INTERVAL_LON, "interval"), (L.PURSUIT_DELTA_T, "delta_t"),
                          (L.PURSUIT_LANE_HALF_WIDTH, "lane_half_width"), (L.PURSUIT_HORIZON, "horizon")):
            r[col] = float(getattr(self, name))
        r[L.PURSUIT_LON_MODE] = _PURSUIT_LON[longitudinal]


class PurePursuitController:
    """`tactics2d.controller.PurePursuitController` (controller/pure_pursuit_controller.py:16-98): the same constructor, class
    default, refusals, `update_driving_style` (forwarded to its longitudinal AccelerationController), `configure` and `step`.
    The host `step` interpolates the look-ahead point from the START of `waypoints`, as the reference does (there is no shapely:
    `interpolate` above); the device path walks from the participant's projection onto its installed route (include/t2d.h).
    `wheel_base` (None: lf + lr of the participant's type) is the build column of the device row."""
    interval = 1.0
    wheel_base = None

    def __init__(self, min_pre_aiming_distance=10.0, target_speed=5.0):
        if min_pre_aiming_distance <= 0:
            raise ValueError("min_pre_aiming_distance must be positive")
        if target_speed < 0:
            raise ValueError("target_speed must be non-negative")
        self.min_pre_aiming_distance = min_pre_aiming_distance
        self._longitudinal_control = AccelerationController(target_speed)

    @property
    def target_speed(self):
        return self._longitudinal_control.target_speed

    def update_driving_style(self, style_id):
        if not isinstance(style_id, (int, float)):
            raise TypeError("style_id must be int or float")
        self._longitudinal_control.update_driving_style(style_id)
        self.interval = _style_value(style_id, 2.0, 1.0)

    def configure(self, **kwargs):
        _configure(self, kwargs)

    def _lateral_control(self, ego_state, pre_aiming_point, wheel_base):
        """pre_aiming_point: (x, y) or an object with .x / .y"""
        f = np.float64
        px, py = (pre_aiming_point.x, pre_aiming_point.y) if hasattr(pre_aiming_point, "x") else pre_aiming_point
        with np.errstate(all="ignore"):
            dy, dx = f(py) - f(ego_state.y), f(px) - f(ego_state.x)
            pre_aiming_angle = np.arctan2(dy, dx)
            distance = np.linalg.norm((dy, dx))
            return np.arctan(f(2.0) * f(wheel_base) * np.sin(pre_aiming_angle - f(ego_state.heading)) / distance)

    def pre_aiming_distance(self, speed):
        return np.max([np.float64(speed) * np.float64(self.interval), np.float64(self.min_pre_aiming_distance)])

    def step(self, ego_state, waypoints, wheel_base=2.637, front_state=None, **kwargs):
        """(steering, acceleration) (:76-98); waypoints: anything traffic.as_polyline accepts; front_state (the one keyword the
        reference's **kwargs carries on to the longitudinal controller): adaptive cruise behind it, TypeError if it is no state"""
        point = interpolate(waypoints, self.pre_aiming_distance(ego_state.speed))
        _, accel = self._longitudinal_control.step(ego_state, front_state=front_state, **kwargs)
        return self._lateral_control(ego_state, point, wheel_base), accel

    def row(self, longitudinal="cruise"):
        r = np.zeros(L.PURSUIT_COLS)
        r[L.PURSUIT_MIN_PRE_AIMING], r[L.PURSUIT_INTERVAL_LAT] = float(self.min_pre_aiming_distance), float(self.interval)
        self._longitudinal_control._fill(r, longitudinal)
        r[L.PURSUIT_LAT_MODE] = L.PURSUIT_LAT_PURE_PURSUIT
        r[L.PURSUIT_WHEEL_BASE] = np.nan if self.wheel_base is None else float(self.wheel_base)
        return r


def install_pursuit(pool, controllers, ctrl_id, target_speed=None, longitudinal="cruise"):
    """controllers: sequence of PurePursuitController / AccelerationController; ctrl_id[n]: index into it or layout.PURSUIT_NONE;
    target_speed[n] (a scalar broadcasts; None: each controller's own target_speed); longitudinal: "cruise", "acc" (adaptive
    cruise behind the leader of t2d_idm_actions' rule, cruise without one) or "caller" (the acceleration of the caller's row).
    An empty sequence uninstalls."""
    if not len(controllers):
        pool.set_pursuit(None)
        return
    rows = np.stack([c.row(longitudinal) for c in controllers])
    cid = np.asarray(ctrl_id, np.uint8).reshape(-1)
    if target_speed is None:
        own = np.float32([c.target_speed for c in controllers] + [0.0])
        target_speed = own[np.where(cid == L.PURSUIT_NONE, len(controllers), np.minimum(cid, len(controllers)))]
    pool.set_pursuit(rows, cid, target_speed)


PURSUIT_EVENTS = ("route_end", "nonfinite", "wrapped", "no_route", "no_leader")   # bit k: layout.PURSUIT_*


class PathFollower(_ActionWriter):
    """The controllers installed on `pool` (install_pursuit) in a step_torch-style loop: LaneKeeper's contract without reset()
    -- the controllers hold no state.  follow() writes the action rows to step with -- bind them with
    pool.bind_actions(rows + 4 bytes, rows, stride=2) -- and returns zero-copy torch views of the records
    (ParticipantPool.pursuit_records) beside them."""

    _record_bytes, _records = L.PURSUIT_RECORD_BYTES, "pursuit_records"

    def follow(self, actions=None, out=None, stream=None):
        """actions: float32 CUDA tensor [n, 2] (steering, accel), the rows of whoever else acts (None: zeros), never written
        unless it is also `out`; out: float32 [n, 2] tensor for the rows to step (None: a buffer of the follower's own).
        Asynchronous on `stream`.  Returns dict(action_rows, point, pre_aiming_distance, distance, cross_track, segment,
        target_segment, leader, events, action), valid until the next follow()."""
        return self._write(self.pool.pursuit_actions, actions, out, stream)
