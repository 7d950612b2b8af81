"""ParticipantPool -- thin, typed Python face of one t2d_pool handle (include/t2d.h).

Host logic only: argument marshalling and error translation.  All compute happens in the
HIP kernels behind libt2d_hip.so.
"""
import contextlib
import ctypes as C
import sys

import numpy as np

from . import _ffi, layout as L


def _arr(a, dtype, n=None, name="array"):
    if a is None:
        return None
    out = np.ascontiguousarray(a, dtype=dtype)
    if n is not None and out.size != n:
        raise ValueError(f"{name}: expected {n} elements, got {out.size}")
    return out


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def pack_track_mask(visited):
    """bool [n_env, <= MAX_TRACK_TILES] -> uint32 [n_env, TRACK_MASK_WORDS]: bit t % 32 of word t // 32 = tile t"""
    v = np.asarray(visited, bool)
    if v.ndim != 2 or v.shape[1] > L.MAX_TRACK_TILES:
        raise ValueError(f"visited: bool [n_env, <= {L.MAX_TRACK_TILES}]")
    full = np.zeros((v.shape[0], L.MAX_TRACK_TILES), bool)
    full[:, :v.shape[1]] = v
    return np.ascontiguousarray(np.packbits(full, axis=1, bitorder="little")).view("<u4")


def unpack_track_mask(mask, n_tile=None):
    """uint32 [n_env, TRACK_MASK_WORDS] -> bool [n_env, n_tile or MAX_TRACK_TILES]"""
    m = np.ascontiguousarray(mask, "<u4")
    return np.unpackbits(m.view(np.uint8), axis=1, bitorder="little")[:, :n_tile].astype(bool)


class _DevArray:
    """Zero-copy view of a pool field for `torch.as_tensor(..., device='cuda')`."""

    def __init__(self, ptr, shape, typestr, owner):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False),
                                         "version": 2, "strides": None}
        self._owner = owner


class HostFrame:
    """numpy views of one host frame of t2d_step_host (include/t2d.h): what ParkingEnv.step hands its caller, for the ego of
    every env.  `copy()` returns a frame that owns its memory; `in_use()` tells whether anything outside this object still
    holds a view of the frame (so that the pinned frame can be handed out again without a copy)."""
    _SECTIONS = (("rel", "off_rel", np.float64, 3), ("obs", "off_obs", np.float32, 6), ("reward", "off_reward", np.float32, 0),
                 ("status", "off_status", np.uint8, 4), ("iou", "off_iou", np.float32, 0),
                 ("frame_ms", "off_frame_ms", np.int32, 0), ("cnt_step", "off_cnt_step", np.int32, 0),
                 ("episode", "off_episode", np.int32, 0), ("target_heading", "off_target_heading", np.float64, 0),
                 ("target", "off_target", np.float32, 8), ("lidar", "off_lidar", np.float32, -1))

    def __init__(self, base, lay):
        """base: uint8 array holding the frame (or its front part up to the lidar section)."""
        self.base, self.lay = base, lay
        n = lay.n_env
        self.header = base[:64].view(np.uint32)
        for name, off_name, dt, cols in self._SECTIONS:
            off = getattr(lay, off_name)
            cols = lay.n_beams if cols < 0 else cols
            nb = n * max(cols, 1) * np.dtype(dt).itemsize
            if off < 0 or off + nb > base.size:
                setattr(self, name, None)
                continue
            v = base[off:off + nb].view(dt)
            setattr(self, name, v.reshape(n, 4, 2) if name == "target" else v.reshape(n, cols) if cols else v)
        st = self.status
        self.terminated, self.truncated = st[:, 2].view(np.bool_), st[:, 3].view(np.bool_)
        del st, v
        # everything a caller can get hold of is one of these objects or a view whose .base is one of them (numpy collapses
        # the base chain of a view to the array that exposes the memory): their reference counts tell whether the frame is held
        self._tracked = [self.base] + [v for v in self.__dict__.values() if isinstance(v, np.ndarray) and v is not self.base]
        self._idle_refs = None   # set by calibrate(); until then the frame counts as in use (the safe answer)

    def calibrate(self):
        """Record the reference counts of the frame's arrays in the IDLE state -- call once, right after construction, when
        nothing outside this object holds a view yet (ParticipantPool._frame does).  Measured, not derived: whatever
        temporaries the interpreter keeps while counting are the same then and later."""
        self._idle_refs = self._refs()
        return self

    def _refs(self):
        # the object itself counts too: a caller that keeps the HostFrame (`frames.append(mgr.step_host(a))`) holds no array
        # reference, and must pin the frame all the same.  (calibrate() and in_use() are both called through one local name
        # beside whatever container owns the frame -- ParticipantPool._frame / _pick_frame keep it that way.)
        return [sys.getrefcount(self)] + [sys.getrefcount(v) for v in self._tracked]

    def in_use(self):
        return self._idle_refs is None or self._refs() != self._idle_refs

    def copy(self, lidar=True):
        """A frame that owns its memory (one memcpy); lidar=False leaves the lidar section out (its views become None)."""
        end = self.lay.bytes if lidar or self.lay.off_lidar < 0 else self.lay.off_lidar
        return HostFrame(self.base[:end].copy(), self.lay)


class OccupancyGrids:
    """What ParticipantPool.occupancy_grid returns: device tensors, one row per env.  weight float64 [n_env, H, W] (free_weight
    or +inf), mask uint8 [n_env, H, W] (1 = occupied), hw int32 [n_env, 2], status int32 [n_env]; cell_size and origin are the
    window's (planner_kwargs(): what the planners of `search` take beside the weights)."""

    def __init__(self, weight, mask, hw, status, cell_size, origin):
        self.weight, self.mask, self.hw, self.status, self.cell_size, self.origin = weight, mask, hw, status, cell_size, origin

    def planner_kwargs(self):
        return dict(cell_size=self.cell_size, origin=self.origin)


class ParticipantPool:
    """n_env environments x max_agents participants resident on one MI355X."""

    def __init__(self, n_env, max_agents=1, device_id=0, library=None):
        """library: the loaded C library the pool lives in -- libt2d_hip.so unless a test / measurement asks for the hooks of
        libt2d_hip_debug.so (tactics2d_amd.debug.pool)."""
        self._lib = library if library is not None else _ffi.lib()
        self._h = C.c_void_p()
        self.n_env, self.max_agents = int(n_env), int(max_agents)
        self.n = self.n_env * self.max_agents
        self.device_id = int(device_id)
        # the installed racing tracks: tiles of each env's ring; whether they were generated on the device, and each env's set then
        self.track_n_tile, self._tracks_generated, self.track_n_tile_set = None, False, None
        _ffi.check(self._lib.t2d_create(self.n_env, self.max_agents, self.device_id, C.byref(self._h)), None, self._lib)

    # ---------------------------------------------------------------- lifetime
    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            self.replay_unbind()
            self.clear_routes()
            for user in list(self.__dict__.get("_replay_users", ())):   # (pools that replay a trajectory of this one let go of it)
                user.replay_unbind()
            for user in list(self.__dict__.get("_route_users", ())):    # (... or take their routes from one)
                user.clear_routes()
            for buf in list(self.__dict__.get("_traj_buffers", ())):   # (DeviceTrajectory buffers bound to this pool go first)
                buf.close()
            self._lib.t2d_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc):
        _ffi.check(rc, self._h, self._lib)

    # ---------------------------------------------------------------- configuration
    def set_param_table(self, rows):
        rows = np.ascontiguousarray(rows, np.float64)
        if rows.ndim != 2 or rows.shape[1] < L.PARAM_COLS:
            raise ValueError("rows must be (n_types, >=24) float64")
        self._ck(self._lib.t2d_set_param_table(self._h, _p(rows), rows.shape[0], rows.shape[1]))
        self.n_types = rows.shape[0]

    @staticmethod
    def _csr(t, n_env):
        if t is None:
            return None, None, None
        eo, vo, xy = t
        eo = _arr(eo, np.int32, n_env + 1, "env offsets")
        vo = _arr(vo, np.int32, None, "vertex offsets")
        xy = _arr(xy, np.float32, None, "verts_xy")
        if vo.size != eo[-1] + 1:
            raise ValueError("vertex offsets must have n_poly + 1 entries")
        if xy.size != 2 * (vo[-1] if vo.size else 0):
            raise ValueError("verts_xy must have 2 * n_vert entries")
        return eo, vo, xy

    def set_static_geometry(self, static=None, boundary=None, boundary_valid=None):
        """static: (env_poly_offsets[E+1], poly_vert_offsets[P+1], verts_xy[V,2]) or None;
        boundary: (E,4) xmin,xmax,ymin,ymax or None."""
        eo, vo, xy = self._csr(static, self.n_env)
        b = _arr(boundary, np.float32, 4 * self.n_env, "boundary")
        bv = _arr(boundary_valid, np.uint8, self.n_env, "boundary_valid")
        self._ck(self._lib.t2d_set_static_geometry(self._h, _p(eo), _p(vo), _p(xy), _p(b), _p(bv)))

    def set_lane_geometry(self, lanes=None):
        eo, vo, xy = self._csr(lanes, self.n_env)
        self._ck(self._lib.t2d_set_lane_geometry(self._h, _p(eo), _p(vo), _p(xy)))

    def set_status_config(self, **kw):
        cfg = _ffi.StatusConfig(20000, 0, 0, 0, -5.0, -1.0, -5.0, 5.0, 0.001, 0, 0, 100, 0, 0.95, 0.999, 0.1)
        for k, v in kw.items():
            if not hasattr(cfg, k):
                raise TypeError(f"unknown status option {k}")
            setattr(cfg, k, v)
        self._ck(self._lib.t2d_set_status_config(self._h, C.byref(cfg)))
        self.status_config = cfg

    def set_target_areas(self, target_xy=None, centroid=None):
        """target_xy: (n_env, 4, 2) quads or None; centroid: (n_env, 2) or None (computed)."""
        t = _arr(target_xy, np.float32, 8 * self.n_env, "target_xy")
        c = _arr(centroid, np.float32, 2 * self.n_env, "centroid")
        self._ck(self._lib.t2d_set_target_areas(self._h, _p(t), _p(c)))

    def lidar_config(self, n_beams=360, max_range=20.0, include_participants=False, subsample_of=None):
        """SingleLineLidar of every ego; beam tables come from numpy like the reference's linspace/sin/cos.
        subsample_of = N: the n_beams beams are every (N / n_beams)-th beam of the N-beam scan -- the SAME angles, so the scan
        equals `full_scan[:, ::N // n_beams]` bit for bit (what the tutorial policy keeps of ParkingEnv's 360 beams)."""
        if subsample_of is None:
            th = np.linspace(0, 2 * np.pi, int(n_beams), endpoint=False)
        else:
            if int(subsample_of) % int(n_beams):
                raise ValueError(f"{n_beams} beams are not a regular subset of {subsample_of}")
            th = np.linspace(0, 2 * np.pi, int(subsample_of), endpoint=False)[::int(subsample_of) // int(n_beams)]
        bs, bc = np.ascontiguousarray(np.sin(th)), np.ascontiguousarray(np.cos(th))
        self._ck(self._lib.t2d_lidar_config(self._h, int(n_beams), float(max_range), int(bool(include_participants)),
                                            _p(bs), _p(bc)))
        self.n_beams = int(n_beams)

    def lidar_scan(self, out_ptr=None, stream=None):
        self._ck(self._lib.t2d_lidar_scan(self._h, out_ptr, stream))

    def lidar_scan_all(self, out_ptr=None, stream=None):
        """The scan of lidar_config with EVERY participant of every env as the sensor, in one launch: float32
        [n_env, max_agents, n_beams] (+inf = no return; rows of inactive participants are all +inf) written to the device
        memory at out_ptr, or -- out_ptr None -- to a buffer of the pool's own (lidar_all(), lidar_all_buffer()).
        Asynchronous on `stream`; status_config.ego_index plays no part."""
        self._ck(self._lib.t2d_lidar_scan_all(self._h, out_ptr, stream))

    def lidar_all_buffer(self):
        """(device pointer, bytes) of the pool's own all-participants scan buffer (after a lidar_scan_all() into it)."""
        ptr, nb = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.t2d_lidar_all_buffer(self._h, C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def lidar_all(self):
        """The last lidar_scan_all() into the pool's own buffer as numpy [n_env, max_agents, n_beams], after the pool's work."""
        import torch
        ptr, nb = self.lidar_all_buffer()
        view = _DevArray(ptr, (self.n_env, self.max_agents, nb // (4 * self.n)), "<f4", self)
        self.sync()
        return torch.as_tensor(view, device=f"cuda:{self.device_id}").cpu().numpy()

    # ---------------------------------------------------------------- Reeds-Shepp planner
    def rs_config(self, radius, center_shift, half_length, half_width, distance_tolerance=0.05, threshold_distance=15.0,
                  sample_step=0.1, length_ratio=2.0, edge_tolerance=1e-4, vehicle_base=None):
        """t2d_rs_config: the tutorial planner's configuration (docs/tutorial/train_parking_demo.ipynb cell 9; planner.RSPlanner
        derives it from a vehicle template).  Needs lidar_config; vehicle_base: n_beams floats or None (computed from the box)."""
        cfg = _ffi.RSParams(radius, center_shift, half_length, half_width, distance_tolerance, threshold_distance, sample_step,
                            length_ratio, edge_tolerance)
        vb = _arr(vehicle_base, np.float32, getattr(self, "n_beams", None), "vehicle_base")
        self._ck(self._lib.t2d_rs_config(self._h, C.byref(cfg), _p(vb)))
        self.rs_params = cfg

    def rs_plan(self, lidar_ptr=None, out_ptr=None, stream=None):
        """t2d_rs_plan: one plan record per env (layout.RS_RECORD_BYTES each) from the scan at lidar_ptr (None: the pool's own
        lidar buffer) into out_ptr (None: the pool's own records, rs_plan_views()).  Asynchronous on `stream`."""
        self._ck(self._lib.t2d_rs_plan(self._h, lidar_ptr, out_ptr, stream))

    def rs_plan_buffer(self):
        """(device pointer, bytes) of the pool's own plan records"""
        ptr, nb = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.t2d_rs_plan_buffers(self._h, C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def rs_plan_views(self, ptr=None, owner=None):
        """Zero-copy torch views of t2d_rs_plan_record [n_env] at `ptr` (None: the pool's own records): status, slot, n_seg,
        n_visited int32 [n]; steer int32 [n, 5] (+1 L, -1 R, 0 S); distance float64 [n, 5] (signed, metres); length, shortest
        float64 [n]."""
        return self._record_views(ptr, self._lib.t2d_rs_plan_buffers, self.n_env, L.RS_RECORD_BYTES, L.RS_RECORD_FIELDS, owner)

    # ---------------------------------------------------------------- Reeds-Shepp path follower
    def rs_follow_config(self, **params):
        """t2d_rs_follow_config: the tutorial follower's configuration (_ffi.RSFollowParams, every field by name; planner.RSFollower
        supplies the notebook's defaults).  Needs rs_config; allocates and clears the follower's state."""
        cfg = _ffi.RSFollowParams(**params)
        self._ck(self._lib.t2d_rs_follow_config(self._h, C.byref(cfg)))
        self.rs_follow_params = cfg

    def rs_follow(self, act_in_ptr, act_out_ptr, plan_ptr=None, out_ptr=None, stream=None):
        """t2d_rs_follow: one launch; float32 [n_env, 2] (steering, accel) rows from act_in_ptr (None: zeros) to act_out_ptr (may
        be the same memory), plan records at plan_ptr (None: the pool's own), records to out_ptr (None: the pool's own)."""
        self._ck(self._lib.t2d_rs_follow(self._h, plan_ptr, act_in_ptr, act_out_ptr, out_ptr, stream))

    def rs_follow_reset(self, mask_ptr=None, stream=None):
        """t2d_rs_follow_reset: agent.reset() for the envs whose byte at mask_ptr (device memory) is non-zero; None: all"""
        self._ck(self._lib.t2d_rs_follow_reset(self._h, mask_ptr, stream))

    def rs_follow_views(self, ptr=None, owner=None):
        """Zero-copy torch views of t2d_rs_follow_record [n_env] at `ptr` (None: the pool's own records): executing, segment,
        events, steps int32 [n]; action float64 [n, 2] (normalised; NaN: the policy's row went through); distance_to_go,
        total_error float64 [n]."""
        return self._record_views(ptr, self._lib.t2d_rs_follow_buffers, self.n_env, L.RS_FOLLOW_RECORD_BYTES,
                                  L.RS_FOLLOW_RECORD_FIELDS, owner)

    def _record_views(self, ptr, own_buffer, n_rows, record_bytes, fields, owner):
        """Zero-copy torch views of the records [n_rows] of record_bytes each at `ptr` (None: the pool's own, which own_buffer
        -- a t2d_*_buffers entry point -- locates), one per entry of `fields` (a layout.*_RECORD_FIELDS table); `owner` (None:
        the pool) is kept alive by the views."""
        import torch
        if ptr is None:
            p_, nb = C.c_void_p(), C.c_size_t()
            self._ck(own_buffer(self._h, C.byref(p_), C.byref(nb)))
            ptr = p_.value
        keep = owner if owner is not None else self
        cols = {t: torch.as_tensor(_DevArray(ptr, (n_rows, record_bytes // int(t[2])), t, keep), device=f"cuda:{self.device_id}")
                for t in ("<i4", "<f8")}
        return {name: cols[t][:, c] for name, (t, c) in fields.items()}

    def _set_ctrl(self, setter, cols, ctrl_rows, ctrl_id, *per_participant):
        """One t2d_set_* call: ctrl_rows [n_ctrl, >= cols] as contiguous float64 and ctrl_id uint8 [n], then the family's further
        per-participant arrays (None: NULL).  ctrl_rows=None uninstalls (n_ctrl 0, every pointer NULL)."""
        if ctrl_rows is None:
            self._ck(setter(self._h, None, 0, 0, None, *[None] * len(per_participant)))
            return
        rows = np.ascontiguousarray(ctrl_rows, np.float64)
        if rows.ndim != 2:
            raise ValueError(f"ctrl_rows must be 2-D [n_ctrl, >= {cols}]")
        cid = _arr(ctrl_id, np.uint8, self.n, "ctrl_id")
        self._ck(setter(self._h, _p(rows), rows.shape[0], rows.shape[1], _p(cid), *map(_p, per_participant)))

    def _f32_per_participant(self, value, name):
        """float32 [n] of a scalar (broadcast) or an array; None stays None"""
        if value is None:
            return None
        v = np.asarray(value, np.float32)
        return _arr(np.broadcast_to(v.reshape(-1) if v.ndim else v, (self.n,)), np.float32, self.n, name)

    def set_idm(self, ctrl_rows, ctrl_id):
        """Install IDM controllers: ctrl_rows [n_ctrl, 8] (layout.IDM_*), ctrl_id [n] uint8 (IDM_NONE =
        action supplied by the caller).  ctrl_rows=None uninstalls."""
        self._set_ctrl(self._lib.t2d_set_idm, L.IDM_COLS, ctrl_rows, ctrl_id)

    def idm_actions(self, forced_leader_ptr=None, stream=None):
        """IDMController.step for every controlled participant (also runs inside step()/integrate())."""
        self._ck(self._lib.t2d_idm_actions(self._h, forced_leader_ptr, stream))

    # ---------------------------------------------------------------- lane-keeping PID controllers
    def set_pid(self, ctrl_rows, ctrl_id=None, target_speed=None, idm_row=None):
        """Install PID controllers (t2d_set_pid): ctrl_rows [n_ctrl, 14] (layout.PID_*; controller.PIDController.row()), ctrl_id
        uint8 [n] (PID_NONE = the caller's row goes through), target_speed float32 [n] (a scalar broadcasts; None: zeros),
        idm_row int32 [n] (rows of set_idm for lon_mode 2; None: row 0).  ctrl_rows=None uninstalls."""
        self._set_ctrl(self._lib.t2d_set_pid, L.PID_COLS, ctrl_rows, ctrl_id, self._f32_per_participant(target_speed, "target_speed"),
                       _arr(idm_row, np.int32, self.n, "idm_row"))

    def pid_actions(self, act_in_ptr, act_out_ptr, record_ptr=None, stream=None):
        """t2d_pid_actions: one launch; float32 [n, 2] (steering, accel) rows from act_in_ptr (None: zeros) to act_out_ptr (may
        be the same memory), records to record_ptr (None: the pool's own, pid_records())."""
        self._ck(self._lib.t2d_pid_actions(self._h, act_in_ptr, act_out_ptr, record_ptr, stream))

    def pid_reset(self, mask_ptr=None, stream=None):
        """t2d_pid_reset: controller.reset() for the envs whose byte at mask_ptr (device memory) is non-zero; None: all"""
        self._ck(self._lib.t2d_pid_reset(self._h, mask_ptr, stream))

    def pid_state(self, state=None):
        """t2d_pid_state: the controllers' state float64 [n, 6] (lat integral, prev_error, prev_derivative, then the longitudinal
        three).  state None: read (after the pool's work); else: replace it."""
        if state is None:
            out = np.empty((self.n, L.PID_STATE_WORDS), np.float64)
            self._ck(self._lib.t2d_pid_state(self._h, _p(out), 0))
            return out
        st = _arr(state, np.float64, self.n * L.PID_STATE_WORDS, "state")
        self._ck(self._lib.t2d_pid_state(self._h, _p(st), 1))

    def pid_records(self, ptr=None, owner=None):
        """Zero-copy torch views of t2d_pid_record [n] at `ptr` (None: the pool's own records): cross_track, lat_error float64
        [n]; segment, leader, events int32 [n]; action float64 [n, 2] (NaN: the caller's row went through).  Views of the pool's own records are valid until the next
        set_pid, which replaces or frees them."""
        return self._record_views(ptr, self._lib.t2d_pid_buffers, self.n, L.PID_RECORD_BYTES, L.PID_RECORD_FIELDS, owner)

    # ---------------------------------------------------------------- pure pursuit and cruise / ACC controllers
    def set_pursuit(self, ctrl_rows, ctrl_id=None, target_speed=None):
        """Install pure-pursuit / acceleration controllers (t2d_set_pursuit): ctrl_rows [n_ctrl, 13] (layout.PURSUIT_*;
        controller.PurePursuitController.row() / AccelerationController.row()), ctrl_id uint8 [n] (PURSUIT_NONE = the caller's row
        goes through), target_speed float32 [n] (a scalar broadcasts; None: zeros).  ctrl_rows=None uninstalls."""
        self._set_ctrl(self._lib.t2d_set_pursuit, L.PURSUIT_COLS, ctrl_rows, ctrl_id,
                       self._f32_per_participant(target_speed, "target_speed"))

    def pursuit_actions(self, act_in_ptr, act_out_ptr, record_ptr=None, stream=None):
        """t2d_pursuit_actions: one launch; float32 [n, 2] (steering, accel) rows from act_in_ptr (None: zeros) to act_out_ptr
        (may be the same memory), records to record_ptr (None: the pool's own, pursuit_records())."""
        self._ck(self._lib.t2d_pursuit_actions(self._h, act_in_ptr, act_out_ptr, record_ptr, stream))

    def pursuit_records(self, ptr=None, owner=None):
        """Zero-copy torch views of t2d_pursuit_record [n] at `ptr` (None: the pool's own records): point float64 [n, 2];
        pre_aiming_distance, distance, cross_track float64 [n]; segment, target_segment, leader, events int32 [n]; action
        float64 [n, 2] (NaN: the caller's row went through).  Views of the pool's own records are valid until the next set_pursuit, which
        replaces or frees them."""
        return self._record_views(ptr, self._lib.t2d_pursuit_buffers, self.n, L.PURSUIT_RECORD_BYTES, L.PURSUIT_RECORD_FIELDS, owner)

    def verify_state_ptr(self, x_ptr, y_ptr, heading_ptr, speed_ptr, interval_ms, valid_ptr, stream=None):
        """verify_state of device-resident candidate columns against the pool's current state."""
        self._ck(self._lib.t2d_verify_state(self._h, x_ptr, y_ptr, heading_ptr, speed_ptr, int(interval_ms),
                                            valid_ptr, stream))

    def verify_state(self, x, y, heading, speed, interval_ms):
        """Host-array convenience: candidate columns are staged in this pool's action / applied-action
        fields (scratch here: the next integrate overwrites them anyway) and the verdict bytes in FLAGS."""
        n = self.n
        saved = [self.download(f) for f in (L.F_ACT0, L.F_ACT1, L.F_APPLIED0, L.F_APPLIED1, L.F_FLAGS)]
        for f, v in zip((L.F_ACT0, L.F_ACT1, L.F_APPLIED0, L.F_APPLIED1), (x, y, heading, speed)):
            self.upload(f, _arr(v, np.float32, n, "candidate"))
        ptr = lambda f: self.field_ptr(f)[0]
        self.verify_state_ptr(ptr(L.F_ACT0), ptr(L.F_ACT1), ptr(L.F_APPLIED0), ptr(L.F_APPLIED1), interval_ms,
                              ptr(L.F_FLAGS))
        out = self.download(L.F_FLAGS).view(np.uint8)[:n].astype(bool)
        for f, v in zip((L.F_ACT0, L.F_ACT1, L.F_APPLIED0, L.F_APPLIED1, L.F_FLAGS), saved):
            self.upload(f, v)
        return out

    def verify_states(self, traj, out_ptr=None, stream=None):
        """`ParticipantBase._verify_trajectory` (participant_base.py:120-131) for every participant at once: bool[N], participant
        i checked under its own type row and model by `PhysicsModelBase.verify_states` (physics_model_base.py:53-73) -- every
        frame against the FIRST one, with the reference's intervals (history.verify_intervals) -- in one launch.
        traj: a DeviceTrajectory of this pool, or a BatchedTrajectory (uploaded into one for the call).
        out_ptr: device memory of N bytes to write the verdicts to, asynchronously on `stream` (then returns None)."""
        from .history import BatchedTrajectory, DeviceTrajectory, verify_intervals
        if not isinstance(traj, BatchedTrajectory) and not (isinstance(traj, DeviceTrajectory) and traj.pool is self):
            raise ValueError("verify_states: a DeviceTrajectory of this pool or a BatchedTrajectory")
        intervals = verify_intervals(traj)   # (the reference's TypeError / IndexError)
        if isinstance(traj, BatchedTrajectory):
            dev = DeviceTrajectory.from_batched(self, traj)
            try:
                return self.verify_states(dev, out_ptr, stream)
            finally:
                dev.close()
        slots = traj.slots()
        iv = np.array([0.0] + [float(v) for v in intervals], np.float64)
        buf = None
        if out_ptr is None:
            import torch
            buf = torch.empty(self.n, dtype=torch.uint8, device=f"cuda:{self.device_id}")
            out_ptr = buf.data_ptr()
        self._ck(self._lib.t2d_verify_states(traj._buf._live(), len(slots), _p(slots), _p(iv), C.c_void_p(out_ptr), stream))
        if buf is None:
            return None
        self.sync()
        return buf.cpu().numpy().astype(bool)

    # ---------------------------------------------------------------- replayed participants
    def replay_bind(self, source, src_env=None, offset_ms=None):
        """Bind a history.ReplaySource: participants whose type row has model layout.MODEL_REPLAY take their state from it
        inside every step (t2d_replay_bind).  src_env int32[n_env]: the source env each env shows (None: its own number);
        offset_ms int32[n_env]: env e at env time f shows stamp f + offset_ms[e] (None: 0; multiples of the period)."""
        import weakref
        se = _arr(src_env, np.int32, self.n_env, "src_env")
        off = _arr(offset_ms, np.int32, self.n_env, "offset_ms")
        buf = source.device_buffer()
        self._ck(self._lib.t2d_replay_bind(self._h, buf._live(), source.n_slots, source.t0_ms, source.period_ms, _p(se), _p(off),
                                           _p(source.first_slot), _p(source.last_slot)))
        self._replay_release_user()
        self.replay_source = source
        self.replay_src_env = np.arange(self.n_env, dtype=np.int32) if se is None else se.copy()
        self.replay_offset_ms = np.zeros(self.n_env, np.int32) if off is None else off.copy()
        buf.pool.__dict__.setdefault("_replay_users", weakref.WeakSet()).add(self)

    def _replay_release_user(self):
        src = self.__dict__.pop("replay_source", None)
        if src is not None and src._buf is not None:
            src._buf.pool.__dict__.get("_replay_users", set()).discard(self)

    def replay_unbind(self):
        if self.__dict__.get("replay_source") is not None and self._h:
            self._ck(self._lib.t2d_replay_bind(self._h, None, 0, 0, 0, None, None, None, None))
            self._replay_release_user()

    def replay_apply(self, stream=None):
        """The replayed participants' state and active byte at the envs' CURRENT time, advancing nothing (t2d_replay_apply):
        after reset() and before snapshot() it puts them where the recording has them at episode start."""
        self._ck(self._lib.t2d_replay_apply(self._h, stream))

    # ---------------------------------------------------------------- off-route detection
    def _route_assignment(self, route_of, threshold):
        """int32[n] / float32[n] (None stays None); scalars and [n_env, max_agents] arrays are accepted"""
        def flat(v, dtype, name):
            if v is None:
                return None
            a = np.asarray(v, dtype)
            return _arr(np.broadcast_to(a.reshape(-1) if a.ndim else a, (self.n,)), dtype, self.n, name)
        return flat(route_of, np.int32, "route_of"), flat(threshold, np.float32, "threshold")

    def set_routes(self, route_sets, set_of_env=None, route_of=None, threshold=0.0):
        """Install map routes for the off-route detector (t2d_set_routes).  route_sets: [[polyline (n, 2), ...] per set] (or
        the CSR triple of traffic.routes_to_csr); set_of_env int32[n_env]: the set each env uses (None: set 0 serves every
        env -- one copy of the map); route_of int32[n]: the route of each participant inside its env's set, -1 = none (a
        scalar broadcasts; None: route 0 for everybody); threshold float32[n] (a scalar broadcasts)."""
        from .traffic import routes_to_csr
        so, vo, xy = route_sets if isinstance(route_sets, tuple) else routes_to_csr(route_sets)
        so, vo = _arr(so, np.int32, None, "set offsets"), _arr(vo, np.int32, None, "route offsets")
        xy = _arr(xy, np.float32, None, "verts_xy")
        if so.size < 2 or vo.size != so[-1] + 1 or xy.size != 2 * vo[-1]:
            raise ValueError("route sets: need n_sets + 1 set offsets (n_sets >= 1), n_route + 1 route offsets and 2 * n_vert coordinates")
        se = _arr(set_of_env, np.int32, self.n_env, "set_of_env")
        ro, th = self._route_assignment(0 if route_of is None else route_of, threshold)
        self._ck(self._lib.t2d_set_routes(self._h, so.size - 1, _p(so), _p(vo), _p(xy), _p(se), _p(ro), _p(th)))
        self._route_release_user()
        self.route_kind = "sets"

    def set_route_assignment(self, route_of=None, threshold=None):
        """route_of / threshold of the installed routes alone (t2d_set_route_assignment; None = unchanged): a new episode on the
        same map uploads no geometry.  For trace routes route_of is the source agent index."""
        ro, th = self._route_assignment(route_of, threshold)
        self._ck(self._lib.t2d_set_route_assignment(self._h, _p(ro), _p(th)))

    def set_routes_from(self, source, src_env=None, windows=None, route_of=None, threshold=0.0):
        """Trace routes straight from a recording (t2d_set_routes_from_traj): the route of participant (e, a) is the polyline
        through the recorded (x, y) of source participant (src_env[e], route_of[i]) -- `get_trace` -- read by the kernel out of
        the trajectory's own columns; nothing is copied or brought to the host.  source: a history.DeviceTrajectory (every slot
        in use) or a history.ReplaySource (its windows; src_env defaults to the current replay binding's when this pool replays
        that source).  windows: (first_slot, last_slot) int32[N_src]; route_of None: the own agent index, -1 = none."""
        import weakref
        from .history import DeviceTrajectory
        if isinstance(source, DeviceTrajectory):
            buf, n_slots = source._buf, source._n_used
        else:
            buf, n_slots = source.device_buffer(), source.n_slots
            if windows is None:
                windows = (source.first_slot, source.last_slot)
            if src_env is None and self.__dict__.get("replay_source") is source:
                src_env = self.replay_src_env
        first, last = (None, None) if windows is None else windows
        first, last = _arr(first, np.int32, buf.n, "first_slot"), _arr(last, np.int32, buf.n, "last_slot")
        se = _arr(src_env, np.int32, self.n_env, "src_env")
        ro, th = self._route_assignment(route_of, threshold)
        self._ck(self._lib.t2d_set_routes_from_traj(self._h, buf._live(), int(n_slots), _p(se), _p(first), _p(last), _p(ro), _p(th)))
        self._route_release_user()
        self.route_kind = "traces"
        self._route_buf = buf
        buf.pool.__dict__.setdefault("_route_users", weakref.WeakSet()).add(self)

    def _route_release_user(self):
        buf = self.__dict__.pop("_route_buf", None)
        if buf is not None:
            buf.pool.__dict__.get("_route_users", set()).discard(self)
        self.route_kind = None

    def clear_routes(self):
        if self.__dict__.get("route_kind") is not None and self._h:
            self._ck(self._lib.t2d_set_routes(self._h, 0, None, None, None, None, None, None))
            self._route_release_user()

    def off_route(self, dist_ptr=None, off_ptr=None, stream=None):
        """OffRoute.update for every participant in one launch (t2d_off_route): distance float32[n] and verdict uint8[n] written
        to the device memory at dist_ptr / off_ptr, or -- None -- to buffers of the pool's own (off_route_buffers(),
        off_route_all()).  Asynchronous on `stream`; reads the pool's current state, changes nothing in it."""
        self._ck(self._lib.t2d_off_route(self._h, dist_ptr, off_ptr, stream))

    @contextlib.contextmanager
    def _route_writer(self, count, stream):
        """What curve_routes / spline_routes / planview_routes / polyline_routes start with: the pool's device, the launch stream (`stream`, or
        torch's current one) and the int32 [n_env] count tensor (`count` checked, or a new one), inside a torch stream context
        of the launch stream, so that uploads and conversions made in it run ahead of the launch."""
        import torch
        dev = torch.device("cuda", self.device_id)
        if count is not None and (count.dtype != torch.int32 or tuple(count.shape) != (self.n_env,) or not count.is_contiguous()):
            raise ValueError(f"count must be a contiguous int32 [{self.n_env}] tensor")
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.stream(torch.cuda.ExternalStream(st, device=dev)):
            yield dev, st, torch.zeros(self.n_env, dtype=torch.int32, device=dev) if count is None else count

    def curve_routes(self, words, starts, radius, step_size, rule, route=0, count=None, stream=None):
        """t2d_curve_routes: sample one curve per env (interpolator.pack_words records, float64 CUDA tensor [n_env, 6]; starts float64
        CUDA tensor [n_env, 3]; rule layout.CURVE_DUBINS / CURVE_RS or "dubins" / "rs") into route `route` of each env's own route
        set, as fp32 vertices in the installed sets' device storage: the route's vertex count is the capacity, vertices past the
        curve's points repeat its end point, a word of 0 segments leaves the route as it is.  Needs set_routes with one set per
        env.  off_route / pid_actions / pursuit_actions see the curve in their next launch on `stream`.  Returns the int32 CUDA
        tensor [n_env] of the curves' full point counts (`count`, or a new one).  Asynchronous."""
        import torch
        rule = {"dubins": L.CURVE_DUBINS, "rs": L.CURVE_RS}.get(rule, rule)
        if words.dtype != torch.float64 or tuple(words.shape) != (self.n_env, L.CURVE_WORD_BYTES // 8) or not words.is_contiguous():
            raise ValueError(f"words must be a contiguous float64 [{self.n_env}, 6] tensor (interpolator.pack_words)")
        if starts.dtype != torch.float64 or tuple(starts.shape) != (self.n_env, 3) or not starts.is_contiguous():
            raise ValueError(f"starts must be a contiguous float64 [{self.n_env}, 3] tensor")
        with self._route_writer(count, stream) as (_, st, count):
            self._ck(self._lib.t2d_curve_routes(self._h, words.data_ptr(), starts.data_ptr(), float(radius), float(step_size),
                                                int(rule), int(route), count.data_ptr(), st))
        self._curve_inputs = (words, starts)   # (kept alive until the launch has run)
        return count

    def spline_routes(self, kind, control_points, n_ctrl=None, n_interpolation=100, degree=0, knot_vectors=None, boundary_type=3,
                      first_derivatives=None, route=0, count=None, stream=None):
        """t2d_spline_routes: one Bezier / B-spline / cubic spline curve per env (kind "bezier" / "bspline" / "cubic" or
        layout.SPLINE_*; control_points [n_env, m, 2] and the other arguments as in interpolator.Bezier / BSpline / CubicSpline
        .get_curve, numpy or float64 CUDA tensors) into route `route` of each env's own route set, under the rules of curve_routes:
        the route's vertex count is the capacity, vertices past the curve's points repeat its last point (for a B-spline its last
        sample, not the curve's end), a row without a curve leaves the route as it is.  Needs set_routes with one set per env.
        Returns the int32 CUDA tensor [n_env] of the curves' full point counts (`count`, or a new one).  Asynchronous."""
        from . import interpolator as I
        kind, n, m, n_interpolation, degree, boundary_type, _ = I.spline_check(kind, control_points, n_ctrl, n_interpolation, degree,
                                                                               knot_vectors, boundary_type, first_derivatives)
        if n != self.n_env:
            raise ValueError(f"control_points must hold one control polygon per env: [{self.n_env}, m, 2]")
        with self._route_writer(count, stream) as (dev, st, count):
            inputs = I.spline_inputs(dev, n, m, control_points, n_ctrl, knot_vectors, first_derivatives)
        ctrl, n_ctrl, knots, derivs = inputs
        self._ck(self._lib.t2d_spline_routes(self._h, kind, ctrl.data_ptr(), n_ctrl.data_ptr(), m, n_interpolation, degree,
                                             None if knots is None else knots.data_ptr(), boundary_type,
                                             None if derivs is None else derivs.data_ptr(), int(route), count.data_ptr(), st))
        self._spline_inputs = inputs   # (kept alive until the launch has run)
        return count

    def planview_routes(self, records, n_geom, stride=1, route=0, rule="reference", count=None, stream=None):
        """t2d_planview_routes: the reference line of one OpenDRIVE plan view per env (records float64 [n_env, max_geom, 14] and
        n_geom int [n_env] of interpolator.pack_planview, CPU or CUDA tensors; rule "reference" / "standard": how spirals are
        evaluated, interpolator.Spiral.get_curve) into route `route` of each env's own route set, under the rules of
        curve_routes.  A road has ten raw points per metre, hence stride >= 1: the vertices are the line's kept points 0, stride,
        2 stride, ... and always its last one.  The route's vertex count is the capacity, vertices past the line's repeat its
        last point, a line of more vertices than the capacity writes the first `capacity`, a road without a line leaves the
        route as it is.  Needs set_routes with one set per env.  Returns the int32 CUDA tensor [n_env] of the lines' vertex
        counts (`count`, or a new one).  Asynchronous."""
        from . import interpolator as I
        rule = I._rule(rule)
        with self._route_writer(count, stream) as (dev, st, count):
            if hasattr(records, "shape") and len(records.shape) and records.shape[0] != self.n_env:
                raise ValueError(f"records must hold one road per env: [{self.n_env}, max_geom, {L.PLANVIEW_RECORD_BYTES // 8}]")
            inputs = I.planview_inputs(dev, records, n_geom)
        self._ck(self._lib.t2d_planview_routes(self._h, inputs[0].data_ptr(), inputs[1].data_ptr(), inputs[0].shape[1], rule, int(stride),
                                               int(route), count.data_ptr(), st))
        self._planview_inputs = inputs   # (kept alive until the launch has run)
        return count

    def polyline_routes(self, points, counts, route=0, count=None, stream=None):
        """t2d_polyline_routes: a polyline per env that is already on the device -- a planner's path -- into route `route` of each
        env's own route set, under the rules of curve_routes.  points: a contiguous float64 CUDA tensor [n_env, max_pts, C], C >= 2,
        x and y first (search.SamplePaths.path and search.HybridPaths.path with its heading column go in as they are); counts: a
        contiguous int32 CUDA tensor [n_env] (a planner's path_len as it is).  The used length is min(counts, max_pts); the vertices
        are the fp32 roundings of the first points, vertices past the end repeat the last point, a route of fewer vertices takes
        the first of them.  A row with counts <= 0, or with a coordinate among the points it would write that is not finite in
        fp32, leaves the route as it is.  Needs set_routes with one set per env.  Returns the int32 CUDA tensor [n_env] of the
        used lengths, 0 for a row left as it is (`count`, or a new one).  Asynchronous."""
        import torch
        if not isinstance(points, torch.Tensor) or points.dtype != torch.float64 or points.dim() != 3 or points.shape[0] != self.n_env \
                or points.shape[1] < 1 or points.shape[2] < 2 or not points.is_contiguous():
            raise ValueError(f"points must be a contiguous float64 [{self.n_env}, max_pts >= 1, C >= 2] tensor")
        if not isinstance(counts, torch.Tensor) or counts.dtype != torch.int32 or tuple(counts.shape) != (self.n_env,) \
                or not counts.is_contiguous():
            raise ValueError(f"counts must be a contiguous int32 [{self.n_env}] tensor")
        with self._route_writer(count, stream) as (_, st, count):
            self._ck(self._lib.t2d_polyline_routes(self._h, points.data_ptr(), counts.data_ptr(), points.shape[1], points.shape[2],
                                                   int(route), count.data_ptr(), st))
        self._polyline_inputs = (points, counts)   # (kept alive until the launch has run)
        return count

    def route_vertices(self):
        """Zero-copy torch view float32 [n_vertices, 2] of the installed route sets' vertices on the device (t2d_route_vertices), in
        the order set_routes flattened them: what curve_routes writes into.  Valid until the routes are replaced or cleared.  The
        view is writable: writing through it edits the routes off_route / pid_actions / pursuit_actions read, and ordering such
        writes against their launches is the caller's own business."""
        import torch
        ptr, n = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.t2d_route_vertices(self._h, C.byref(ptr), C.byref(n)))
        return torch.as_tensor(_DevArray(ptr.value, (n.value, 2), "<f4", self), device=f"cuda:{self.device_id}")

    def off_route_buffers(self):
        """(distance pointer, verdict pointer, elements) of the pool's own result buffers (after an off_route() into them)."""
        d, o, n = C.c_void_p(), C.c_void_p(), C.c_size_t()
        self._ck(self._lib.t2d_off_route_buffers(self._h, C.byref(d), C.byref(o), C.byref(n)))
        return d.value, o.value, n.value

    def off_route_all(self):
        """The last off_route() into the pool's own buffers as numpy (distance float32, off bool), each [n_env, max_agents],
        after the pool's work."""
        import torch
        d, o, n = self.off_route_buffers()
        shape = (self.n_env, self.max_agents)
        self.sync()
        dev = f"cuda:{self.device_id}"
        return (torch.as_tensor(_DevArray(d, shape, "<f4", self), device=dev).cpu().numpy(),
                torch.as_tensor(_DevArray(o, shape, "|u1", self), device=dev).cpu().numpy().astype(bool))

    def off_route_host(self, stream=None):
        """off_route() into the pool's own buffers + off_route_all()."""
        self.off_route(None, None, stream)
        return self.off_route_all()

    # ---------------------------------------------------------------- racing tile progress
    def set_tracks(self, tracks, set_of_env=None, ego_index=0, rule="forward", max_advance=8, check_off_road=False):
        """Install racing tracks (t2d_set_tracks).  tracks: a list of float32 [n_tile, 4, 2] arrays -- the tiles of each track
        in ring order, tile i's successor is (i + 1) % n_tile, vertices in the order of Lane.geometry -- shared between envs;
        set_of_env int32[n_env]: the track each env drives on (None: track 0); ego_index: the agent that drives;
        rule: "reference" (the reference's march and gap filling, degenerate case included) or "forward" (build-defined: only
        max_advance successors of tile_visiting are looked at, 0 = the whole ring, and only the tiles strictly between
        tile_visiting and the touched run are filled); check_off_road: the ego's off-lane flag ends the episode (traffic
        status 6, reward -5; build-defined).  Every env starts as after track_reset().  None removes the tracks."""
        if tracks is None:
            self._ck(self._lib.t2d_set_tracks(self._h, 0, None, None, None, 0, 0, 0, 0))
            self.track_n_tile = None
            self._tracks_generated = False
            return
        rules = {"reference": L.TRACK_RULE_REFERENCE, "forward": L.TRACK_RULE_FORWARD}
        if rule not in rules:
            raise ValueError(f"unknown progress rule {rule!r}")
        tiles = [np.ascontiguousarray(t, np.float32).reshape(-1, 4, 2) for t in tracks]
        off = np.concatenate([[0], np.cumsum([len(t) for t in tiles])]).astype(np.int32)
        xy = np.ascontiguousarray(np.concatenate(tiles) if tiles else np.zeros((0, 4, 2), np.float32))
        se = _arr(set_of_env, np.int32, self.n_env, "set_of_env")
        self._ck(self._lib.t2d_set_tracks(self._h, len(tiles), _p(off), _p(xy), _p(se), int(ego_index), rules[rule],
                                          int(max_advance), int(bool(check_off_road))))
        n = np.diff(off)
        self.track_n_tile = (n[se] if se is not None else np.full(self.n_env, n[0])).astype(np.int32)
        self._tracks_generated = False

    def set_tracks_generated(self, n_sets, seed, first_track=0, track_stride=None, set_of_env=None, ego_index=0, rule="forward",
                             max_advance=8, regenerate=False, car_length=None, check_off_road=False):
        """Generate n_sets racing tracks ON THE DEVICE and install them (t2d_set_tracks_generated): set s is the track of the
        counter stream (seed, first_track + s) -- what RacingTrackGenerator.generate_batch returns for the same key; env e
        drives on set_of_env[e] (None: n_sets == 1 -> track 0, n_sets == n_env -> its own).  Besides the tiles the call puts each
        env's out-bound boundary, the ego's start pose (state columns and episode snapshot, speed 0) and the progress state of
        track_reset() in place; only the tile counts come back to the host (`track_n_tile`).  Needs set_param_table, reset,
        snapshot and a boundary array first.  regenerate=True (every env its own set, track_stride >= n_env, default n_env)
        allows regenerate_tracks().  car_length: the ego's length (None: the medium car's).  Off-road detection needs the
        host's lane geometry: check_off_road=True raises ValueError."""
        if check_off_road:
            raise ValueError("check_off_road is not supported with generated tracks (the lane geometry is built on the host)")
        rules = {"reference": L.TRACK_RULE_REFERENCE, "forward": L.TRACK_RULE_FORWARD}
        if rule not in rules:
            raise ValueError(f"unknown progress rule {rule!r}")
        if car_length is None:
            from .participant import VEHICLE_TEMPLATE
            car_length = VEHICLE_TEMPLATE["medium_car"][0]
        se = _arr(set_of_env, np.int32, self.n_env, "set_of_env")
        stride = self.n_env if track_stride is None else int(track_stride)
        self._ck(self._lib.t2d_set_tracks_generated(self._h, int(n_sets), int(seed) & (2**64 - 1), int(first_track), stride,
                                                    float(car_length), _p(se), int(ego_index), rules[rule], int(max_advance),
                                                    int(bool(regenerate))))
        self._tracks_generated = True
        import torch
        b, S = self.generated_track_buffers()      # (the call was synchronous) -- the tile counts alone cross to the host
        n = torch.as_tensor(_DevArray(b["n_tile"], (S,), "<i4", self), device=f"cuda:{self.device_id}").cpu().numpy()
        soe = se if se is not None else (np.zeros(self.n_env, np.int32) if int(n_sets) == 1 else np.arange(self.n_env))
        self.track_n_tile = n[soe].astype(np.int32)
        self.track_n_tile_set = np.asarray(soe, np.int64)

    def regenerate_tracks(self, stream=None):
        """One launch between track_progress(True) and restore(done_only=True) (t2d_tracks_regenerate): every env whose track
        status says its episode ended gets the track of its next episode, generated in place into its own set, with its tile
        count, boundary and snapshot start pose; asynchronous on `stream`.  Needs set_tracks_generated(regenerate=True)."""
        self._ck(self._lib.t2d_tracks_regenerate(self._h, stream))

    def generated_track_buffers(self):
        """Device pointers of the generated track sets' records + their number: dict(tiles, n_tile, n_checkpoint, attempt,
        start_pose, start_line, boundary, episode), n_sets."""
        ptrs = [C.c_void_p() for _ in range(8)]
        n = C.c_size_t()
        self._ck(self._lib.t2d_generated_track_buffers(self._h, *[C.byref(q) for q in ptrs], C.byref(n)))
        names = ("tiles", "n_tile", "n_checkpoint", "attempt", "start_pose", "start_line", "boundary", "episode")
        return dict(zip(names, (q.value for q in ptrs))), int(n.value)

    def generated_tracks(self, tiles=True):
        """The generated track sets as numpy, after the pool's work: n_tile, n_checkpoint, attempt int32[n_sets], start_pose
        f64[n_sets, 3], start_line f32[n_sets, 2, 2], boundary f32[n_sets, 4], episode int32[n_env] and (tiles=True) `tiles`, a
        list of float32 [n_tile, 4, 2] arrays (the 64 KiB slot of every set is downloaded: a test / inspection helper)."""
        import torch
        self.sync()
        b, S = self.generated_track_buffers()
        dev = f"cuda:{self.device_id}"
        shapes = dict(n_tile=((S,), "<i4"), n_checkpoint=((S,), "<i4"), attempt=((S,), "<i4"), start_pose=((S, 3), "<f8"),
                      start_line=((S, 2, 2), "<f4"), boundary=((S, 4), "<f4"), episode=((self.n_env,), "<i4"))
        out = {k: torch.as_tensor(_DevArray(b[k], sh, ts, self), device=dev).cpu().numpy() for k, (sh, ts) in shapes.items()}
        if tiles:
            t = torch.as_tensor(_DevArray(b["tiles"], (S, L.MAX_TRACK_TILES, 4, 2), "<f4", self), device=dev)
            out["tiles"] = [t[s, :int(out["n_tile"][s])].cpu().numpy() for s in range(S)]
        return out

    def _track_env_mask(self, env_mask):
        return None if env_mask is None else _arr(np.asarray(env_mask, bool), np.uint8, self.n_env, "env_mask")

    def track_reset(self, env_mask=None):
        """_reset_map (envs/racing.py:303-312) for the selected envs (None: all): only tile 0 visited, tile_visiting = 0."""
        self._ck(self._lib.t2d_track_reset(self._h, _p(self._track_env_mask(env_mask))))

    def set_track_state(self, tile_visiting, visited, env_mask=None):
        """The progress state of the selected envs from the caller's values (t2d_track_upload): tile_visiting int32[n_env];
        visited bool [n_env, <= MAX_TRACK_TILES] (tile t of env e) or the packed uint32 [n_env, TRACK_MASK_WORDS] mask."""
        tv = _arr(tile_visiting, np.int32, self.n_env, "tile_visiting")
        v = np.asarray(visited)
        if v.dtype != np.uint32:
            v = pack_track_mask(v)
        m = _arr(v, np.uint32, self.n_env * L.TRACK_MASK_WORDS, "visited mask")
        self._ck(self._lib.t2d_track_upload(self._h, _p(self._track_env_mask(env_mask)), _p(tv), _p(m)))

    def track_progress(self, write_status=False, stream=None):
        """_locate_agent + check_status + _get_rewards of the racing env for every env in one launch (t2d_track_progress),
        asynchronous on `stream`, from the state and the status bytes the last step left.  write_status: status and reward also
        go to the pool's own fields (restore(1) then puts finished episodes back)."""
        self._ck(self._lib.t2d_track_progress(self._h, int(bool(write_status)), stream))

    def track_buffers(self):
        """Device pointers of the progress results: dict(tile_visiting, num_visited, mask, status, reward)."""
        ptrs = [C.c_void_p() for _ in range(5)]
        n = C.c_size_t()
        self._ck(self._lib.t2d_track_buffers(self._h, *[C.byref(q) for q in ptrs], C.byref(n)))
        return dict(zip(("tile_visiting", "num_visited", "mask", "status", "reward"), (q.value for q in ptrs)))

    def track_views(self):
        """Zero-copy torch views of track_buffers() (valid until set_tracks / close), and `num_tile` int32[n_env], the tiles
        of each env's ring: a view of the device's counts when every env owns a generated set, else a gathered / uploaded copy."""
        import torch
        b, E, dev = self.track_buffers(), self.n_env, f"cuda:{self.device_id}"
        shapes = dict(tile_visiting=((E,), "<i4"), num_visited=((E,), "<i4"), mask=((E, L.TRACK_MASK_WORDS), "<u4"),
                      status=((E, 4), "|u1"), reward=((E,), "<f4"))
        # (torch has no uint32 everywhere: the mask is viewed as int32, same bits)
        out = {}
        for k, (shape, ts) in shapes.items():
            out[k] = torch.as_tensor(_DevArray(b[k], shape, "<i4" if ts == "<u4" else ts, self), device=dev)
        # the tiles of each env's ring: the device's own counts for generated tracks (regeneration changes them), one per env
        if self._tracks_generated:
            g, S = self.generated_track_buffers()
            n = torch.as_tensor(_DevArray(g["n_tile"], (S,), "<i4", self), device=dev)
            own = S == E and np.array_equal(self.track_n_tile_set, np.arange(E))
            out["num_tile"] = n if own else n[torch.as_tensor(self.track_n_tile_set, device=dev)]
        else:
            out["num_tile"] = torch.as_tensor(self.track_n_tile, device=dev)
        return out

    def track_state(self):
        """The progress results as numpy, after the pool's work: dict(tile_visiting int32[n_env], num_visited int32[n_env],
        mask uint32[n_env, TRACK_MASK_WORDS], status uint8[n_env, 4], reward float32[n_env], num_tile int32[n_env]: the tiles
        of each env's ring -- the device's own counts with generated tracks, which regeneration changes)."""
        self.sync()
        out = {k: v.cpu().numpy() for k, v in self.track_views().items()}
        out["mask"] = out["mask"].view(np.uint32)
        return out

    # ---------------------------------------------------------------- BEV camera
    def camera_config(self, width, height, perception_range, bind_slot=0, heading_up=True, layers=L.CAMERA_LAYER_ALL,
                      format=L.CAMERA_FORMAT_CLASS | L.CAMERA_FORMAT_RGB):
        """Configure the BEV camera of every env (t2d_camera_config): width x height pixels, perception_range = (left,
        right, front, back) in metres around participant `bind_slot`, heading_up (the participant points to the front of
        the image) or north-up, layers / format = layout.CAMERA_LAYER_* / CAMERA_FORMAT_* bits.  width = 0 removes it."""
        l, r, f, b = (0.0,) * 4 if not width else [float(v) for v in perception_range]
        self._ck(self._lib.t2d_camera_config(self._h, int(width), int(height), l, r, f, b, int(bind_slot), int(bool(heading_up)),
                                             int(layers), int(format)))
        self._camera_shape = (int(height), int(width)) if width else None

    def camera_set_palette(self, rgb):
        """Colours of classes 0 .. len(rgb) - 1: uint8 [n_class, 3] (t2d_camera_set_palette)."""
        a = np.ascontiguousarray(rgb, np.uint8).reshape(-1, 3)
        self._ck(self._lib.t2d_camera_set_palette(self._h, _p(a), len(a)))

    def camera_set_style(self, class_of_type=None, z_of_class=None):
        """class_of_type uint8[MAX_TYPES]: the class participants of each parameter row are drawn as (None: boxes are
        vehicles, discs pedestrians; CAMERA_CLASS_BACKGROUND = not drawn); z_of_class uint8[CAMERA_N_CLASS] (None: the
        reference's resolved z-orders)."""
        c = None if class_of_type is None else _arr(class_of_type, np.uint8, L.MAX_TYPES, "class_of_type")
        z = None if z_of_class is None else _arr(z_of_class, np.uint8, L.CAMERA_N_CLASS, "z_of_class")
        self._ck(self._lib.t2d_camera_set_style(self._h, _p(c), _p(z)))

    def camera_render(self, stream=None, out_class=None, out_rgb=None):
        """One launch, asynchronous on `stream`: the camera image of every env from the pool's current state
        (t2d_camera_render).  out_class / out_rgb: device pointers (both None: the library's own images, camera_views())."""
        self._ck(self._lib.t2d_camera_render(self._h, out_class, out_rgb, stream))

    def camera_buffers(self):
        """Device pointers and byte sizes of the library's own images: dict(image_class=(ptr, nbytes), image=(ptr, nbytes));
        the pointer of a format that was not configured is None."""
        pc, pr, nc, nr = C.c_void_p(), C.c_void_p(), C.c_size_t(), C.c_size_t()
        self._ck(self._lib.t2d_camera_buffers(self._h, C.byref(pc), C.byref(pr), C.byref(nc), C.byref(nr)))
        return dict(image_class=(pc.value, nc.value), image=(pr.value, nr.value))

    def camera_views(self):
        """Zero-copy torch views of the library's own images (valid until camera_config / close): image_class uint8
        [n_env, H, W] and image uint8 [n_env, H, W, 3]; a format that was not configured is absent."""
        import torch
        b, (H, W), dev = self.camera_buffers(), self._camera_shape, f"cuda:{self.device_id}"
        out = {}
        for k, shape in (("image_class", (self.n_env, H, W)), ("image", (self.n_env, H, W, 3))):
            if b[k][0]:
                out[k] = torch.as_tensor(_DevArray(b[k][0], shape, "|u1", self), device=dev)
        return out

    # ---------------------------------------------------------------- occupancy grid
    def occupancy_grid(self, H, W, cell_size, origin, inflate=0.0, include_participants=False, exclude_slot=None, free_weight=1.0,
                       weight=None, mask=None, stream=None, naive=False):
        """t2d_occupancy_grid: the occupancy grid of every env's current scene in one launch, asynchronous on `stream` (None:
        torch's current stream).  The window is shared by the batch: cell (row, col) is the closed square of side cell_size
        centred at origin + (col, row) * cell_size, occupied iff its distance to a static ring (or a live quad of a generated
        scene) or -- include_participants -- to an active participant's box or disc is <= inflate; exclude_slot: the participant
        left out (None: the pool's ego index, -1: none).  weight: a contiguous float64 CUDA tensor [n_env, H, W] written in place
        (free_weight in free cells, +inf in occupied ones: what search.plan_batch / HybridAStar.plan_batch / RRT.plan_batch read
        in place), mask: uint8 [n_env, H, W] (1 = occupied); what is not passed is allocated.  naive=True: the measurement
        yardstick (the same grid).  Returns OccupancyGrids: weight, mask, hw int32 [n_env, 2], status int32 [n_env] (OCC_OK /
        OCC_INVALID: a listed participant's pose is not finite, every cell of the row is an obstacle), cell_size, origin."""
        import torch
        dev = torch.device("cuda", self.device_id)
        H, W = int(H), int(W)
        if exclude_slot is None:
            exclude_slot = self.status_config.ego_index if hasattr(self, "status_config") else 0
        if len(origin) != 2:
            raise ValueError(f"origin must be two numbers, got {origin}")
        if H >= 1 and W >= 1:
            for name, t, dt in (("weight", weight, torch.float64), ("mask", mask, torch.uint8)):
                if t is not None and (not isinstance(t, torch.Tensor) or t.dtype != dt or tuple(t.shape) != (self.n_env, H, W)
                                      or not t.is_contiguous() or t.device != dev):
                    raise ValueError(f"{name} must be a contiguous {dt} [{self.n_env}, {H}, {W}] tensor on {dev}")
        st = stream if stream is not None else torch.cuda.current_stream(dev).cuda_stream
        with torch.cuda.stream(torch.cuda.ExternalStream(st, device=dev)):
            shape = (self.n_env, max(H, 0), max(W, 0))
            weight = torch.empty(shape, dtype=torch.float64, device=dev) if weight is None else weight
            mask = torch.empty(shape, dtype=torch.uint8, device=dev) if mask is None else mask
            hw = torch.empty((self.n_env, 2), dtype=torch.int32, device=dev)
            status = torch.empty(self.n_env, dtype=torch.int32, device=dev)
            self._ck(self._lib.t2d_occupancy_grid(self._h, H, W, float(cell_size), float(origin[0]), float(origin[1]), float(inflate),
                                                  int(bool(include_participants)), int(exclude_slot), float(free_weight),
                                                  weight.data_ptr(), mask.data_ptr(), hw.data_ptr(), status.data_ptr(),
                                                  L.OCC_FORMAT_NAIVE if naive else 0, st))
        return OccupancyGrids(weight, mask, hw, status, float(cell_size), (float(origin[0]), float(origin[1])))

    def parking_scenes(self, seed, type_proportion=0.5, vehicle_size=(5.3, 2.5), regenerate=False, first_env=0,
                       env_stride=None):
        """Device-side ParkingLotGenerator writing straight into this pool (one participant per env): obstacles,
        boundary, target, start pose, snapshot, IoU state -- nothing crosses PCIe.  regenerate=True: after every
        step, envs whose episode ended get the scene of their next episode (stream first_env + e + k * env_stride) --
        from a ring of 16 lots per env staged ahead on a stream of the pool's own, copied in by the step launch itself
        (single-ego pools) or by one small launch behind it.  An env cannot outrun its ring (an episode lasts at least
        two steps, the ring is topped up every 8); should a slot ever be found unstaged the env keeps its lot and the
        next sync() / download() raises T2DError(ERR_STATE) once (include/t2d.h, t2d_parking_scenes).
        regenerate="inline" generates them on the step's stream instead of staging them ahead (C ABI value 2)."""
        stride = self.n_env if env_stride is None else int(env_stride)
        self._ck(self._lib.t2d_parking_scenes(self._h, int(seed) & (2**64 - 1), int(first_env), stride,
                                              float(type_proportion), float(vehicle_size[0]), float(vehicle_size[1]),
                                              2 if regenerate == "inline" else int(bool(regenerate))))

    def get_parking_scenes(self):
        """The scenes currently installed by parking_scenes(): a generator.ParkingScenes plus `.episode`."""
        from .generator import MAX_QUADS, ParkingScenes
        n = self.n_env
        out = ParkingScenes(np.zeros((n, MAX_QUADS, 4, 2), np.float32), np.zeros((n, MAX_QUADS), np.int32),
                            np.zeros(n, np.int32), np.zeros((n, 3)), np.zeros((n, 4, 2), np.float32), np.zeros(n),
                            np.zeros((n, 4), np.float32), np.zeros(n, np.uint32), None)
        episode = np.zeros(n, np.int32)
        ptr = lambda a: a.ctypes.data_as(C.c_void_p)
        self._ck(self._lib.t2d_get_parking_scenes(self._h, ptr(out.quads), ptr(out.quad_id), ptr(out.n_quads),
                                                  ptr(out.start), ptr(out.target), ptr(out.target_heading),
                                                  ptr(out.boundary), ptr(out.info), ptr(episode)))
        out.episode = episode
        return out

    # ---------------------------------------------------------------- the Gym-API host path
    def frame_config(self, lidar=False, target=False, zero_copy=False, n_frames=4):
        """Sections of the host frame t2d_step_host fills (t2d_frame_config) and the number of pinned host frames; returns
        the layout."""
        lay = _ffi.FrameLayout()
        mask = (L.FRAME_LIDAR if lidar else 0) | (L.FRAME_TARGET if target else 0) | (L.FRAME_ZEROCOPY if zero_copy else 0)
        self._ck(self._lib.t2d_frame_config(self._h, mask, int(n_frames), C.byref(lay)))
        key = (mask, int(n_frames), bytes(lay))
        if getattr(self, "_frame_key", None) == key:
            # the configuration already in place (every env reset asks): the library kept the pinned frames, and so do we --
            # HostFrame objects, their views and what callers still hold of them stay valid and tracked
            return self.frame_layout
        self._frame_key = key
        self.frame_layout = lay
        self.n_frames = int(n_frames)
        self._frames = [None] * self.n_frames
        self._frame_ptr = C.c_void_p()
        self._frame_turn = 0
        return lay

    def host_action_buffer(self):
        """float32 [n, 2] numpy view of the pool's own pinned action staging buffer (t2d_host_action_buffer): actions written
        there and passed to step_host as this very array are not copied again (valid until the next frame_config)."""
        ptr = C.c_void_p()
        self._ck(self._lib.t2d_host_action_buffer(self._h, C.byref(ptr)))
        buf = (C.c_float * (2 * self.n)).from_address(ptr.value)
        return np.frombuffer(buf, np.float32).reshape(self.n, 2)

    def set_target_headings(self, heading):
        h = _arr(heading, np.float64, self.n_env, "target_heading")
        self._ck(self._lib.t2d_set_target_headings(self._h, _p(h)))

    def _pick_frame(self, fresh):
        """Index of the pinned frame the next call fills and whether its contents must be copied out.  fresh=False: the frames
        in turn (views valid until n_frames - 1 further calls).  fresh=True: a frame nobody holds a view of any more -- what the
        caller gets is then as good as a new array, without a copy; should every frame but the last still be held (a caller
        that keeps the results of many steps by reference), the last one is filled and copied out."""
        if not fresh:
            k = self._frame_turn
            self._frame_turn = (k + 1) % self.n_frames
            return k, False
        last = self.n_frames - 1
        for k in range(last):
            fr = self._frames[k]
            if fr is None or not fr.in_use():
                return k, False
        return last, True

    def _frame(self, k):
        fr = self._frames[k]
        if fr is None:   # (the views of a pinned frame are built once)
            buf = (C.c_uint8 * self.frame_layout.bytes).from_address(self._frame_ptr.value)
            arr = np.frombuffer(buf, np.uint8)
            fr = HostFrame(arr, self.frame_layout)
            del arr, buf
            self._frames[k] = fr   # (first: the idle reference counts include the list's reference and the local name's,
            fr.calibrate()         #  exactly what _pick_frame's `fr.in_use()` sees when nobody else holds the frame)
        return fr

    def step_host(self, actions, interval_ms=100, stream=None, action_box=None, fresh=False):
        """ParkingEnv.step for every env, host to host (t2d_step_host): actions float32 [n, 2] (steering, accel) C-contiguous or
        None (the actions already in the pool); returns the HostFrame -- views of pinned memory (see _pick_frame for how long
        they stay valid).  action_box: float32 [4] (steering lo, hi, accel lo, hi) = `action_space.contains` for every row,
        checked by the library while it stages the actions (T2DError with code ERR_ACTION, nothing stepped)."""
        if actions is not None:
            if actions.dtype != np.float32 or actions.size != 2 * self.n or not actions.flags.c_contiguous:
                raise ValueError(f"actions must be C-contiguous float32 [{self.n}, 2]")
            actions = actions.ctypes.data
        if action_box is not None:
            action_box = action_box.ctypes.data
        k, must_copy = self._pick_frame(fresh)
        rc = self._lib.t2d_step_host(self._h, actions, action_box, interval_ms, stream, k, C.byref(self._frame_ptr))
        if rc:
            self._ck(rc)
        fr = self._frame(k)
        return fr.copy() if must_copy else fr

    def frame_fetch(self, stream=None, fresh=False):
        """The frame of the current state without stepping (t2d_frame_fetch)."""
        k, must_copy = self._pick_frame(fresh)
        self._ck(self._lib.t2d_frame_fetch(self._h, stream, k, C.byref(self._frame_ptr)))
        fr = self._frame(k)
        return fr.copy() if must_copy else fr

    def set_integrator_variant(self, variant):
        v = {"exact": 0, "fast": 1, "fast_iterated": 2, "fast_resummed": 3}.get(variant, variant)
        self._ck(self._lib.t2d_set_integrator_variant(self._h, int(v)))

    def set_outputs(self, velocity=True, applied=True):
        """Which pure output columns the integrators store (t2d_set_outputs): vx / vy of the single-track models
        and the applied action.  Both on = the reference's State; a point mass's velocity is state and always stored."""
        self._ck(self._lib.t2d_set_outputs(self._h, (L.OUT_VELOCITY if velocity else 0) | (L.OUT_APPLIED if applied else 0)))

    # ---------------------------------------------------------------- state
    def reset(self, x, y, heading, speed, type_id, active=None, vx=None, vy=None, env_mask=None):
        n = self.n
        a = [_arr(v, np.float32, n, k) for k, v in (("x", x), ("y", y), ("heading", heading), ("speed", speed))]
        vx_ = _arr(vx, np.float32, n, "vx"); vy_ = _arr(vy, np.float32, n, "vy")
        tid = _arr(type_id, np.uint8, n, "type_id")
        act = _arr(np.ones(n, np.uint8) if active is None else active, np.uint8, n, "active")
        mask = _arr(env_mask, np.uint8, self.n_env, "env_mask")
        self._ck(self._lib.t2d_reset(self._h, _p(mask), _p(a[0]), _p(a[1]), _p(a[2]), _p(a[3]),
                                     _p(vx_), _p(vy_), _p(tid), _p(act)))

    def upload(self, field, values):
        dt = np.dtype(L.FIELD_DTYPES[field])
        v = np.ascontiguousarray(values, dt)
        self._ck(self._lib.t2d_upload(self._h, field, _p(v), v.nbytes))

    def download(self, field):
        dt = np.dtype(L.FIELD_DTYPES[field])
        n = self.n_env if field in L.PER_ENV_FIELDS else self.n
        if field == L.F_LIDAR:
            ptr, nb = self.field_ptr(field)
            out = np.empty((n, nb // (4 * n)), dt)
        elif field == L.F_STATUS:
            out = np.empty((n, 4), dt)
        elif field == L.F_RECORD:
            out = np.empty((L.RECORD_RING, n, 2), dt)
        else:
            out = np.empty(n, dt)
        self._ck(self._lib.t2d_download(self._h, field, _p(out), out.nbytes))
        return out

    def set_actions(self, act0, act1):
        self.upload(L.F_ACT0, act0)
        self.upload(L.F_ACT1, act1)

    def bind_actions(self, act0_ptr=None, act1_ptr=None, stride=1, extent=None):
        """Zero-copy actions from caller-owned device memory (raw pointers, e.g. tensor.data_ptr()); participant i reads
        element i * stride of each (a policy's [N, 2] (steering, accel) tensor: act0 = ptr + 4, act1 = ptr, stride = 2).
        extent = elements readable behind each pointer (an action ring of K sets: K * N * stride): `step_n` then refuses a
        fragment that would read past it instead of faulting on the device (t2d_set_action_extent)."""
        if stride == 1:
            self._ck(self._lib.t2d_bind_actions(self._h, act0_ptr, act1_ptr))
        else:
            self._ck(self._lib.t2d_bind_actions_strided(self._h, act0_ptr, act1_ptr, int(stride)))
        if extent is not None and act0_ptr is not None:
            self._ck(self._lib.t2d_set_action_extent(self._h, int(extent)))

    def field_ptr(self, field):
        ptr, nb = C.c_void_p(), C.c_size_t()
        self._ck(self._lib.t2d_get_field(self._h, field, C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def device_array(self, field):
        """Object exposing __cuda_array_interface__ (zero-copy) for torch.as_tensor."""
        ptr, nb = self.field_ptr(field)
        dt = np.dtype(L.FIELD_DTYPES[field])
        shape = (nb // 4, 4) if field == L.F_STATUS else (L.RECORD_RING, nb // (8 * L.RECORD_RING), 2) if field == L.F_RECORD else \
            (self.n_env, nb // (4 * self.n_env)) if field == L.F_LIDAR else (nb // dt.itemsize,)
        return _DevArray(ptr, shape, dt.str, self)

    # ---------------------------------------------------------------- the hot path
    def integrate(self, interval_ms=100, stream=None):
        self._ck(self._lib.t2d_integrate(self._h, int(interval_ms), stream))

    def collide(self, stream=None):
        self._ck(self._lib.t2d_collide(self._h, stream))

    def check_status(self, interval_ms=100, stream=None):
        self._ck(self._lib.t2d_check_status(self._h, int(interval_ms), stream))

    def step(self, interval_ms=100, stream=None):
        self._ck(self._lib.t2d_step(self._h, int(interval_ms), stream))

    def step_n(self, n_steps, interval_ms=100, act_step_stride=0, stream=None):
        """n_steps consecutive steps enqueued by one call (t2d_step_n): step k reads the action of participant i at
        act[i * stride + k * act_step_stride]; 0 repeats one action set.  Same results as n_steps `step` calls."""
        self._ck(self._lib.t2d_step_n(self._h, int(interval_ms), int(n_steps), int(act_step_stride), stream))

    def set_split_step(self, on=True):
        """Small pools of 33..64-agent envs: one env per workgroup, its event stages on four waves (t2d_set_split_step)."""
        self._ck(self._lib.t2d_set_split_step(self._h, int(bool(on))))

    STEP_FORMS = ("unfused", "step", "step_split", "ego", "ego_loop", "chain", "chain_split", "loop", "loop_pipe", "ego_loop_pipe")

    def step_form(self, n_steps=1):
        """Name of the step-kernel form a call of n_steps steps takes on this pool now (t2d_step_form)."""
        rc = self._lib.t2d_step_form(self._h, int(n_steps))
        if rc < 0:
            raise ValueError("t2d_step_form: null pool")
        return self.STEP_FORMS[rc]

    def set_step_chaining(self, on=True, priority_rule=1):
        """on: False / True, or (measurements, tests) 2 = always the chained form, 3 = small pools loop without the
        integrator waves (t2d_set_step_chaining)"""
        self._ck(self._lib.t2d_set_step_chaining(self._h, int(on), int(priority_rule)))

    def snapshot(self):
        """Record the current state as the episode start for device-side resets."""
        self._ck(self._lib.t2d_snapshot(self._h))

    def restore(self, done_only=False, stream=None):
        """Device-side reset to the snapshot: all envs, or only terminated/truncated ones."""
        self._ck(self._lib.t2d_restore(self._h, 1 if done_only else 0, stream))

    def set_fused_step(self, on=True):
        """step() as one fused launch (default) or as integrate + check_status (two launches)."""
        self._ck(self._lib.t2d_set_fused_step(self._h, int(bool(on))))

    def set_ego_kernel(self, on=True):
        """single-ego pools: one wave per env (default) or the general one-lane-per-participant kernel"""
        self._ck(self._lib.t2d_set_ego_kernel(self._h, int(bool(on))))

    def set_auto_reset(self, on=True):
        """Fuse the reset of finished envs (to the snapshot) into every step()."""
        self._ck(self._lib.t2d_set_auto_reset(self._h, int(bool(on))))

    def sync(self):
        self._ck(self._lib.t2d_sync(self._h))

    # ---------------------------------------------------------------- multi-GPU result gather
    @staticmethod
    def comm_unique_id():
        """ncclGetUniqueId (rank 0): 128 bytes for the other ranks' comm_init, shipped by the launcher's own channel."""
        from . import _ffi
        buf = (C.c_uint8 * 128)()
        _ffi.check(_ffi.lib().t2d_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id, rank, world):
        """ncclCommInitRank on this pool's device (collective).  unique_id None = a world of one without RCCL."""
        buf = None if unique_id is None else (C.c_uint8 * 128).from_buffer_copy(unique_id)
        self._ck(self._lib.t2d_comm_init(self._h, buf, int(rank), int(world)))
        self._comm_id = buf

    def gather(self, n_steps, out_ptr, stream=None, comm=None):
        """All-gather of the per-env result records of the last n_steps steps into caller-owned device memory
        (u32 [world][n_steps][n_env][2]); asynchronous, ordered after `stream`."""
        self._ck(self._lib.t2d_gather(self._h, comm, int(n_steps), out_ptr, stream))

    def gather_wait(self, stream=None, block_host=False):
        self._ck(self._lib.t2d_gather_wait(self._h, stream, int(bool(block_host))))

    def comm_info(self):
        """(native_rccl, world, rank) read back from the pool's communicator (ncclCommCount / ncclCommUserRank when RCCL
        created one): what a multi-GPU run prints as proof that RCCL saw N ranks."""
        a, b, c = C.c_int32(), C.c_int32(), C.c_int32()
        self._ck(self._lib.t2d_comm_info(self._h, C.byref(a), C.byref(b), C.byref(c)))
        return bool(a.value), b.value, c.value

    def step_count(self):
        """Steps taken so far (t2d_step_count): what t2d_gather's fragment length must divide."""
        return int(self._lib.t2d_step_count(self._h))

    def step_occupancy(self):
        """(resident workgroups per CU, LDS bytes per workgroup) of the fused step kernel with this pool's geometry."""
        b, l, g = C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self._lib.t2d_step_occupancy(self._h, C.byref(b), C.byref(l), C.byref(g)))
        return b.value, l.value

    def geometry_bytes_per_launch(self):
        """bytes of packed geometry records (polygons, boxes, lane-union boundary pieces) one step launch stages into LDS"""
        b, l, g = C.c_int32(), C.c_int64(), C.c_int64()
        self._ck(self._lib.t2d_step_occupancy(self._h, C.byref(b), C.byref(l), C.byref(g)))
        return g.value

    # ---------------------------------------------------------------- profiling
    def profile_enable(self, on=True):
        self._ck(self._lib.t2d_profile_enable(self._h, int(bool(on))))

    def profile_read(self, kernel_id):
        ms, n = C.c_double(), C.c_int64()
        self._ck(self._lib.t2d_profile_read(self._h, kernel_id, C.byref(ms), C.byref(n)))
        return ms.value, n.value
