"""Histories of a batch of participants: `BatchedTrajectory` on the host (opt-in, scope row a7), `DeviceTrajectory`, recorded
and kept on the device, and `ReplaySource`: a recorded history that participants of a pool are replayed from inside the step.

The device pool keeps only the CURRENT state: the reference's per-participant frame -> State dictionary
(`tactics2d.participant.trajectory.Trajectory`, participant/trajectory/trajectory.py:12-188) grows without bound and is exactly
the Python object churn the batched path removes.  A caller who does want the history records whole-batch snapshots:

* `BatchedTrajectory` keeps `BatchedState` objects on the host (`record` downloads six columns per step);
* `DeviceTrajectory` keeps them in a t2d_traj buffer on the pool's device (include/t2d.h): `record` is one stream-ordered
  launch, states are materialised as `BatchedState`s only when asked for, and `ParticipantPool.verify_states` /
  `model.verify_states` check the whole history in one launch (physics_model_base.py:53-73).

Both follow the reference's rules -- which exception for which misuse, when `stable_freq` drops, what `reset` keeps -- through
one piece of frame bookkeeping (`FrameBook`), restated for a batch.
"""
import ctypes as C
import logging
import weakref

import numpy as np

from . import layout as L
from .physics import BatchedState

_log = logging.getLogger(__name__)


class FrameBook:
    """The reference Trajectory's frame bookkeeping (trajectory.py:115-149) over opaque handles: the stamps in insertion order
    (duplicates included), frame -> handle, the current handle and `stable_freq`.  BatchedTrajectory's handles are the states
    themselves, DeviceTrajectory's are slots of its device buffer.  Pure Python."""

    def __init__(self, id_, stable_freq=True):
        self.id_, self.stable_freq = id_, stable_freq
        self.stamps = []         # frames in insertion order (ms)
        self.by_frame = {}       # frame -> handle
        self.now = None

    def add(self, frame, handle):
        """add_state once the state is known to be one: a repeated frame overwrites (with a warning), a frame before the last one
        raises KeyError, an interval change clears `stable_freq` (with a warning)."""
        if frame in self.by_frame:
            # (the reference overwrites BEFORE it checks the order, :131-135: a repeated frame that also lies before the last one
            # replaces the stored state and THEN raises -- found by replaying the reference: tests/golden/trajectory_kats.json)
            self.by_frame[frame] = handle
            _log.warning("trajectory %s: state at time stamp %s overwritten", self.id_, frame)
        if self.stamps and frame < self.stamps[-1]:
            raise KeyError(f"trajectory {self.id_}: time stamp {frame} lies before the last one ({self.stamps[-1]})")
        uneven = len(self.by_frame) > 1 and frame - self.stamps[-1] != self.stamps[-1] - self.stamps[-2]
        if uneven and self.stable_freq:
            self.stable_freq = False
            _log.warning("trajectory %s: uneven time interval", self.id_)
        self.stamps.append(frame)
        self.by_frame[frame] = self.now = handle

    def edge(self, i):
        return self.by_frame[self.stamps[i]] if self.stamps else None

    def get(self, frame):
        try:
            return self.by_frame[frame]
        except KeyError:
            raise KeyError(f"trajectory {self.id_}: no state at time stamp {frame}") from None

    def clear(self):
        self.stamps, self.by_frame = [], {}


def verify_intervals(trajectory):
    """The interval `PhysicsModelBase.verify_states` (physics_model_base.py:63-71) passes for each frame after the first, computed
    as the reference does: `1000 / fps` (a float) for a stable-frequency trajectory, `frame_k - frame_0` otherwise.  Its
    errors are the reference's: TypeError for a stable trajectory without fps (`1000 / None`), IndexError for an empty one
    (`frames[0]`).  Duplicated stamps stay in the list."""
    if trajectory.stable_freq is True:
        interval = 1000 / trajectory.fps
    first = trajectory.frames[0]
    out = []
    for frame in trajectory.frames[1:]:
        interval = interval if trajectory.stable_freq else frame - first
        out.append(interval)
    return out


class _TrajectoryBase:
    """The public surface shared by both histories (names as in the reference); subclasses say how a handle becomes a state."""

    def __init__(self, id_, fps=None, stable_freq=True):
        self.id_, self.fps = id_, fps
        self._book = FrameBook(id_, stable_freq)

    stable_freq = property(lambda self: self._book.stable_freq, lambda self, v: setattr(self._book, "stable_freq", v))

    def _state(self, handle):
        raise NotImplementedError

    def __len__(self):
        return len(self._book.stamps)

    @property
    def frames(self):
        return self._book.stamps

    @property
    def history_states(self):
        return {f: self._state(h) for f, h in self._book.by_frame.items()}

    def _edge(self, i):
        h = self._book.edge(i)
        return None if h is None else self._state(h)

    initial_state = property(lambda self: self._edge(0))
    last_state = property(lambda self: self._edge(-1))
    first_frame = property(lambda self: self._book.stamps[0] if self._book.stamps else None)
    last_frame = property(lambda self: self._book.stamps[-1] if self._book.stamps else None)

    def has_state(self, frame):
        return frame in self._book.by_frame

    def get_state(self, frame=None):
        if frame is None:
            return None if self._book.now is None else self._state(self._book.now)
        return self._state(self._book.get(frame))

    def get_trace(self, frame_range=None):
        """[(x[n], y[n]), ...] of the frames inside [start, end] (the whole history by default) (:151-168)."""
        lo, hi = (self.first_frame, self.last_frame) if frame_range is None else frame_range
        return [self._state(self._book.by_frame[f]).location for f in self._book.stamps if lo <= f <= hi]


class BatchedTrajectory(_TrajectoryBase):
    """Host history: frame -> BatchedState."""

    def _state(self, handle):
        return handle

    @property
    def history_states(self):
        return self._book.by_frame

    @property
    def average_speed(self):
        """float64[n]: per participant, the mean speed over the recorded frames (:85-87)."""
        return np.stack([np.asarray(s.speed, np.float64) for s in self._book.by_frame.values()]).mean(0)

    # ---- mutation ----------------------------------------------------------------------------------
    def add_state(self, state):
        """Append a snapshot (:115-149): ValueError for a non-state, KeyError for a frame before the last one,
        a repeated frame overwrites (with a warning), an interval change clears `stable_freq` (with a warning)."""
        if not isinstance(state, BatchedState):
            raise ValueError("add_state expects a BatchedState")
        self._book.add(state.frame, state)

    def reset(self, state=None, keep_history=False):
        """(:170-188) no state: back to the initial state, history dropped unless keep_history;
        with a state: history dropped, the state becomes the only entry."""
        first = self.initial_state if state is None else state
        if state is None and keep_history:
            self._book.now = first
            return
        self._book.clear()
        self.add_state(first)

    def record(self, pool, frame):
        """Append the pool's current state (one download per column) as the state of `frame`."""
        col = pool.download
        self.add_state(BatchedState(frame, col(L.F_X), col(L.F_Y), col(L.F_HEADING), col(L.F_VX), col(L.F_VY),
                                    speed=col(L.F_SPEED)))
        return self._book.now


def _state_columns(state, n):
    """the six fp32 columns a slot holds (x, y, heading, speed, vx, vy) of a host BatchedState: the velocity and speed as the
    state derives them (0 where it has none)"""
    z = np.zeros(n, np.float32)
    v = state.velocity
    sp = state.speed
    cols = (state.x, state.y, state.heading, z if sp is None else sp, z if v is None else v[0], z if v is None else v[1])
    return np.stack([np.broadcast_to(np.asarray(c, np.float32), (n,)) for c in cols])


class _DevArray:
    """Zero-copy view for `torch.as_tensor(..., device='cuda')` (as ParticipantPool.device_array); keeps its buffer alive."""

    def __init__(self, ptr, shape, owner):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": "<f4", "data": (ptr, False), "version": 2, "strides": None}
        self._owner = owner


class _TrajBuffer:
    """One t2d_traj of `capacity` slots bound to `pool` (include/t2d.h).  Freed by close(), by the pool's close(), or when the
    last reference (a DeviceTrajectory, a column view) goes."""

    def __init__(self, pool, capacity):
        self.pool, self.capacity, self.n = pool, int(capacity), pool.n
        self._h = C.c_void_p()
        pool._ck(pool._lib.t2d_traj_create(pool._h, self.capacity, C.byref(self._h)))
        reg = pool.__dict__.setdefault("_traj_buffers", weakref.WeakSet())
        reg.add(self)

    def close(self):
        if getattr(self, "_h", None) is not None and self._h:
            # (refused -- T2DError, ERR_STATE -- while a pool still replays this buffer: pool.replay_unbind() first)
            self.pool._ck(self.pool._lib.t2d_traj_destroy(self._h))
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _live(self):
        if not self._h:
            raise ValueError("the trajectory buffer is closed (or its pool is)")
        return self._h

    def write(self, slot, cols):
        cols = np.ascontiguousarray(cols, np.float32)
        self.pool._ck(self.pool._lib.t2d_traj_write(self._live(), int(slot), cols.ctypes.data_as(C.c_void_p)))

    def read(self, slot):
        out = np.empty((L.TRAJ_COLS, self.n), np.float32)
        self.pool._ck(self.pool._lib.t2d_traj_read(self._live(), int(slot), out.ctypes.data_as(C.c_void_p)))
        return out

    def record(self, slot, stream=None):
        self.pool._ck(self.pool._lib.t2d_traj_record(self._live(), int(slot), stream))

    def column_ptr(self, col):
        ptr, nb = C.c_void_p(), C.c_size_t()
        self.pool._ck(self.pool._lib.t2d_traj_column(self._live(), int(col), C.byref(ptr), C.byref(nb)))
        return ptr.value, nb.value

    def rows(self, col, n_rows):
        """host copy of rows [0, n_rows) of one column"""
        import torch
        self.pool.sync()
        ptr, _ = self.column_ptr(col)
        view = _DevArray(ptr, (self.capacity, self.n), self)
        return torch.as_tensor(view, device=f"cuda:{self.pool.device_id}")[:n_rows].cpu().numpy()

    def grown(self, capacity, n_slots, stream=None):
        """a buffer of `capacity` slots holding this one's first n_slots (one device-to-device copy)"""
        new = _TrajBuffer(self.pool, capacity)
        new.copy_from(self, n_slots, stream)
        return new

    def copy_from(self, src, n_slots, stream=None):
        self.pool._ck(self.pool._lib.t2d_traj_copy(self._live(), src._live(), int(n_slots), stream))


class DeviceTrajectory(_TrajectoryBase):
    """The reference's Trajectory for every participant of `pool`, recorded and kept on the pool's device.

    Same surface and rules as BatchedTrajectory.  A state lives in a slot of a t2d_traj buffer: a new frame takes the next free
    slot, a repeated frame reuses its slot (a fresh one only where the reference would keep the old state as the current one),
    a reset that drops the history starts again from slot 0.  A full buffer is replaced by one of twice the capacity (one
    device-to-device copy), so the object is as unbounded as the reference's.  States come back to the host only on demand:
    `get_state` / `history_states` materialise a BatchedState with one t2d_traj_read each."""

    def __init__(self, pool, id_, fps=None, stable_freq=True, capacity=64, _storage=None):
        super().__init__(id_, fps, stable_freq)
        self.pool = pool
        self._buf = _storage if _storage is not None else _TrajBuffer(pool, capacity)
        self.n = self._buf.n
        self._n_used = 0          # slots [0, _n_used) may be referenced
        self._slot_frame = {}     # slot -> frame of the state it holds

    @classmethod
    def from_batched(cls, pool, traj, capacity=None):
        """a DeviceTrajectory on `pool` holding a BatchedTrajectory's states (one upload per distinct frame) and bookkeeping"""
        frames = list(traj.history_states)
        dev = cls(pool, traj.id_, traj.fps, traj.stable_freq, capacity=max(1, capacity or len(frames)))
        for s, f in enumerate(frames):
            dev._buf.write(s, _state_columns(traj.history_states[f], dev.n))
            dev._slot_frame[s] = f
        slot_of = {f: s for s, f in enumerate(frames)}
        dev._book.stamps = list(traj.frames)
        dev._book.by_frame = dict(slot_of)
        now = traj.get_state()
        dev._book.now = None if now is None else slot_of.get(now.frame)
        dev._n_used = len(frames)
        return dev

    def copy_to(self, pool):
        """a DeviceTrajectory on another pool of the same size and device (one device-to-device copy)"""
        dev = DeviceTrajectory(pool, self.id_, self.fps, self.stable_freq, capacity=max(1, self._n_used))
        dev._buf.copy_from(self._buf, self._n_used)
        dev._book.stamps, dev._book.by_frame, dev._book.now = list(self._book.stamps), dict(self._book.by_frame), self._book.now
        dev._slot_frame, dev._n_used = dict(self._slot_frame), self._n_used
        return dev

    def close(self):
        self._buf.close()

    @property
    def capacity(self):
        return self._buf.capacity

    def _state(self, slot):
        c = self._buf.read(slot)
        return BatchedState(self._slot_frame[slot], c[0], c[1], c[2], c[4], c[5], speed=c[3])

    @property
    def average_speed(self):
        """float64[n]: per participant, the mean speed over the recorded frames (:85-87)."""
        sp = self._buf.rows(L.TRAJ_SPEED, self._n_used)
        return np.stack([np.asarray(sp[s], np.float64) for s in self._book.by_frame.values()]).mean(0)

    def column(self, name):
        """zero-copy [slots in use, N] fp32 view (row k = slot k: for a trajectory without overwritten or reset frames, the k-th
        distinct frame) with __cuda_array_interface__, valid while the view is held"""
        col = {"x": L.TRAJ_X, "y": L.TRAJ_Y, "heading": L.TRAJ_HEADING, "speed": L.TRAJ_SPEED, "vx": L.TRAJ_VX,
               "vy": L.TRAJ_VY}[name]
        ptr, _ = self._buf.column_ptr(col)
        return _DevArray(ptr, (self._n_used, self.n), self._buf)

    def traces(self):
        """host copy of the recorded (x, y) of every participant: float32 [slots in use, N, 2], row k = slot k (tests; the
        device-side counterpart is set_routes_from)"""
        return np.stack([self._buf.rows(L.TRAJ_X, self._n_used), self._buf.rows(L.TRAJ_Y, self._n_used)], -1)

    def set_routes_from(self, pool, route_of=None, threshold=0.0, src_env=None, windows=None):
        """Make this recording the routes of `pool`'s off-route detector without touching the host: participant (e, a) follows
        the recorded trace of participant (src_env[e], route_of) -- its own by default (pool.set_routes_from)."""
        pool.set_routes_from(self, src_env, windows, route_of, threshold)

    def slots(self):
        """int32[len(frames)]: the slot of each stamp (duplicates resolve to the overwritten state, as the reference's dict)"""
        return np.array([self._book.by_frame[f] for f in self._book.stamps], np.int32)

    # ---- mutation ----------------------------------------------------------------------------------
    def _slot_for(self, frame, stream=None):
        b = self._book
        s = b.by_frame.get(frame)
        # a repeated frame reuses its slot -- unless that slot is also the current state and the frame lies early: the reference
        # then keeps the OLD state as the current one while the dictionary takes the new one
        if s is not None and not (s == b.now and b.stamps and frame < b.stamps[-1]):
            return s
        s = self._n_used
        if s >= self._buf.capacity:
            self._buf = self._buf.grown(2 * self._buf.capacity, self._n_used, stream)
        return s

    def _commit(self, frame, slot):
        try:
            self._book.add(frame, slot)
        finally:
            if self._book.by_frame.get(frame) == slot:
                self._slot_frame[slot] = frame
                self._n_used = max(self._n_used, slot + 1)

    def add_state(self, state):
        """Append a host BatchedState (one upload): the reference's rules, as BatchedTrajectory.add_state."""
        if not isinstance(state, BatchedState):
            raise ValueError("add_state expects a BatchedState")
        if len(state) != self.n:
            raise ValueError(f"add_state: a state of {len(state)} participants for a trajectory of {self.n}")
        slot = self._slot_for(state.frame)
        self._buf.write(slot, _state_columns(state, self.n))
        self._commit(state.frame, slot)

    def record(self, pool, frame, stream=None):
        """Append the pool's current state as the state of `frame`: one launch on `stream`, no host sync (a record enqueued after a
        step on the same stream sees that step's state).  Returns the slot."""
        if pool is not self.pool:
            raise ValueError("record: a DeviceTrajectory records the pool it was created on")
        frame = int(frame)
        slot = self._slot_for(frame, stream)
        self._buf.record(slot, stream)
        self._commit(frame, slot)
        return slot

    def reset(self, state=None, keep_history=False):
        """(:170-188) no state: back to the initial state, history dropped unless keep_history;
        with a state: history dropped, the state becomes the only entry.  The kept state moves to slot 0."""
        b = self._book
        if state is None and keep_history:
            b.now = b.edge(0)
            return
        if state is not None or not b.stamps:
            b.clear()
            self._n_used = 0
            self.add_state(state)   # (None on an empty trajectory: ValueError, as the reference's add_state(None))
            return
        f0, s0 = b.stamps[0], b.by_frame[b.stamps[0]]
        if s0 != 0:
            self._buf.write(0, self._buf.read(s0))
        b.clear()
        self._n_used = 0
        self._commit(f0, 0)


class _ReplayedParticipant:
    """One participant of a ReplaySource, answering as the reference's ParticipantBase does (participant_base.py:166-203)."""

    def __init__(self, source, j):
        self._src, self._j = source, int(j)

    @property
    def first_frame(self):
        s, j = self._src, self._j
        return None if s.first_slot[j] > s.last_slot[j] else s.t0_ms + int(s.first_slot[j]) * s.period_ms

    @property
    def last_frame(self):
        s, j = self._src, self._j
        return None if s.first_slot[j] > s.last_slot[j] else s.t0_ms + int(s.last_slot[j]) * s.period_ms

    def is_active(self, frame):
        # (the reference's two comparisons, :175 -- a participant without a single state raises its TypeError: `frame < None`)
        if frame < self.first_frame or frame > self.last_frame:
            return False
        return True

    def get_state(self, frame):
        """BatchedState of one participant; KeyError (:201-202) for a stamp the recording does not hold: outside the window
        or off the grid."""
        s, j = self._src, self._j
        k, r = divmod(frame - s.t0_ms, s.period_ms)
        if r != 0 or not (s.first_slot[j] <= k <= s.last_slot[j]):
            raise KeyError(f"Time stamp {frame} is not found in the trajectory {j}.")
        c = s.slot_states(int(k))[j]
        return BatchedState(int(frame), c[0], c[1], c[2], c[4], c[5], speed=c[3])


class ReplaySource:
    """A recorded history on a uniform stamp grid that participants of a pool are replayed from (pool.replay_bind; model
    layout.MODEL_REPLAY): slot k holds the states of stamp t0_ms + k * period_ms of n_src_env x max_agents source
    participants, participant j being present in slots [first_slot[j], last_slot[j]] (first > last: never) -- the reference's
    `first_frame <= frame <= last_frame` (participant_base.py:166-177).  The states live in a t2d_traj on the device (a
    DeviceTrajectory's own buffer, or one uploaded into a pool that serves as the library); a source built from host data
    without a pool answers is_active / get_state on the host and is uploaded by `upload(pool_like)`."""

    def __init__(self, n_src_env, max_agents, n_slots, t0_ms, period_ms, first_slot=None, last_slot=None, states=None, buf=None,
                 owner=None):
        self.n_src_env, self.max_agents, self.n_slots = int(n_src_env), int(max_agents), int(n_slots)
        self.n = self.n_src_env * self.max_agents
        self.t0_ms, self.period_ms = int(t0_ms), int(period_ms)
        if self.period_ms < 1:
            raise ValueError("ReplaySource: period_ms must be >= 1")
        if self.n_slots < 1:
            raise ValueError("ReplaySource: a source holds at least one slot")
        if self.t0_ms % self.period_ms:
            raise ValueError(f"ReplaySource: t0_ms {self.t0_ms} is not a multiple of period_ms {self.period_ms} (env time starts "
                             "at 0: no step could land on a stamp)")
        first = np.zeros(self.n, np.int32) if first_slot is None else np.ascontiguousarray(first_slot, np.int32).reshape(-1)
        last = np.full(self.n, self.n_slots - 1, np.int32) if last_slot is None else \
            np.ascontiguousarray(last_slot, np.int32).reshape(-1)
        if first.size != self.n or last.size != self.n:
            raise ValueError(f"ReplaySource: windows of {first.size} / {last.size} participants for a source of {self.n}")
        if ((first < 0) | (first >= self.n_slots) | (last < 0) | (last >= self.n_slots)).any():
            raise ValueError(f"ReplaySource: a window slot outside [0, {self.n_slots})")
        self.first_slot, self.last_slot = first, last
        self._states = states    # host copy [n_slots, n, 6] float32, or None (device only)
        self._buf = buf          # _TrajBuffer, or None (host only)
        self._owner = owner      # whatever keeps the buffer's pool / trajectory alive

    # ---- constructors ------------------------------------------------------------------------------
    @classmethod
    def from_device(cls, traj, t0_ms, period_ms, windows=None):
        """A DeviceTrajectory recorded with `record` replays as it is: its slots in use must hold the stamps t0_ms, t0_ms +
        period_ms, ... in order.  windows: (first_slot, last_slot) int32 [N] or None = every slot."""
        n_slots = traj._n_used
        for k in range(n_slots):
            if traj._slot_frame.get(k) != int(t0_ms) + k * int(period_ms):
                raise ValueError(f"from_device: slot {k} holds stamp {traj._slot_frame.get(k)}, not {int(t0_ms) + k * int(period_ms)}: "
                                 "the recording does not lie on the grid")
        first, last = (None, None) if windows is None else windows
        pool = traj.pool
        return cls(pool.n_env, pool.max_agents, n_slots, t0_ms, period_ms, first, last, buf=traj._buf, owner=traj)

    @classmethod
    def from_arrays(cls, pool_like, states, first_slot=None, last_slot=None, t0_ms=0, period_ms=40):
        """states float32 [n_slots, n_src_env, max_agents, 6] (x, y, heading, speed, vx, vy; anything where a participant is
        outside its window).  pool_like: a pool of the same max_agents on the device the source shall live on -- it holds the
        buffer itself when it has n_src_env envs, else a library pool of n_src_env envs (never stepped) is created beside
        it; None: a host-only source (`upload` later)."""
        st = np.ascontiguousarray(states, np.float32)
        if st.ndim != 4 or st.shape[3] != L.TRAJ_COLS:
            raise ValueError("from_arrays: states must be [n_slots, n_src_env, max_agents, 6]")
        src = cls(st.shape[1], st.shape[2], st.shape[0], t0_ms, period_ms, first_slot, last_slot,
                  states=st.reshape(st.shape[0], -1, L.TRAJ_COLS))
        return src if pool_like is None else src.upload(pool_like)

    @classmethod
    def from_trajectories(cls, pool_like, trajectories, t0_ms, period_ms, n_slots=None):
        """Pack reference-style per-participant trajectories -- objects with `frames` and `get_state(frame)` whose states
        carry x, y, heading, speed, vx / vy (scalars or one-element columns) -- onto the grid.  trajectories:
        [n_src_env][max_agents] (None or an empty trajectory: a participant the recording never has).  A participant's
        window is [first frame, last frame]; every grid stamp inside it must be in the trajectory (the reference's KeyError,
        participant_base.py:201-202, otherwise), and its first and last frame must lie on the grid (ValueError)."""
        n_src_env, A = len(trajectories), len(trajectories[0])
        t0_ms, period_ms = int(t0_ms), int(period_ms)
        if period_ms < 1:
            raise ValueError("ReplaySource: period_ms must be >= 1")
        spans = []
        for row in trajectories:
            if len(row) != A:
                raise ValueError("from_trajectories: every source env needs the same number of participants")
            for tr in row:
                fr = [] if tr is None else list(tr.frames)
                if not fr:
                    spans.append(None)
                    continue
                lo, hi = min(fr), max(fr)
                if (lo - t0_ms) % period_ms or (hi - t0_ms) % period_ms or lo < t0_ms:
                    raise ValueError(f"from_trajectories: a trajectory spans [{lo}, {hi}] ms, off the grid {t0_ms} + k * {period_ms}")
                spans.append(((lo - t0_ms) // period_ms, (hi - t0_ms) // period_ms))
        need = 1 + max([hi for sp in spans if sp for hi in sp[1:]], default=0)
        n_slots = need if n_slots is None else int(n_slots)
        if n_slots < need:
            raise ValueError(f"from_trajectories: the trajectories need {need} slots, n_slots is {n_slots}")
        st = np.zeros((n_slots, n_src_env * A, L.TRAJ_COLS), np.float32)
        first, last = np.ones(n_src_env * A, np.int32), np.zeros(n_src_env * A, np.int32)   # (first > last: never present)
        flat = [tr for row in trajectories for tr in row]
        for j, (tr, sp) in enumerate(zip(flat, spans)):
            if sp is None:
                continue
            first[j], last[j] = sp
            have = set(tr.frames)
            for k in range(sp[0], sp[1] + 1):
                f = t0_ms + k * period_ms
                if f not in have:
                    raise KeyError(f"Time stamp {f} is not found in the trajectory {getattr(tr, 'id_', j)}.")
                st[k, j] = _scalar_state(tr.get_state(f))
        src = cls(n_src_env, A, n_slots, t0_ms, period_ms, first, last, states=st)
        return src if pool_like is None else src.upload(pool_like)

    # ---- device ------------------------------------------------------------------------------------
    def upload(self, pool_like):
        """Put a host-built source on pool_like's device (see from_arrays); returns self."""
        if self._buf is not None:
            return self
        if pool_like.max_agents != self.max_agents:
            raise ValueError(f"ReplaySource: {self.max_agents} participants per source env, the pool has {pool_like.max_agents}")
        owner = pool_like
        if pool_like.n_env != self.n_src_env:   # a library pool of the source's size, on the same device, never stepped
            owner = type(pool_like)(self.n_src_env, self.max_agents, pool_like.device_id, library=pool_like._lib)
            self._library_pool = owner
        buf = _TrajBuffer(owner, self.n_slots)
        for k in range(self.n_slots):
            buf.write(k, self._states[k].T)
        self._buf, self._owner = buf, owner
        return self

    def device_buffer(self):
        if self._buf is None:
            raise ValueError("the replay source lives on the host only: upload(pool_like) first")
        return self._buf

    def close(self):
        """Free a buffer this source uploaded itself (a DeviceTrajectory's stays its own)."""
        if self._buf is not None and not isinstance(self._owner, DeviceTrajectory):
            self._buf.close()
            self._buf = None
            if getattr(self, "_library_pool", None) is not None:
                self._library_pool.close()
                self._library_pool = None

    # ---- the reference's questions, on the host ----------------------------------------------------------
    def slot_states(self, k):
        """float32 [n, 6] of slot k (one read of the device buffer for a source without a host copy)"""
        if self._states is not None:
            return self._states[k]
        return self._buf.read(k).T

    def traces(self):
        """host copies of every source participant's trace -- `get_trace` over its window: a list of N float32 (k, 2) arrays,
        the (x, y) of slots first_slot[j] .. last_slot[j] in order (k = 0 where first > last)"""
        xy = np.stack([self.slot_states(k)[:, :2] for k in range(self.n_slots)])   # [n_slots, N, 2]
        return [np.ascontiguousarray(xy[self.first_slot[j]:self.last_slot[j] + 1, j], np.float32) for j in range(self.n)]

    def set_routes_from(self, pool, route_of=None, threshold=0.0, src_env=None, windows=None):
        """Make the source's traces the routes of `pool`'s off-route detector, read on the device (pool.set_routes_from: the
        source's windows, and the src_env of the pool's replay binding of this source, unless given)."""
        pool.set_routes_from(self, src_env, windows, route_of, threshold)

    def participant(self, j, src_env=0):
        return _ReplayedParticipant(self, int(src_env) * self.max_agents + int(j))

    def is_active(self, j, frame, src_env=0):
        return self.participant(j, src_env).is_active(frame)

    def get_state(self, j, frame, src_env=0):
        return self.participant(j, src_env).get_state(frame)

    def slot_of(self, stamp_ms):
        """the slot holding stamp_ms (array or scalar), -1 before t0_ms -- floor on the grid, as the kernel computes it"""
        d = np.asarray(stamp_ms, np.int64) - self.t0_ms
        return np.where(d < 0, -1, d // self.period_ms)

    def active_mask(self, stamp_ms, src_env=None):
        """bool [n_env, max_agents]: the window rule for env e showing source env src_env[e] at stamp stamp_ms[e] (scalar: all)"""
        se = np.arange(self.n_src_env) if src_env is None else np.asarray(src_env, np.int64)
        k = np.broadcast_to(self.slot_of(stamp_ms), se.shape)[:, None]
        first = self.first_slot.reshape(self.n_src_env, self.max_agents)[se]
        last = self.last_slot.reshape(self.n_src_env, self.max_agents)[se]
        return (k >= first) & (k <= last) & (k < self.n_slots)


def _scalar_state(s):
    """x, y, heading, speed, vx, vy of one participant's state (a reference State or a one-element BatchedState), as the
    pool stores them: the velocity and speed as the state derives them"""
    one = lambda v: 0.0 if v is None else float(np.asarray(v, np.float64).reshape(-1)[0])
    v = getattr(s, "velocity", None)
    vx, vy = (s.vx, s.vy) if getattr(s, "vx", None) is not None and getattr(s, "vy", None) is not None else \
        (v if v is not None else (None, None))
    return np.array([one(s.x), one(s.y), one(s.heading), one(s.speed), one(vx), one(vy)], np.float32)
