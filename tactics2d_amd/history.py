"""Histories of a batch of participants: `BatchedTrajectory` on the host (opt-in, scope row a7) and `DeviceTrajectory`, recorded
and kept on the device.

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
            self.pool._lib.t2d_traj_destroy(self._h)
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
