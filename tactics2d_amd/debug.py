"""Test and measurement hooks (include/t2d_debug.h) -- NOT part of the product.

Everything here runs on libt2d_hip_debug.so: the product's sources built with -DT2D_DEBUG_HOOKS plus t2d_loop.hip
(`python -m tactics2d_amd.build --debug-lib`; `__graft_entry__.build()` builds it next to the product).  It exports the whole
product ABI as well, and a pool belongs to the library that created it: `pool()` / `env_groups()` below make pools there.
Loaded by tests/, bench.py's closed_loop leg and scripts/; no product module imports this one (tests/test_layout.py), and
libt2d_hip.so exports no t2d_debug_* symbol.

    pool(n_env, A)                    a ParticipantPool living in the debug library
    set_step_placement(pool, map)     which logical workgroup / wave rotation each physical workgroup of a step launch takes
    chain_fault(pool, kind)           break one hand-off of the chained t2d_step_n on purpose
    set_step_shape64(pool, on)        keep the plain forms on their generic instantiations / last_step_shape() tells which ran
    delay_gather(pool, us)            hold the pool's gather stream (a slow peer)
    feedback_policy(pool, act, ...)   the stand-in policy kernel
    env_groups(scene, G) / ClosedLoop policy kernel -> t2d_step per env group, enqueued by one C call
    math(fn, a, b=None, table=False)  one device function of csrc/t2d_math.h over arrays (tests/test_gpu_math.py)
    geom(fn, a, b=None)               one device predicate of csrc/t2d_geom_dev.h over arrays (tests/test_gpu_geom.py)
    wave_scan(counts)                 the step kernel's prefix sum of 64 candidate counts (tests/test_gpu_wave_scan.py)
"""
import ctypes as C
import os

import numpy as np

from . import _ffi
from .pipeline import EnvGroups
from .pool import ParticipantPool


_vp = C.c_void_p
# every symbol include/t2d_debug.h declares: test / measurement hooks, exported by libt2d_hip_debug.so ONLY (tactics2d_amd/debug.py)
DEBUG_LIB_PATH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "libt2d_hip_debug.so")
DEBUG_SYMBOLS = {
    "t2d_debug_set_step_placement": (C.c_int, [_vp, C.POINTER(C.c_uint32), C.c_int32]),
    "t2d_debug_chain_fault": (C.c_int, [_vp, C.c_int32]),
    "t2d_debug_delay_gather": (C.c_int, [_vp, C.c_int32]),
    "t2d_debug_feedback_policy": (C.c_int, [_vp, _vp, C.c_float, C.c_float, C.c_float, _vp]),
    "t2d_debug_closed_loop_create": (C.c_int, [_vp, _vp, _vp, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.POINTER(_vp)]),
    "t2d_debug_closed_loop_run": (C.c_int, [_vp, C.c_int32]),
    "t2d_debug_closed_loop_destroy": (C.c_int, [_vp]),
    "t2d_debug_last_step_kernel": (C.c_char_p, []),
    "t2d_debug_last_step_shape": (C.c_int, []),
    "t2d_debug_set_step_shape64": (C.c_int, [_vp, C.c_int32]),
    "t2d_debug_math": (C.c_int, [C.c_int32, C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "t2d_debug_geom": (C.c_int, [C.c_int32, C.c_int32, C.c_int64, _vp, _vp, _vp]),
    "t2d_debug_memory": (C.c_int, [C.POINTER(C.c_int64)]),
    "t2d_debug_wave_scan": (C.c_int, [C.c_int32, C.c_int32, _vp, _vp, _vp]),
}

_debug_lib = None


def lib():
    """libt2d_hip_debug.so: everything libt2d_hip.so exports + the hooks of include/t2d_debug.h; a pool belongs to the
    library that created it."""
    global _debug_lib
    if _debug_lib is None:
        _debug_lib = _ffi._load(DEBUG_LIB_PATH, {**_ffi.SYMBOLS, **DEBUG_SYMBOLS}, " --debug-lib")
    return _debug_lib


def pool(n_env, max_agents=1, device_id=0):
    return ParticipantPool(n_env, max_agents, device_id, library=lib())


def env_groups(scene, groups, device_id=0, raw_streams=False):
    return EnvGroups(scene, groups, device_id, raw_streams, library=lib())


def _need(p):
    if p._lib is not lib():
        raise ValueError("this pool lives in libt2d_hip.so, which has no test hooks: create it with tactics2d_amd.debug.pool(...)")


def set_step_placement(p, wgmap=None):
    """Which logical workgroup (and wave rotation << 16) each physical workgroup of the step launch steps; None = identity.
    Never changes a result (t2d_debug.h: t2d_debug_set_step_placement)."""
    _need(p)
    if wgmap is None:
        p._ck(p._lib.t2d_debug_set_step_placement(p._h, None, 0))
        return
    m = np.ascontiguousarray(wgmap, np.uint32)
    p._ck(p._lib.t2d_debug_set_step_placement(p._h, m.ctypes.data_as(C.POINTER(C.c_uint32)), int(m.size)))


def chain_fault(p, kind):
    """t2d_debug_chain_fault: the CHAIN launches of step_n break one hand-off on purpose -- 1: a foreign XCC id in the word,
    2: a word that never comes, 3: a foreign XCC id at step 0; 0: off."""
    _need(p)
    p._ck(p._lib.t2d_debug_chain_fault(p._h, int(kind)))


def delay_gather(p, microseconds):
    """t2d_debug_delay_gather: one idle wave holds the pool's gather stream for that long"""
    _need(p)
    p._ck(p._lib.t2d_debug_delay_gather(p._h, int(microseconds)))


def memory():
    """t2d_debug_memory: (device bytes, device blocks, pinned bytes, pinned blocks) this library holds right now"""
    out = (C.c_int64 * 4)()
    assert lib().t2d_debug_memory(out) == 0
    return tuple(out)


def last_step_kernel():
    """template arguments of the collide_kernel instantiation the last launch took, e.g. "(true, 1, false, true)\""""
    return lib().t2d_debug_last_step_kernel().decode()


def last_step_shape():
    """64: the last launch took the twin of its form compiled for envs of 64 participants, four per workgroup; 0: the generic one"""
    return int(lib().t2d_debug_last_step_shape())


def set_step_shape64(p, on):
    """t2d_debug_set_step_shape64: False keeps the pool's plain step / chained step on the generic instantiations"""
    _need(p)
    p._ck(p._lib.t2d_debug_set_step_shape64(p._h, int(bool(on))))


def feedback_policy(p, act_out_ptr, v_target, k_speed, k_steer, stream=None):
    """t2d_debug_feedback_policy: the stand-in policy, one launch; act_out_ptr = device f32 [N][2] (steering, accel)"""
    _need(p)
    p._ck(p._lib.t2d_debug_feedback_policy(p._h, act_out_ptr, v_target, k_speed, k_steer, stream))


# t2d_debug_math's fn (include/t2d_debug.h: T2D_MATH_*) -> number of outputs
MATH_FUNCTIONS = {"sincos": (0, 2), "sincos_small": (1, 2), "sincos_steer": (2, 2), "sincos_steer_and": (3, 4), "tan": (4, 1),
                  "atan": (5, 1), "atan2": (6, 1), "mod_two_pi": (7, 1), "log": (8, 1), "exp": (9, 1), "pow": (10, 1),
                  "fresnel": (12, 2)}


def math(fn, a, b=None, table=False, device_id=0):
    """t2d_debug_math: the device function `fn` of csrc/t2d_math.h (a key of MATH_FUNCTIONS, or a raw T2D_MATH_* value) over the
    fp64 array a (and b: sincos_steer_and's heading, atan2's x, pow's exponent).  Element i runs in lane i % 64 of wave i // 64.
    table=True: the T2D_TRIG_TABLE compilation.  Returns fp64 [outputs, n] -- [n] for a function with one output."""
    code, nout = MATH_FUNCTIONS[fn] if fn in MATH_FUNCTIONS else (int(fn), 4)
    a = np.ascontiguousarray(a, np.float64).reshape(-1)
    if b is not None:
        b = np.ascontiguousarray(b, np.float64).reshape(-1)
        if b.size != a.size:
            raise ValueError("a and b differ in length")
    out = np.empty((nout, a.size), np.float64)
    rc = lib().t2d_debug_math(int(device_id), code, int(table), a.size, a.ctypes.data, None if b is None else b.ctypes.data,
                              out.ctypes.data)
    _ffi.check(rc, None, lib())
    return out[0] if nout == 1 else out


# t2d_debug_geom's fn (include/t2d_debug.h: T2D_GEOM_*) -> (code, components of a, components of b, outputs)
GEOM_FUNCTIONS = {"sat_quads": (0, 8, 8, 1), "rect_pair_filter": (1, 8, 8, 1), "rect_vs_convex_filter": (2, 8, 8, 1),
                  "point_in_quad": (3, 8, 2, 1), "seg_dist2": (4, 6, 0, 1), "piece_meets_quad_interior": (5, 8, 4, 1),
                  "iou_terms": (6, 8, 8, 10)}
GEOM_MAX_N = 65536


def geom(fn, a, b=None, device_id=0):
    """t2d_debug_geom: the device predicate `fn` of csrc/t2d_geom_dev.h (a key of GEOM_FUNCTIONS) over fp64 arrays, one element
    per row: a = [n, 8] quads x0 y0 .. x3 y3 (seg_dist2: [n, 6] = p, q, c), b = [n, 8] quads, [n, 2] points or [n, 4] pieces (the
    header's table).  Element i runs in lane i % 64 of wave i // 64.  Returns fp64 [n] -- [10, n] for iou_terms."""
    code, na, nb, nout = GEOM_FUNCTIONS[fn]
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, na).T)
    n = a.shape[1]
    if nb:
        b = np.ascontiguousarray(np.asarray(b, np.float64).reshape(-1, nb).T)
        if b.shape[1] != n:
            raise ValueError("a and b differ in length")
    out = np.empty((nout, n), np.float64)
    rc = lib().t2d_debug_geom(int(device_id), code, n, a.ctypes.data, b.ctypes.data if nb else None, out.ctypes.data)
    _ffi.check(rc, None, lib())
    return out[0] if nout == 1 else out


def wave_scan(counts, device_id=0):
    """t2d_debug_wave_scan: the step kernel's wave_excl_scan (csrc/t2d_collide.hip) on one wave per row of `counts` (int32
    [n_waves, 64], or [64]).  Returns (offsets int32 like counts, totals int32 [n_waves] -- a scalar for one row)."""
    c = np.ascontiguousarray(counts, np.int32)
    if c.ndim not in (1, 2) or c.shape[-1] != 64:
        raise ValueError("counts must be [64] or [n_waves, 64]")
    c2 = c.reshape(-1, 64)
    off = np.empty_like(c2)
    total = np.empty(c2.shape[0], np.int32)
    rc = lib().t2d_debug_wave_scan(int(device_id), c2.shape[0], c2.ctypes.data, off.ctypes.data, total.ctypes.data)
    _ffi.check(rc, None, lib())
    return (off[0], int(total[0])) if c.ndim == 1 else (off, total)


class ClosedLoop:
    """The closed loop a policy-driven caller runs -- per env group and step: policy kernel -> t2d_step, no host
    synchronisation -- enqueued `n` iterations at a time by one C call (t2d_debug_closed_loop_*, t2d_loop.hip).  The policy is
    the library's stand-in (per-participant state feedback, a few flops): what is timed is the step path under a real
    dependency -- step k + 1 of a group cannot start before its policy has read step k's state -- not a network.

    launcher: "thread" (the calling thread goes round the groups), "threads" (one host thread per group) or "graph" (one
    captured hipGraph of `graph_steps` iterations per group, replayed).  Results equal those of the same policy and t2d_step
    calls on one pool holding all the envs (tests/test_gpu_closed_loop.py)."""
    LAUNCHERS = {"thread": 0, "threads": 1, "graph": 2}

    def __init__(self, groups, launcher="thread", interval_ms=100, graph_steps=64):
        import torch
        self.groups, self.launcher = groups, launcher
        self._lib = lib()
        if any(p._lib is not self._lib for p in groups.pools):
            raise ValueError("ClosedLoop needs env groups created on libt2d_hip_debug.so: debug.env_groups(...)")
        dev = torch.device("cuda", groups.device_id)
        # one [n_g, 2] (steering, accel) tensor per group: what a policy network would return for the group's participants
        self.actions = [torch.zeros((p.n, 2), dtype=torch.float32, device=dev) for p in groups.pools]
        torch.cuda.synchronize(dev)
        G = groups.groups
        vp = C.c_void_p * G
        self._h = C.c_void_p()
        rc = self._lib.t2d_debug_closed_loop_create(vp(*[p._h for p in groups.pools]), vp(*[s.cuda_stream for s in groups.streams]),
                                                    vp(*[a.data_ptr() for a in self.actions]), G, int(interval_ms),
                                                    self.LAUNCHERS[launcher], int(graph_steps), C.byref(self._h))
        if rc:
            for p in groups.pools:
                if self._lib.t2d_last_error(p._h):
                    _ffi.check(rc, p._h, self._lib)
            _ffi.check(rc, None, self._lib)

    def run(self, n_steps):
        """enqueue n_steps iterations of (policy, step) on every group; returns when everything is enqueued"""
        rc = self._lib.t2d_debug_closed_loop_run(self._h, int(n_steps))
        if rc:
            for p in self.groups.pools:
                if self._lib.t2d_last_error(p._h):
                    _ffi.check(rc, p._h, self._lib)
            _ffi.check(rc, None, self._lib)

    def close(self):
        if self._h:
            self.groups.sync()
            self._lib.t2d_debug_closed_loop_destroy(self._h)
            self._h = None
