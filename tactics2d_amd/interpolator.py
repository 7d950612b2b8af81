"""Reeds-Shepp curves for batches of queries on the device (tactics2d/interpolator/reeds_shepp.py).

`ReedsShepp(radius).get_all_path(...)` is the reference's method of that name for n queries in one launch of
t2d_rs_paths (include/t2d.h): the 48 slots of the reference's list, in its order, as device tensors.  The point lists of
ReedsSheppPath.get_curve_line are not provided.  There is no CPU path: without a device the calls raise T2DError.
"""
import ctypes as C
import functools

import numpy as np

from . import _ffi, layout as L

_LETTER = {1: "L", -1: "R", 0: "S"}
_CURVE = ("CSC", "CCC", "CCCC", "CCSC", "CCSCC")


def slot_tables(library=None):
    """letters int8 [48, 5] (+1 L, -1 R, 0 S), signs int8 [48, 5], n_seg int32 [48], curve_type int32 [48]: the library's own
    slot table (t2d_rs_slot_info), the one the kernels read."""
    lib = library if library is not None else _ffi.lib()
    letters, signs = np.zeros((L.RS_SLOTS, L.RS_MAX_SEGMENTS), np.int8), np.zeros((L.RS_SLOTS, L.RS_MAX_SEGMENTS), np.int8)
    n_seg, ctype = np.zeros(L.RS_SLOTS, np.int32), np.zeros(L.RS_SLOTS, np.int32)
    for s in range(L.RS_SLOTS):
        n, c = C.c_int32(), C.c_int32()
        _ffi.check(lib.t2d_rs_slot_info(s, letters[s].ctypes.data_as(C.c_void_p), signs[s].ctypes.data_as(C.c_void_p),
                                        C.byref(n), C.byref(c)), None, lib)
        n_seg[s], ctype[s] = n.value, c.value
    return letters, signs, n_seg, ctype


@functools.lru_cache(None)
def _tables():
    """the slot tables and the words / curve types made of them, read from the library on first use"""
    letters, signs, n_seg, ctype = slot_tables()
    words = tuple("".join(_LETTER[int(v)] for v in letters[s, :n_seg[s]]) for s in range(L.RS_SLOTS))
    return dict(LETTERS=letters, SIGNS=signs, N_SEG=n_seg, WORDS=words, CURVE_TYPES=tuple(_CURVE[int(c)] for c in ctype))


class _SlotTables(type):
    """ReedsShepp.WORDS, .CURVE_TYPES, .LETTERS, .SIGNS, .N_SEG as class attributes that load the library on first access"""
    WORDS = property(lambda cls: _tables()["WORDS"])
    CURVE_TYPES = property(lambda cls: _tables()["CURVE_TYPES"])
    LETTERS = property(lambda cls: _tables()["LETTERS"])
    SIGNS = property(lambda cls: _tables()["SIGNS"])
    N_SEG = property(lambda cls: _tables()["N_SEG"])


class RSPaths:
    """What get_all_path returns: device tensors, one row per query.
    valid bool [n, 48]; segments float64 [n, 48, 5] = signs * segments of the slot's ReedsSheppPath in units of the radius, zero
    padded (all zero where the reference's list holds None); length float64 [n, 48] in metres, +inf for None; shortest int32
    [n] = get_path's slot (the last of equal shortest lengths); shortest_first int32 [n] = the lowest-index shortest one; -1
    where no slot is a path.  mask int64 [n]: bit s = valid[:, s]."""

    def __init__(self, mask, segments, length, shortest, radius):
        import torch
        self.mask, self.segments, self.length, self.radius = mask, segments, length, radius
        self.shortest, self.shortest_first = shortest[:, 0], shortest[:, 1]
        self.valid = ((mask[:, None] >> torch.arange(L.RS_SLOTS, device=mask.device)) & 1).bool()
        self.WORDS, self.CURVE_TYPES = ReedsShepp.WORDS, ReedsShepp.CURVE_TYPES


class RSPath:
    """What get_path returns: per query the chosen slot (-1: none), its signed segments [n, 5], steer signs [n, 5] (+1 L, -1 R,
    0 S), n_seg [n] and length [n] (+inf without a path), as device tensors."""

    def __init__(self, slot, segments, steer, n_seg, length):
        self.slot, self.segments, self.steer, self.n_seg, self.length = slot, segments, steer, n_seg, length


class ReedsShepp(metaclass=_SlotTables):
    """ReedsShepp (reeds_shepp.py:142-156) for batches.  WORDS / CURVE_TYPES: the word ("LSL", ...) and the curve type ("CSC",
    ...) of each of the 48 slots; LETTERS / SIGNS / N_SEG the same table as arrays (on the class; read from the library on first
    access)."""

    def __init__(self, radius, device_id=0):
        self.radius = float(radius)
        if not self.radius > 0:
            raise ValueError("The minimum turning radius must be positive.")
        self.device_id = int(device_id)

    def _poses(self, points, headings):
        """[n, 3] float64 (x, y, heading) on the device.  A contiguous float64 CUDA tensor [n, 3] with headings None is what the
        kernel reads, in place; separate points / headings (tensors or numpy) are packed into a new device tensor."""
        import torch
        dev = torch.device("cuda", self.device_id)
        if headings is None:
            if isinstance(points, torch.Tensor):
                p = points.to(dev, torch.float64).contiguous()   # (the same tensor when it already is all of that)
            else:
                p = torch.as_tensor(np.ascontiguousarray(points, np.float64)).to(dev)
            if p.ndim != 2 or p.shape[1] != 3:
                raise ValueError("packed poses must be [n, 3] (x, y, heading)")
            return p
        if isinstance(points, torch.Tensor) and isinstance(headings, torch.Tensor):
            p, h = points.to(dev, torch.float64).reshape(-1, 2), headings.to(dev, torch.float64).reshape(-1, 1)
        else:
            p = torch.as_tensor(np.asarray(points, np.float64).reshape(-1, 2)).to(dev)
            h = torch.as_tensor(np.asarray(headings, np.float64).reshape(-1, 1)).to(dev)
        if p.shape[0] != h.shape[0]:
            raise ValueError("points and headings must have one row per query")
        return torch.cat([p, h], 1)

    def get_all_path(self, start_points, start_headings, end_points, end_headings, stream=None):
        """start_points / end_points [n, 2] with start_headings / end_headings [n], numpy or torch: packed into [n, 3] device
        tensors (one upload or one device copy each).  Or packed poses: start_points / end_points float64 CUDA tensors [n, 3]
        (x, y, heading) with the headings None -- those are read in place, nothing is copied.  Asynchronous on `stream` (a torch
        stream; default: the current one); the inputs must stay alive and unchanged until the launch has run."""
        import torch
        lib = _ffi.lib()
        try:
            dev = torch.device("cuda", self.device_id)
            st = stream if stream is not None else torch.cuda.current_stream(dev)
        except (RuntimeError, AssertionError) as exc:
            raise _ffi.T2DError(_ffi.ERR_HIP, f"no usable HIP device: {exc}") from None
        with torch.cuda.stream(st):
            start, goal = self._poses(start_points, start_headings), self._poses(end_points, end_headings)
            n = start.shape[0]
            if goal.shape[0] != n:
                raise ValueError("start and end must have the same number of queries")
            mask = torch.empty(n, dtype=torch.int64, device=dev)
            seg = torch.empty((n, L.RS_SLOTS, L.RS_MAX_SEGMENTS), dtype=torch.float64, device=dev)
            length = torch.empty((n, L.RS_SLOTS), dtype=torch.float64, device=dev)
            short = torch.empty((n, 2), dtype=torch.int32, device=dev)
            _ffi.check(lib.t2d_rs_paths(self.device_id, n, self.radius, start.data_ptr(), goal.data_ptr(), mask.data_ptr(),
                                        seg.data_ptr(), length.data_ptr(), short.data_ptr(), st.cuda_stream), None, lib)
            out = RSPaths(mask, seg, length, short, self.radius)
            out._inputs = (start, goal)   # (kept alive with the result)
            return out

    def get_path(self, start_points, start_headings, end_points, end_headings, stream=None):
        """The shortest path of each query by the reference's rule (get_path :529-558: the last of equal shortest lengths)."""
        import torch
        r = self.get_all_path(start_points, start_headings, end_points, end_headings, stream)
        dev = r.mask.device
        k = r.shortest.long().clamp(min=0)
        rows = torch.arange(k.shape[0], device=dev)
        none = r.shortest < 0
        letters = torch.as_tensor(_tables()["LETTERS"], device=dev)[k]
        n_seg = torch.as_tensor(_tables()["N_SEG"], device=dev)[k]
        zero = none[:, None]
        return RSPath(r.shortest, r.segments[rows, k].masked_fill(zero, 0.0), letters.masked_fill(zero, 0),
                      n_seg.masked_fill(none, 0), r.length[rows, k].masked_fill(none, float("inf")))
