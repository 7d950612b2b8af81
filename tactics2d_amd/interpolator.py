"""Reeds-Shepp and Dubins curves for batches of queries, and Bezier, B-spline and cubic spline curves for batches of control
polygons, on the device (tactics2d/interpolator/reeds_shepp.py, dubins.py, bezier.py, b_spline.py, cubic_spline.py); Spiral and
ParamPoly3 curves (spiral.py, param_poly3.py) and, on top of them, the plan-view reference lines of OpenDRIVE roads
(map/parser/parse_xodr.py): `Spiral`, `ParamPoly3`, `pack_planview`, `planview_lines`.

`ReedsShepp(radius).get_all_path(...)` is the reference's method of that name for n queries in one launch of
t2d_rs_paths (include/t2d.h): the 48 slots of the reference's list, in its order, as device tensors.  `Dubins(radius)` is the
same for the six Dubins words (t2d_dubins_paths).  `get_curve(...)` of either class samples the shortest path of every query into
the point list of the reference's get_curve_line (t2d_curve_lines); `curve_lines(...)` is that call for words of the caller's own.
`Bezier`, `BSpline` and `CubicSpline` have the reference's get_curve for n control polygons in one launch of t2d_spline_curves.
There is no CPU path: without a device the calls raise T2DError.
"""
import ctypes as C
import enum
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


def _stream_of(device_id, stream):
    """(torch device, torch stream) a call works on: `stream`, or the device's current one"""
    import torch
    try:
        dev = torch.device("cuda", device_id)
        return dev, stream if stream is not None else torch.cuda.current_stream(dev)
    except (RuntimeError, AssertionError) as exc:
        raise _ffi.T2DError(_ffi.ERR_HIP, f"no usable HIP device: {exc}") from None


class CurveLines:
    """What curve_lines / get_curve return: device tensors, one row per curve.  xy float64 [n, max_points, 2] and yaw float64
    [n, max_points]: the first min(count, max_points) rows of a curve are its points, the rest is not written; count int32 [n]:
    the curve's FULL point count (0: no curve; > max_points: truncated); end float64 [n, 3]: the pose after the last segment
    (not written where count is 0); slot int32 [n]: the path each curve was sampled from (get_curve; None for curve_lines)."""

    def __init__(self, xy, yaw, count, end, slot=None):
        self.xy, self.yaw, self.count, self.end, self.slot = xy, yaw, count, end, slot


def pack_words(segments, letters, n_seg):
    """The word records of t2d_curve_lines (layout.CURVE_WORD_BYTES each) as a float64 device tensor [n, 6], made on the device of
    `segments`: segments float64 [n, 5] signed lengths in units of the radius, letters int [n, 5] (+1 L, -1 R, 0 S), n_seg int [n]."""
    import torch
    n = segments.shape[0]
    words = torch.zeros((n, L.CURVE_WORD_BYTES // 8), dtype=torch.float64, device=segments.device)
    words[:, :L.RS_MAX_SEGMENTS] = segments
    tail = words.view(torch.int8).view(n, L.CURVE_WORD_BYTES)
    tail[:, 40:40 + L.RS_MAX_SEGMENTS] = letters.to(torch.int8)
    tail[:, 40 + L.RS_MAX_SEGMENTS] = n_seg.to(torch.int8)
    return words


def curve_lines(words, starts, radius, step_size, rule, max_points, device_id=0, stream=None):
    """t2d_curve_lines: words float64 CUDA tensor [n, 6] (pack_words), starts float64 CUDA tensor [n, 3] (x, y, heading), rule
    layout.CURVE_DUBINS / CURVE_RS (or "dubins" / "rs").  One launch, asynchronous on `stream`.  Returns CurveLines."""
    import torch
    lib = _ffi.lib()
    rule = {"dubins": L.CURVE_DUBINS, "rs": L.CURVE_RS}.get(rule, rule)
    try:
        dev = torch.device("cuda", device_id)
        st = stream if stream is not None else torch.cuda.current_stream(dev)
    except (RuntimeError, AssertionError) as exc:
        raise _ffi.T2DError(_ffi.ERR_HIP, f"no usable HIP device: {exc}") from None
    n = words.shape[0]
    if words.dtype != torch.float64 or tuple(words.shape) != (n, L.CURVE_WORD_BYTES // 8) or not words.is_contiguous():
        raise ValueError("words must be a contiguous float64 [n, 6] tensor (pack_words)")
    if starts.dtype != torch.float64 or tuple(starts.shape) != (n, 3) or not starts.is_contiguous():
        raise ValueError("starts must be a contiguous float64 [n, 3] tensor")
    max_points = int(max_points)
    with torch.cuda.stream(st):
        rows = max(max_points, 0)
        xy = torch.empty((n, rows, 2), dtype=torch.float64, device=dev)
        yaw = torch.empty((n, rows), dtype=torch.float64, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        end = torch.empty((n, 3), dtype=torch.float64, device=dev)
        _ffi.check(lib.t2d_curve_lines(device_id, n, words.data_ptr(), starts.data_ptr(), float(radius), float(step_size), int(rule),
                                       max_points, xy.data_ptr(), yaw.data_ptr(), count.data_ptr(), end.data_ptr(), st.cuda_stream),
                   None, lib)
    out = CurveLines(xy, yaw, count, end)
    out._inputs = (words, starts)   # (kept alive with the result)
    return out


def default_max_points(radius, step_size, reach):
    """A point budget for get_curve: a shortest path between poses at most `reach` metres apart is shorter than reach + 7 pi
    radius (three arcs of a full turn and a half at the very most), one point per step and two per segment on top."""
    return int(np.ceil((float(reach) + 7.0 * np.pi * float(radius)) / float(step_size))) + 2 * L.RS_MAX_SEGMENTS


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
        """The shortest path of each query by the reference's rule (get_path :529-558: the last of equal shortest lengths).  The
        launch and the gather behind it are both enqueued on `stream`."""
        import torch
        dev, st = _stream_of(self.device_id, stream)
        with torch.cuda.stream(st):
            r = self.get_all_path(start_points, start_headings, end_points, end_headings, st)
            k = r.shortest.long().clamp(min=0)
            rows = torch.arange(k.shape[0], device=dev)
            none = r.shortest < 0
            letters = torch.as_tensor(_tables()["LETTERS"], device=dev)[k]
            n_seg = torch.as_tensor(_tables()["N_SEG"], device=dev)[k]
            zero = none[:, None]
            out = RSPath(r.shortest, r.segments[rows, k].masked_fill(zero, 0.0), letters.masked_fill(zero, 0),
                         n_seg.masked_fill(none, 0), r.length[rows, k].masked_fill(none, float("inf")))
        out._inputs = r._inputs
        return out

    def get_curve(self, start_points, start_headings, end_points, end_headings, step_size=0.01, max_points=None, stream=None):
        """ReedsShepp.get_curve (:560-585): get_path's choice of every query sampled by ReedsSheppPath.get_curve_line (:46-139) at
        the reference's default step.  max_points None: default_max_points for poses up to 64 m apart (at the default step some
        16 000 points, 0.4 MB, per query: pass a budget that fits the scene).  The gather from (segments, slot) to words is torch
        ops on the device; both launches and those ops are enqueued on `stream`.  Returns CurveLines (count 0 where no slot is a
        path)."""
        import torch
        _, st = _stream_of(self.device_id, stream)
        if max_points is None:
            max_points = default_max_points(self.radius, step_size, 64.0)
        with torch.cuda.stream(st):
            path = self.get_path(start_points, start_headings, end_points, end_headings, st)
            words = pack_words(path.segments, path.steer, path.n_seg)
            out = curve_lines(words, path._inputs[0], self.radius, step_size, L.CURVE_RS, max_points, self.device_id, st)
        out.slot = path.slot
        return out


def dubins_slot_table(library=None):
    """letters int8 [6, 3] (+1 L, -1 R, 0 S): the library's own table of the six Dubins words (t2d_dubins_slot_info)"""
    lib = library if library is not None else _ffi.lib()
    letters = np.zeros((L.DUBINS_SLOTS, 3), np.int8)
    for s in range(L.DUBINS_SLOTS):
        _ffi.check(lib.t2d_dubins_slot_info(s, letters[s].ctypes.data_as(C.c_void_p)), None, lib)
    return letters


@functools.lru_cache(None)
def _dubins_tables():
    letters = dubins_slot_table()
    return dict(LETTERS=letters, WORDS=tuple("".join(_LETTER[int(v)] for v in row) for row in letters))


class _DubinsTables(type):
    """Dubins.WORDS, .LETTERS as class attributes that load the library on first access"""
    WORDS = property(lambda cls: _dubins_tables()["WORDS"])
    LETTERS = property(lambda cls: _dubins_tables()["LETTERS"])


class DubinsPaths:
    """What Dubins.get_all_path returns: device tensors, one row per query.
    valid bool [n, 6]; segments float64 [n, 6, 3] = (t, p, q) of the slot's DubinsPath in units of the radius (zero where the
    reference's list holds None); length float64 [n, 6] in metres, +inf for None; shortest int32 [n] = get_path's slot (the last
    of equal shortest lengths); shortest_first int32 [n] = the lowest-index shortest one; -1 where no slot is a path.  mask uint8
    [n]: bit s = valid[:, s]."""

    def __init__(self, mask, segments, length, shortest, radius):
        import torch
        self.mask, self.segments, self.length, self.radius = mask, segments, length, radius
        self.shortest, self.shortest_first = shortest[:, 0], shortest[:, 1]
        self.valid = ((mask[:, None].to(torch.int32) >> torch.arange(L.DUBINS_SLOTS, device=mask.device, dtype=torch.int32)) & 1).bool()
        self.WORDS = Dubins.WORDS


class DubinsPath:
    """What Dubins.get_path returns: per query the chosen slot (-1: none), its segments [n, 3], steer signs [n, 3] (+1 L, -1 R,
    0 S), n_seg [n] (3, or 0 without a path) and length [n] (+inf without a path), as device tensors."""

    def __init__(self, slot, segments, steer, n_seg, length):
        self.slot, self.segments, self.steer, self.n_seg, self.length = slot, segments, steer, n_seg, length


class Dubins(metaclass=_DubinsTables):
    """Dubins (dubins.py:107-331) for batches.  WORDS: the word of each of the six slots, LETTERS the same as an array (on the
    class; read from the library on first access).  lrl: "reference" keeps Dubins._LRL (:216-231) as written -- its curve misses
    the goal, DESIGN.md 4.18 --, "standard" (build-defined) corrects the sign of its `tmp` term and changes nothing else."""

    LRL_RULES = {"reference": 0, "standard": 1}
    _poses = ReedsShepp._poses

    def __init__(self, radius, lrl="reference", device_id=0):
        self.radius = float(radius)
        if not self.radius > 0:
            raise ValueError("The minimum turning radius must be positive.")
        if lrl not in self.LRL_RULES:
            raise ValueError(f"lrl must be one of {sorted(self.LRL_RULES)}")
        self.lrl = lrl
        self.device_id = int(device_id)

    def get_all_path(self, start_points, start_headings, end_points, end_headings, stream=None):
        """The input conventions of ReedsShepp.get_all_path: points [n, 2] with headings [n] (numpy or torch), or packed float64
        CUDA tensors [n, 3] with the headings None, read in place.  Asynchronous on `stream`.  Returns DubinsPaths."""
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
            mask = torch.empty(n, dtype=torch.uint8, device=dev)
            seg = torch.empty((n, L.DUBINS_SLOTS, 3), dtype=torch.float64, device=dev)
            length = torch.empty((n, L.DUBINS_SLOTS), dtype=torch.float64, device=dev)
            short = torch.empty((n, 2), dtype=torch.int32, device=dev)
            _ffi.check(lib.t2d_dubins_paths(self.device_id, n, self.radius, start.data_ptr(), goal.data_ptr(),
                                            self.LRL_RULES[self.lrl], mask.data_ptr(), seg.data_ptr(), length.data_ptr(),
                                            short.data_ptr(), st.cuda_stream), None, lib)
            out = DubinsPaths(mask, seg, length, short, self.radius)
            out._inputs = (start, goal)   # (kept alive with the result)
            return out

    def get_path(self, start_points, start_headings, end_points, end_headings, stream=None):
        """The shortest path of each query by the reference's rule (get_path :275-304: the last of equal shortest lengths).  The
        launch and the gather behind it are both enqueued on `stream`."""
        import torch
        dev, st = _stream_of(self.device_id, stream)
        with torch.cuda.stream(st):
            r = self.get_all_path(start_points, start_headings, end_points, end_headings, st)
            k = r.shortest.long().clamp(min=0)
            rows = torch.arange(k.shape[0], device=dev)
            none = r.shortest < 0
            letters = torch.as_tensor(_dubins_tables()["LETTERS"], device=dev)[k]
            out = DubinsPath(r.shortest, r.segments[rows, k].masked_fill(none[:, None], 0.0), letters.masked_fill(none[:, None], 0),
                             torch.full_like(r.shortest, 3).masked_fill(none, 0), r.length[rows, k].masked_fill(none, float("inf")))
        out._inputs = r._inputs
        return out

    def get_curve(self, start_points, start_headings, end_points, end_headings, step_size=0.1, max_points=None, stream=None):
        """Dubins.get_curve (:306-331): get_path's choice of every query sampled by DubinsPath.get_curve_line (:28-104) at the
        reference's default step.  max_points None: default_max_points for poses up to 64 m apart.  The gather from (segments,
        slot) to words is torch ops on the device; both launches and those ops are enqueued on `stream`.  Returns CurveLines
        (count 0 where no slot is a path)."""
        import torch
        _, st = _stream_of(self.device_id, stream)
        if max_points is None:
            max_points = default_max_points(self.radius, step_size, 64.0)
        with torch.cuda.stream(st):
            path = self.get_path(start_points, start_headings, end_points, end_headings, st)
            pad = torch.zeros((path.segments.shape[0], L.RS_MAX_SEGMENTS - 3), dtype=torch.float64, device=path.segments.device)
            words = pack_words(torch.cat([path.segments, pad], 1), torch.cat([path.steer, pad.to(torch.int8)], 1), path.n_seg)
            out = curve_lines(words, path._inputs[0], self.radius, step_size, L.CURVE_DUBINS, max_points, self.device_id, st)
        out.slot = path.slot
        return out


# ---- Bezier, B-spline and cubic spline curves (t2d_spline_curves) ----------------------------------------------------------------
class SplineCurves:
    """What Bezier / BSpline / CubicSpline.get_curve return: device tensors, one row per control polygon.  xy float64
    [n, max_points, 2]: the first min(count, max_points) rows of a curve are its points, the rest is not written; count int32 [n]:
    the curve's FULL point count (0: no curve -- too few control points in the row, abscissae that do not increase, knots that
    decrease, an input that is not finite; > max_points: truncated)."""

    def __init__(self, xy, count):
        self.xy, self.count = xy, count


SPLINE_KINDS = {"bezier": L.SPLINE_BEZIER, "bspline": L.SPLINE_BSPLINE, "cubic": L.SPLINE_CUBIC}
_SHAPE_MESSAGE = "Control points should have shape (n, 2)."


def _is_tensor(x):
    import torch
    return isinstance(x, torch.Tensor)


def _used(values, used):
    """numpy [n, k] with the entries past each row's `used` count replaced by the row's last used one (their differences are 0)"""
    v = np.asarray(values, np.float64)
    idx = np.minimum(np.arange(v.shape[1])[None, :], np.maximum(np.asarray(used).reshape(-1, 1) - 1, 0))
    return np.take_along_axis(v, idx, 1)


def spline_check(kind, control_points, n_ctrl=None, n_interpolation=100, degree=0, knot_vectors=None,
                 boundary_type=L.SPLINE_NOT_A_KNOT, first_derivatives=None):
    """The host side of a t2d_spline_curves / t2d_spline_routes call: every check that needs no device, raising the reference's
    ValueError with its message (bezier.py:29-39, b_spline.py:39-51, cubic_spline.py:56-75 and the invalid_argument of the
    compiled module); data-dependent ones (increasing x, non-decreasing knots) only for numpy inputs -- for device tensors those
    rows come back with count 0.  Returns (kind, n, m, n_interpolation, degree, boundary_type, full point count of an m-point row)."""
    kind = SPLINE_KINDS.get(kind, kind)
    if kind not in SPLINE_KINDS.values():
        raise ValueError(f"kind must be one of {sorted(SPLINE_KINDS)}")
    shape = tuple(control_points.shape) if hasattr(control_points, "shape") else np.asarray(control_points).shape
    if len(shape) not in (2, 3) or shape[-1] != 2:
        raise ValueError(_SHAPE_MESSAGE)
    n, m = (1, shape[0]) if len(shape) == 2 else shape[:2]
    n_interpolation, degree = int(n_interpolation), int(degree)
    if kind == L.SPLINE_BSPLINE:
        if degree < 0:
            raise ValueError("Degree must be non-negative.")
        expected = m + degree + 1
        if knot_vectors is not None:
            kshape = tuple(knot_vectors.shape)
            if kshape not in ((n, expected), (expected,)) or (len(kshape) == 1 and n != 1):
                raise ValueError(f"Expected {expected} knots, got {kshape[-1] if kshape else 0}.")
            if not _is_tensor(knot_vectors):
                k = np.asarray(knot_vectors, np.float64).reshape(n, expected)
                if n_ctrl is not None and not _is_tensor(n_ctrl):
                    k = _used(k, np.asarray(n_ctrl) + degree + 1)
                if np.any(np.diff(k, axis=1) < 0):
                    raise ValueError("Knot vector must be non-decreasing.")
        if m < degree + 1:
            raise ValueError("Number of control points must be at least degree + 1.")
        if n_interpolation <= 0:
            raise ValueError("Number of interpolation points must be positive.")
        if degree > L.SPLINE_MAX_DEGREE:
            raise ValueError(f"degree {degree} is above the device cap of {L.SPLINE_MAX_DEGREE}")
    elif kind == L.SPLINE_CUBIC:
        names = ", ".join(CubicSpline.BoundaryType.__members__)
        try:
            boundary_type = CubicSpline.BoundaryType(boundary_type)
        except ValueError:
            raise ValueError(f"Invalid boundary type: {boundary_type}. Available options are: {names} or an integer value from 1 to "
                             f"{len(CubicSpline.BoundaryType.__members__)}.") from None
        if m < 3:
            raise ValueError("Need at least 3 control points.")
        if not _is_tensor(control_points):
            x = np.asarray(control_points, np.float64).reshape(n, m, 2)[:, :, 0]
            d = np.diff(x, axis=1)
            if n_ctrl is not None and not _is_tensor(n_ctrl):
                d = np.where(np.arange(1, m)[None, :] < np.asarray(n_ctrl).reshape(-1, 1), d, 1.0)
            if np.any(d <= 0):
                raise ValueError("x-values must be strictly increasing.")
        if n_interpolation < 2:
            raise ValueError("Number of interpolation points must be at least 2.")
        boundary_type = boundary_type.value
    elif n_interpolation < 2:
        raise ValueError("n_interpolation must be greater than or equal to 2.")
    if m > L.SPLINE_MAX_CTRL:
        raise ValueError(f"{m} control points are above the device cap of {L.SPLINE_MAX_CTRL}")
    if n_ctrl is not None and tuple(n_ctrl.shape) != (n,):
        raise ValueError(f"n_ctrl must have shape ({n},)")
    if first_derivatives is not None and tuple(np.shape(first_derivatives)) not in ((2,), (n, 2)):
        raise ValueError(f"first_derivatives must be a pair or have shape ({n}, 2)")
    full = (m - 1) * n_interpolation + 1 if kind == L.SPLINE_CUBIC else n_interpolation
    return kind, n, m, n_interpolation, degree, boundary_type if kind == L.SPLINE_CUBIC else 0, full


def spline_inputs(dev, n, m, control_points, n_ctrl, knot_vectors, first_derivatives):
    """The device tensors of a launch: ctrl float64 [n, m, 2], n_ctrl int32 [n], knots float64 [n, m + degree + 1] or None,
    derivs float64 [n, 2] or None.  A contiguous float64 CUDA tensor is used in place, anything else is uploaded or converted."""
    import torch

    def f64(x, shape):
        if x is None:
            return None
        t = x.to(dev, torch.float64) if _is_tensor(x) else torch.as_tensor(np.ascontiguousarray(x, np.float64)).to(dev)
        return t.reshape(shape).contiguous()

    ctrl = f64(control_points, (n, m, 2))
    if n_ctrl is None:
        n_ctrl = torch.full((n,), m, dtype=torch.int32, device=dev)
    elif _is_tensor(n_ctrl):
        n_ctrl = n_ctrl.to(dev, torch.int32).contiguous()
    else:
        n_ctrl = torch.as_tensor(np.ascontiguousarray(n_ctrl, np.int32)).to(dev)
    knots = f64(knot_vectors, (n, -1))
    derivs = f64(first_derivatives, (-1, 2))
    if derivs is not None and derivs.shape[0] != n:   # (one pair for every row)
        derivs = derivs.expand(n, 2).contiguous()
    return ctrl, n_ctrl, knots, derivs


def _ptr(t):
    return None if t is None else t.data_ptr()


def spline_curves(kind, control_points, n_ctrl=None, n_interpolation=100, degree=0, knot_vectors=None,
                  boundary_type=L.SPLINE_NOT_A_KNOT, first_derivatives=None, max_points=None, device_id=0, stream=None):
    """t2d_spline_curves: the curves of n control polygons of one family ("bezier" / "bspline" / "cubic" or layout.SPLINE_*) in
    one launch, asynchronous on `stream`.  The arguments are those of the three classes below.  Returns SplineCurves."""
    import torch
    kind, n, m, n_interpolation, degree, boundary_type, full = spline_check(kind, control_points, n_ctrl, n_interpolation, degree,
                                                                            knot_vectors, boundary_type, first_derivatives)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    max_points = full if max_points is None else int(max_points)
    with torch.cuda.stream(st):
        ctrl, n_ctrl, knots, derivs = spline_inputs(dev, n, m, control_points, n_ctrl, knot_vectors, first_derivatives)
        xy = torch.empty((n, max(max_points, 0), 2), dtype=torch.float64, device=dev)
        count = torch.empty(n, dtype=torch.int32, device=dev)
        _ffi.check(lib.t2d_spline_curves(device_id, n, kind, ctrl.data_ptr(), n_ctrl.data_ptr(), m, n_interpolation, degree, _ptr(knots),
                                         boundary_type, _ptr(derivs), max_points, xy.data_ptr(), count.data_ptr(), st.cuda_stream),
                   None, lib)
    out = SplineCurves(xy, count)
    out._inputs = (ctrl, n_ctrl, knots, derivs)   # (kept alive with the result)
    return out


class Bezier:
    """Bezier (interpolator/bezier.py) for batches."""

    @staticmethod
    def get_curve(control_points, n_interpolation, order=None, n_ctrl=None, max_points=None, device_id=0, stream=None):
        """Bezier.get_curve (bezier.py:16-44) for n control polygons in one launch.  control_points [n, m, 2], or [m, 2] for a batch
        of one: numpy, or a float64 CUDA tensor (a contiguous one is read in place); n_ctrl int [n] (optional): row e uses its
        first n_ctrl[e] points; n_interpolation >= 2 points per curve; order: None or m - 1, as in the reference.  max_points: the
        rows of the result (default: n_interpolation).  Asynchronous on `stream` (a torch stream; default: the current one).
        Returns SplineCurves.  The reference's ValueErrors are raised with its messages."""
        shape = tuple(control_points.shape) if hasattr(control_points, "shape") else ()
        if len(shape) not in (2, 3) or shape[-1] != 2:
            raise ValueError(_SHAPE_MESSAGE)
        m = shape[-2]
        order = m - 1 if order is None else int(order)
        if order < 1:
            raise ValueError("Order must be greater than or equal to one.")
        if m != order + 1:
            raise ValueError("Number of control points must be equal to order plus one.")
        return spline_curves(L.SPLINE_BEZIER, control_points, n_ctrl, n_interpolation, max_points=max_points, device_id=device_id,
                             stream=stream)


class BSpline:
    """BSpline (interpolator/b_spline.py) for batches."""

    @staticmethod
    def get_curve(control_points, knot_vectors=None, degree=0, n_interpolation=100, n_ctrl=None, max_points=None, device_id=0,
                  stream=None):
        """BSpline.get_curve (b_spline.py:16-57) for n control polygons in one launch; the conventions of Bezier.get_curve.
        knot_vectors [n, m + degree + 1] (or [m + degree + 1] for a batch of one), numpy or a float64 CUDA tensor; None: the
        reference's default, np.linspace(0, 1, n_ctrl + degree + 1) per row, made on the device.  A row of n_ctrl[e] points uses
        its first n_ctrl[e] + degree + 1 knots.  n_interpolation >= 1 points per curve at u_start + j (u_end - u_start) /
        n_interpolation: the curve's end is not among them.  degree <= layout.SPLINE_MAX_DEGREE."""
        return spline_curves(L.SPLINE_BSPLINE, control_points, n_ctrl, n_interpolation, degree, knot_vectors, max_points=max_points,
                             device_id=device_id, stream=stream)


class CubicSpline:
    """CubicSpline (interpolator/cubic_spline.py) for batches."""

    class BoundaryType(enum.Enum):
        """Natural: zero second derivative at both ends; Clamped: the given first derivatives; NotAKnot: the first two and the last
        two cubics are one cubic each."""
        Natural = 1
        Clamped = 2
        NotAKnot = 3

    @staticmethod
    def get_curve(control_points, first_derivatives=(0, 0), n_interpolation=100, boundary_type=BoundaryType.NotAKnot, n_ctrl=None,
                  max_points=None, device_id=0, stream=None):
        """CubicSpline.get_curve (cubic_spline.py:36-84) for n control polygons in one launch; the conventions of Bezier.get_curve.
        y as a function of strictly increasing x; (n_ctrl - 1) * n_interpolation + 1 points per curve, n_interpolation >= 2 per
        segment (the abscissa is accumulated step by step, so a segment's last sample only approximates the next knot, which the
        next segment then repeats exactly).  first_derivatives: a pair for every row or [n, 2], read under Clamped only;
        boundary_type: a BoundaryType or 1 .. 3.  With three control points the NotAKnot system is singular and the curve is, for
        most rows, the polyline through them, as in the reference.  max_points default: (m - 1) *
        n_interpolation + 1."""
        if isinstance(first_derivatives, tuple) and tuple(first_derivatives) == (0, 0):
            first_derivatives = None
        return spline_curves(L.SPLINE_CUBIC, control_points, n_ctrl, n_interpolation, 0, None, boundary_type, first_derivatives,
                             max_points, device_id, stream)


# ---- Spiral and ParamPoly3 curves, plan-view reference lines (t2d_spiral_curves / t2d_param_poly3_curves / t2d_planview_lines) ----
# Not here: ParamPoly3.fit and split_polyline (np.polyfit on the host: not a hot path), lane widths and lane polygons off the
# reference line, and the XML parser itself -- pack_planview takes the attributes of <geometry> elements already parsed.
class RoadCurves:
    """What Spiral / ParamPoly3.get_curve return for a batch: xy float64 [n, max_points, 2]: the first min(count, max_points) rows
    of a curve are its points, the rest is not written; count int32 [n]: the curve's FULL point count (0: no curve -- a value that
    is not finite, a negative length, an unknown p_range; > max_points: truncated).  Device tensors (numpy arrays where nothing
    was launched: n_interpolation == 0)."""

    def __init__(self, xy, count):
        self.xy, self.count = xy, count


class PlanviewLines:
    """What planview_lines returns: device tensors, one row per road.  xy float64 [n, max_points, 2], s and kappa float64
    [n, max_points]: the first min(count, max_points) rows are the road's kept points, their s and their curvature; count int32
    [n]: the FULL number of kept points (0: the road has no line)."""

    def __init__(self, xy, s, kappa, count):
        self.xy, self.s, self.kappa, self.count = xy, s, kappa, count


SPIRAL_RULES = {"reference": L.SPIRAL_REFERENCE, "standard": L.SPIRAL_STANDARD}
P_RANGES = {"normalized": L.P_RANGE_NORMALIZED, "arcLength": L.P_RANGE_ARC_LENGTH}
GEOMETRY_KINDS = {"line": L.GEOM_LINE, "spiral": L.GEOM_SPIRAL, "arc": L.GEOM_ARC, "poly3": L.GEOM_POLY3,
                  "paramPoly3": L.GEOM_PARAM_POLY3}
GEOMETRY_ATTRIBUTES = {"line": (), "spiral": ("curvStart", "curvEnd"), "arc": ("curvature",), "poly3": ("a", "b", "c", "d"),
                       "paramPoly3": ("aU", "bU", "cU", "dU", "aV", "bV", "cV", "dV")}


def _rule(rule):
    rule = SPIRAL_RULES.get(rule, rule)
    if rule not in SPIRAL_RULES.values():
        raise ValueError(f"rule must be one of {sorted(SPIRAL_RULES)}")
    return rule


def _columns(dev, cols):
    """float64 [n, len(cols)] on `dev` from scalars, arrays and tensors of n (or one) values each"""
    import torch
    parts = [c.to(dev, torch.float64).reshape(-1) if _is_tensor(c) else
             torch.as_tensor(np.ascontiguousarray(np.asarray(c, np.float64).reshape(-1))).to(dev) for c in cols]
    n = max(len(p) for p in parts)
    return torch.stack([p.expand(n) if len(p) == 1 else p for p in parts], 1).contiguous()


def _host_values(x):
    return None if _is_tensor(x) else np.asarray(x, np.float64).reshape(-1)


class Spiral:
    """Spiral (interpolator/spiral.py) for batches."""

    @staticmethod
    def get_curve(length, start_point, heading, start_curvature, gamma, n_interpolation=100, rule="reference", max_points=None,
                  device_id=0, stream=None):
        """Spiral.get_curve (spiral.py:15-89).  Scalars (start_point a pair) give one curve as a numpy array (n_interpolation, 2);
        arrays or float64 CUDA tensors of n values (start_point [n, 2]) give n curves in one launch of t2d_spiral_curves as
        RoadCurves, asynchronous on `stream`.  rule "reference": the class as written -- the Euler spiral only for
        start_curvature == 0 and gamma > 0 --; "standard": the clothoid heading + k0 s + gamma s^2 / 2.
        n_interpolation == 0 gives (0, 2) and launches nothing.  The reference's ValueErrors are raised with its messages (a
        negative length inside a device tensor is not looked at: that row comes back with count 0)."""
        import torch
        rule = _rule(rule)
        single = not any(_is_tensor(v) or np.ndim(v) for v in (length, heading, start_curvature, gamma)) and not _is_tensor(start_point) and np.ndim(start_point) == 1
        host = _host_values(length)
        if host is not None and np.any(host < 0):
            raise ValueError("Length must be non-negative.")
        n_interpolation = int(n_interpolation)
        if n_interpolation < 0:
            raise ValueError("Number of interpolation points must be non-negative.")
        if n_interpolation == 0:
            if single:
                return np.empty((0, 2))
            n = max(int(np.prod(v.shape)) if hasattr(v, "shape") else np.size(v) for v in (length, heading, start_curvature, gamma))
            return RoadCurves(np.empty((n, 0, 2)), np.zeros(n, np.int32))
        lib = _ffi.lib()
        dev, st = _stream_of(device_id, stream)
        max_points = n_interpolation if max_points is None else int(max_points)
        with torch.cuda.stream(st):
            sp = start_point.to(dev, torch.float64).reshape(-1, 2) if _is_tensor(start_point) else np.asarray(start_point, np.float64).reshape(-1, 2)
            par = _columns(dev, (length, sp[:, 0], sp[:, 1], heading, start_curvature, gamma))
            n = par.shape[0]
            xy = torch.empty((n, max(max_points, 0), 2), dtype=torch.float64, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            _ffi.check(lib.t2d_spiral_curves(device_id, n, par.data_ptr(), n_interpolation, rule, max_points, xy.data_ptr(),
                                             count.data_ptr(), st.cuda_stream), None, lib)
        if single:
            st.synchronize()
            return xy[0, :min(int(count[0]), max_points)].cpu().numpy()
        out = RoadCurves(xy, count)
        out._inputs = (par,)   # (kept alive with the result)
        return out


class ParamPoly3:
    """ParamPoly3 (interpolator/param_poly3.py) for batches: get_curve only (fit and split_polyline stay on the host)."""

    @staticmethod
    def get_curve(length, start_point, heading, aU, bU, cU, dU, aV, bV, cV, dV, p_range_type="normalized", max_points=None,
                  device_id=0, stream=None):
        """ParamPoly3.get_curve (param_poly3.py:17-65); the conventions of Spiral.get_curve.  A row has max(2, int(length / 0.1))
        points: the result is ragged, count says how many rows of xy each curve has.  p_range_type: "normalized" / "arcLength",
        one for all rows or a sequence of them (or int codes 0 / 1, an int32 tensor included); anything else is "normalized", as
        in the reference.  max_points default: the longest row's count."""
        import torch
        single = not any(_is_tensor(v) or np.ndim(v) for v in (length, heading, aU, bU, cU, dU, aV, bV, cV, dV)) and not _is_tensor(start_point) and np.ndim(start_point) == 1
        lib = _ffi.lib()
        dev, st = _stream_of(device_id, stream)
        with torch.cuda.stream(st):
            sp = start_point.to(dev, torch.float64).reshape(-1, 2) if _is_tensor(start_point) else np.asarray(start_point, np.float64).reshape(-1, 2)
            par = _columns(dev, (length, sp[:, 0], sp[:, 1], heading, aU, bU, cU, dU, aV, bV, cV, dV))
            n = par.shape[0]
            if _is_tensor(p_range_type):
                p_range = p_range_type.to(dev, torch.int32).reshape(-1)
            else:
                codes = [v if isinstance(v, (int, np.integer)) else P_RANGES.get(v, L.P_RANGE_NORMALIZED)
                         for v in ([p_range_type] if isinstance(p_range_type, (str, int, np.integer)) else list(p_range_type))]
                p_range = torch.as_tensor(np.asarray(codes, np.int32)).to(dev)
            p_range = (p_range.expand(n) if len(p_range) == 1 else p_range).contiguous()
            if max_points is None:
                finite = torch.nan_to_num(par[:, 0], nan=0.0, posinf=0.0, neginf=0.0).clamp(0.0, 1e8)
                max_points = max(2, int((finite / 0.1).to(torch.int64).max()))
            max_points = int(max_points)
            xy = torch.empty((n, max(max_points, 0), 2), dtype=torch.float64, device=dev)
            count = torch.empty(n, dtype=torch.int32, device=dev)
            _ffi.check(lib.t2d_param_poly3_curves(device_id, n, par.data_ptr(), p_range.data_ptr(), max_points, xy.data_ptr(),
                                                  count.data_ptr(), st.cuda_stream), None, lib)
        if single:
            st.synchronize()
            return xy[0, :min(int(count[0]), max_points)].cpu().numpy()
        out = RoadCurves(xy, count)
        out._inputs = (par, p_range)
        return out


def pack_planview(roads, max_geom=None):
    """The records of t2d_planview_lines / t2d_planview_routes from parsed <planView> elements.  roads: one list per road of one
    dict per <geometry>, with the OpenDRIVE attribute names: s, x, y, hdg, length and the child element under its own name as a
    dict of ITS attributes -- {"s": 0.0, "x": .., "y": .., "hdg": .., "length": .., "arc": {"curvature": 0.05}}; "line": {} (or
    None); "paramPoly3": {"aU": .., .., "dV": .., "pRange": "arcLength"} (pRange optional, "normalized" when absent or anything
    else, as in the reference).  A flat dict naming the child under "type" with the child's attributes beside its own is taken
    too.  Values may be numbers or the strings of the XML.  Returns (records float64 CPU tensor [n, max_geom, 14] -- the first
    double of a record holds the two int32 kind and p_range --, n_geom int32 CPU tensor [n]); max_geom default: the longest road
    (at least 1).  ValueError for a geometry without exactly one known child, a missing attribute, or more geometries than
    max_geom / layout.PLANVIEW_MAX_GEOM."""
    import torch
    longest = max([len(r) for r in roads] + [1])
    max_geom = longest if max_geom is None else int(max_geom)
    if longest > max_geom or max_geom > L.PLANVIEW_MAX_GEOM or max_geom < 1:
        raise ValueError(f"a road has {longest} geometries; max_geom is {max_geom}, the device cap layout.PLANVIEW_MAX_GEOM = {L.PLANVIEW_MAX_GEOM}")
    rec = np.zeros((len(roads), max_geom, L.PLANVIEW_RECORD_BYTES // 8), np.float64)
    head = rec.view(np.int32).reshape(len(roads), max_geom, L.PLANVIEW_RECORD_BYTES // 4)
    for e, road in enumerate(roads):
        for i, g in enumerate(road):
            kinds = [k for k in GEOMETRY_KINDS if k in g] if "type" not in g else [g["type"]]
            if len(kinds) != 1 or kinds[0] not in GEOMETRY_KINDS:
                raise ValueError(f"road {e}, geometry {i}: exactly one of {sorted(GEOMETRY_KINDS)} is needed, got {kinds}")
            child = g if "type" in g else (g[kinds[0]] or {})
            try:
                rec[e, i, 1:6] = [float(g[k]) for k in ("s", "x", "y", "hdg", "length")]
                attrs = [float(child[k]) for k in GEOMETRY_ATTRIBUTES[kinds[0]]]
            except KeyError as exc:
                raise ValueError(f"road {e}, geometry {i} ({kinds[0]}): attribute {exc} is missing") from None
            rec[e, i, 6:6 + len(attrs)] = attrs
            head[e, i, 0] = GEOMETRY_KINDS[kinds[0]]
            head[e, i, 1] = L.P_RANGE_ARC_LENGTH if child.get("pRange") == "arcLength" else L.P_RANGE_NORMALIZED
    return torch.from_numpy(rec), torch.as_tensor(np.array([len(r) for r in roads], np.int32))


def planview_inputs(dev, records, n_geom):
    """(records float64 [n, max_geom, 14], n_geom int32 [n]) on `dev`, checked: what pack_planview returns, or the same on the device"""
    import torch
    if not _is_tensor(records) or records.dtype != torch.float64 or records.dim() != 3 or records.shape[2] != L.PLANVIEW_RECORD_BYTES // 8 \
            or not 1 <= records.shape[1] <= L.PLANVIEW_MAX_GEOM:
        raise ValueError(f"records must be a float64 tensor [n, max_geom <= {L.PLANVIEW_MAX_GEOM}, {L.PLANVIEW_RECORD_BYTES // 8}] (pack_planview)")
    if not _is_tensor(n_geom) or tuple(n_geom.shape) != (records.shape[0],):
        raise ValueError(f"n_geom must be an integer tensor [{records.shape[0]}]")
    return records.to(dev).contiguous(), n_geom.to(dev, torch.int32).contiguous()


def planview_max_points(records, n_geom):
    """an upper bound of a road's raw (and so of its kept) points: per geometry int(length / 0.1) + 2, a spiral's 100"""
    import torch
    if records.shape[0] == 0:
        return 1
    length = torch.nan_to_num(records[:, :, 5], nan=0.0, posinf=0.0, neginf=0.0).clamp(0.0, 1e8)
    used = torch.arange(records.shape[1], device=records.device)[None, :] < n_geom[:, None].to(records.device)
    per = torch.maximum((length / 0.1).to(torch.int64) + 2, torch.tensor(100, device=records.device)) * used
    return max(2, min(int(per.sum(1).max()), L.PLANVIEW_MAX_RAW))


def planview_lines(records, n_geom, rule="reference", max_points=None, want_s=True, want_kappa=True, device_id=0, stream=None):
    """t2d_planview_lines: the reference line of n roads in one launch, as load_road builds pts_arr, s_arr and kappa_arr
    (map/parser/parse_xodr.py:773-809): every geometry sampled by its _sample_* method, a geometry's last point dropped where it
    repeats the one before, then every point within 0.02 m of the RAW point before it dropped.  records, n_geom: pack_planview's
    (CPU or CUDA tensors); rule: how spirals are evaluated (Spiral.get_curve); max_points default: a bound computed from the
    lengths.  Asynchronous on `stream`.  Returns PlanviewLines (s / kappa None where not wanted)."""
    import torch
    rule = _rule(rule)
    lib = _ffi.lib()
    dev, st = _stream_of(device_id, stream)
    with torch.cuda.stream(st):
        records, n_geom = planview_inputs(dev, records, n_geom)
        n, max_geom = records.shape[:2]
        max_points = planview_max_points(records, n_geom) if max_points is None else int(max_points)
        xy = torch.empty((n, max(max_points, 0), 2), dtype=torch.float64, device=dev)
        s = torch.empty((n, max(max_points, 0)), dtype=torch.float64, device=dev) if want_s else None
        kappa = torch.empty((n, max(max_points, 0)), dtype=torch.float64, device=dev) if want_kappa else None
        count = torch.empty(n, dtype=torch.int32, device=dev)
        _ffi.check(lib.t2d_planview_lines(device_id, n, records.data_ptr(), n_geom.data_ptr(), max_geom, rule, max_points, xy.data_ptr(),
                                          _ptr(s), _ptr(kappa), count.data_ptr(), st.cuda_stream), None, lib)
    out = PlanviewLines(xy, s, kappa, count)
    out._inputs = (records, n_geom)
    return out
