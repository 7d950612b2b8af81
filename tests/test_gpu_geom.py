"""The device geometry predicates of tactics2d_amd/csrc/t2d_geom_dev.h, one at a time, against the oracle -- at contact.

The event kernels decide collisions, out-of-bound, off-lane and arrival with these predicates, and they can be wrong only within
nanometres of a touch, where random scenes practically never look.  t2d_debug_geom (the probe of include/t2d_debug.h,
libt2d_hip_debug.so only) evaluates one predicate over fp64 arrays with the product's compile flags.  The arrays are those of
tests/geom_cases.py; tests/test_geom_cases.py holds the oracle against exact rational arithmetic on them and checks, on numpy
restatements of the two filters, that the share conditions asserted here are satisfiable.  The filters have no specification of
their own: they are CERTIFICATES -- wherever one answers 0 or 1 the answer must be convex_intersects'.
"""
import numpy as np
import pytest

import geom_cases as GC

gpu = pytest.mark.gpu

UNWRITTEN = np.uint64(0xFFFFFFFFFFFFFFFF)      # what the probe fills its output with before the launch


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def dev():
    from tactics2d_amd import debug
    debug.lib()
    return debug


def run(dev, fn, *arrays):
    """the probe over any number of rows, T2D_GEOM_MAX_N at a time; (f): no element keeps the fill pattern"""
    n = len(arrays[0])
    parts = [dev.geom(fn, *[a[i:i + dev.GEOM_MAX_N] for a in arrays]) for i in range(0, n, dev.GEOM_MAX_N)]
    out = np.concatenate(parts, axis=-1)
    assert not (bits(out) == UNWRITTEN).any(), f"{fn}: an element the kernel never wrote"
    return out


def assert_equal_by_name(got, want, names, what, bitwise=False):
    bad = (bits(got) != bits(want)) if bitwise else (got != want)
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{what}: {i.size} of {bad.size} differ, in {sorted(set(names[i]))}; first at {i[:5].tolist()}: "
                             f"got {got[i[:5]].tolist()}, want {want[i[:5]].tolist()}")


def assert_certificate(v, truth, names, what):
    assert np.isin(v, (0.0, 1.0, 2.0)).all(), what
    bad = (v != 2) & ((v == 1) != (truth != 0))
    if bad.any():
        i = np.flatnonzero(bad)
        raise AssertionError(f"{what}: {i.size} answers contradict convex_intersects, in {sorted(set(names[i]))}; first at {i[:5].tolist()}: "
                             f"filter {v[i[:5]].tolist()}, oracle {truth[i[:5]].tolist()}")


def undecided(v):
    return float((v == 2).mean())


def _pair_family(oracle):
    return {"random": GC.pair_random(), "near_parallel": GC.pair_near_parallel(), **GC.pair_exact(),
            **{"bisected" + k: v for k, v in GC.pair_bisected(oracle).items()}}


def _convex_family():
    return {"random": GC.convex_random(), "close": GC.convex_close(), **GC.convex_exact(), **GC.convex_offsets()}


# ---- (a) the predicates equal the oracle's, element for element --------------------------------------------------------------
@gpu
def test_sat_quads_equals_convex_intersects_in_both_roles(dev, oracle):
    """every pair and polygon case, each way round: sat_quads(A, B) = sat_quads(B, A) = t2do_convex_intersects -- padded triangles
    against the oracle's real triangles"""
    A, B, names = GC.join({**{"pair_" + k: v for k, v in _pair_family(oracle).items()}, **_convex_family()})
    want = oracle.geom("sat_quads", A, B)
    assert_equal_by_name(run(dev, "sat_quads", A, B), want, names, "sat_quads(A, B)")
    assert_equal_by_name(run(dev, "sat_quads", B, A), want, names, "sat_quads(B, A)")
    assert 0.3 < want.mean() < 0.8


@gpu
def test_point_in_quad_equals_point_in_convex(dev, oracle):
    B, pt, names = GC.join(GC.point_cases())
    assert_equal_by_name(run(dev, "point_in_quad", B, pt), oracle.geom("point_in_quad", B, pt), names, "point_in_quad")


@gpu
def test_piece_meets_quad_interior_equals_the_oracle(dev, oracle):
    P, piece, names = GC.join(GC.piece_cases())
    assert_equal_by_name(run(dev, "piece_meets_quad_interior", P, piece), oracle.geom("piece_meets_quad_interior", P, piece), names,
                         "piece_meets_quad_interior")


# ---- (b) seg_dist2, bit for bit ----------------------------------------------------------------------------------------------
@gpu
def test_seg_dist2_equals_the_oracle_bit_for_bit(dev, oracle):
    a, names = GC.join(GC.seg_cases())
    assert_equal_by_name(run(dev, "seg_dist2", a), oracle.geom("seg_dist2", a), names, "seg_dist2", bitwise=True)


# ---- (c), (d) the two filters: certificates, neither vacuous nor overconfident ----------------------------------------------------
@gpu
def test_rect_pair_filter_is_a_certificate_that_answers_where_it_should(dev, oracle):
    """(c) wherever rect_pair_filter answers, it is convex_intersects' answer.  (d) at most 10 % undecided in generic position; all
    undecided on the touching cases and within 1e-8 m of contact (its band is 1e-6 / (2 L) >= 2.5e-8 m at L <= 20 m; a slide of d
    along the line of centres opens at most d); deep overlaps with collinear sides certified; all decided, and right, 1e-3 m either
    side.  (tests/test_geom_cases.py: the same conditions on the restatement, and that a margin of 0 breaks the certificate)"""
    fam = _pair_family(oracle)
    A, B, names = GC.join(fam)
    v = run(dev, "rect_pair_filter", A, B)
    truth = oracle.geom("sat_quads", A, B)
    assert_certificate(v, truth, names, "rect_pair_filter")
    sel = lambda *k: np.isin(names, k)
    r = v[sel("random")]
    assert undecided(r) <= 0.10 and (r == 0).mean() > 0.2 and (r == 1).mean() > 0.2, (undecided(r), (r == 0).mean(), (r == 1).mean())
    for name in GC.PAIR_TOUCHING + ("bisectedlo", "bisectedhi", "bisected+3e-10", "bisected-3e-10", "bisected+1e-08", "bisected-1e-08"):
        assert undecided(v[sel(name)]) == 1.0, (name, undecided(v[sel(name)]))
    for name in GC.PAIR_DEEP:
        assert (v[sel(name)] == 1).all(), name
    assert (v[sel("bisected+0.001")] == 0).all() and (v[sel("bisected-0.001")] == 1).all()


@gpu
def test_rect_vs_convex_filter_is_a_certificate_that_answers_where_it_should(dev, oracle):
    """(c) wherever rect_vs_convex_filter answers, it is convex_intersects' answer -- quads and padded triangles.  (d) its band is
    1e-9 .. 1.42e-9 m and it has two certificates with a gap between them (a box across the outline is left to sat_quads), so: at
    most 10 % undecided on the widely placed random class, triangles certified `intersecting` as often as quads (the zero-normal
    exemption); all undecided at exact contact and 1e-10 m either side of it; `separated` for every box 1e-8 m .. 1e-3 m beyond an
    edge; `intersecting` for every box whose centre lies 1e-8 m .. 1e-3 m inside an edge, half way along it; undecided for a centre
    on the outline or outside it."""
    A, B, names = GC.join(_convex_family())
    v = run(dev, "rect_vs_convex_filter", A, B)
    truth = oracle.geom("sat_quads", A, B)
    assert_certificate(v, truth, names, "rect_vs_convex_filter")
    sel = lambda *k: np.isin(names, k)
    r = v[sel("random")]
    assert undecided(r) <= 0.10 and (r == 0).mean() > 0.2 and (r == 1).mean() > 0.2, (undecided(r), (r == 0).mean(), (r == 1).mean())
    tri = (B[:, 6] == B[:, 0]) & (B[:, 7] == B[:, 1])
    assert (v[sel("random") & tri] == 1).mean() > 0.2 and (v[sel("random") & ~tri] == 1).mean() > 0.2
    for name in ("side_on_edge_line", "corner_on_vertex", "beyond+1e-10", "beyond-1e-10", "centre+1e-10", "centre-1e-10"):
        assert undecided(v[sel(name)]) == 1.0, (name, undecided(v[sel(name)]))
    for d in GC.EDGE_OFFSETS[2:]:
        assert (v[sel(f"beyond{d:+g}")] == 0).all(), d
        assert (v[sel(f"centre{-d:+g}")] == 1).all(), d
        assert undecided(v[sel(f"centre{d:+g}")]) == 1.0 and undecided(v[sel(f"beyond{-d:+g}")]) == 1.0, d


# ---- (e) the IoU arithmetic ----------------------------------------------------------------------------------------------------
@gpu
def test_iou_terms_sum_to_the_oracles_area_and_iou_and_stay_finite(dev, oracle):
    """the eight clipped_edge_term values in quad_iou's order and tree, clamped at 0 = t2do_quad_intersection_area2 (clamped alike),
    the quotient with the two areas = t2do_quad_iou, bit for bit; and no inf / nan out of the divisions by den == 0 that the
    branch-free form performs and never selects -- identical quads, contact along an edge or at a corner, collinear sides, the
    NoAction and Arrival regimes, near the origin and at the far end of the domain"""
    A, B, names = GC.join(GC.iou_cases())
    out = run(dev, "iou_terms", A, B)
    s = out[:8]
    assert np.isfinite(out).all(), sorted(set(names[~np.isfinite(out).all(axis=0)]))
    inter = ((s[0] + s[1]) + (s[2] + s[3])) + ((s[4] + s[5]) + (s[6] + s[7]))
    inter = np.where(inter < 0.0, 0.0, inter)
    want_area2, want_iou = oracle.geom("iou", A, B)
    assert_equal_by_name(inter, np.where(want_area2 < 0.0, 0.0, want_area2), names, "intersection area", bitwise=True)
    assert_equal_by_name(inter / (out[8] + out[9] - inter), want_iou, names, "IoU", bitwise=True)
    # the cases are what they say: contact only = 0, identical = 1, and the rest in between
    for name in ("shared_edge", "shared_edge_full", "shared_corner", "corner_on_corner"):
        assert (inter[names == name] == 0.0).all(), name
    assert (want_iou[np.isin(names, ("identical", "identical_turned"))] == 1.0).all()
    assert (want_iou[names == "no_action"] > 0.999).all() and (want_iou[names == "arrival"] > 0.3).mean() > 0.5


# ---- (g) the probe's argument errors ---------------------------------------------------------------------------------------------
@gpu
def test_probe_argument_errors_return_their_codes_and_the_next_call_works(dev, oracle):
    from tactics2d_amd import _ffi
    lib = dev.lib()
    A, B = GC.pair_random(3)
    a, b = np.ascontiguousarray(A.T), np.ascontiguousarray(B.T)
    out = np.zeros(30)
    pa, pb, po = a.ctypes.data, b.ctypes.data, out.ctypes.data
    S, D, I = (dev.GEOM_FUNCTIONS[k][0] for k in ("sat_quads", "seg_dist2", "iou_terms"))
    for what, args in (("unknown fn", (0, 7, 3, pa, pb, po)), ("negative fn", (0, -1, 3, pa, pb, po)), ("n = 0", (0, S, 0, pa, pb, po)),
                       ("n < 0", (0, S, -5, pa, pb, po)), ("n too large", (0, S, dev.GEOM_MAX_N + 1, pa, pb, po)),
                       ("null a", (0, S, 3, None, pb, po)), ("null b", (0, I, 3, pa, None, po)), ("null output", (0, S, 3, pa, pb, None)),
                       ("null a of seg_dist2", (0, D, 3, None, None, po)), ("no such device", (1 << 20, S, 3, pa, pb, po)),
                       ("negative device", (-1, S, 3, pa, pb, po))):
        assert lib.t2d_debug_geom(*args) == _ffi.ERR_INVALID, what
        assert b"t2d_debug_geom" in lib.t2d_last_error(None), what
        assert (out == 0).all(), what
    with pytest.raises(ValueError):
        dev.geom("sat_quads", A, B[:2])
    # seg_dist2 takes a null second array, the largest n is accepted, and the call after the errors works
    seg, _ = GC.join(GC.seg_cases())
    s3 = np.ascontiguousarray(seg[:3].T)
    assert lib.t2d_debug_geom(0, D, 3, s3.ctypes.data, None, po) == _ffi.OK
    assert np.array_equal(bits(out[:3]), bits(oracle.geom("seg_dist2", seg[:3])))
    big = np.resize(seg, (dev.GEOM_MAX_N, 6))
    assert np.array_equal(bits(dev.geom("seg_dist2", big)), bits(oracle.geom("seg_dist2", big)))
    assert np.array_equal(dev.geom("sat_quads", A, B), oracle.geom("sat_quads", A, B))
