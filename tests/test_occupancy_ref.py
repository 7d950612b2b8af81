"""The occupancy specification (tests/occupancy_ref.py) against the rule in exact rational arithmetic, over every
cell of every scene of tests/occupancy_scenes.py:
  1. no false negative, ever: a cell whose exact distance is <= inflate is occupied;
  2. false positives lie in a band: a cell the specification marks has exact distance <= inflate + BAND;
  3. on the contact scenes the specification IS the exact answer."""
from fractions import Fraction

import numpy as np
import pytest

import occupancy_ref as R
import occupancy_scenes as S


def _exact(sc):
    """per cell the (d2, radius) pairs of the listed elements, exact"""
    els, invalid = R.elements(sc["rings"], sc["participants"], sc["include_participants"], sc["exclude_slot"])
    assert not invalid
    return R.exact_cells(sc["H"], sc["W"], sc["cell_size"], sc["origin"], els)


_RANDOM = S.random_scenes()
_CONTACT = S.contact_scenes()


def test_the_band_is_below_a_ten_thousandth_of_the_smallest_cell():
    assert R.BAND <= 1e-4 * min(S.CELL_SIZES)
    assert R.BAND == 4 * R.GUARD * R.MAGNITUDE
    for sc in _RANDOM + _CONTACT:   # the scenes stay within the magnitude the band is derived for
        m = R.window_magnitude(sc["H"], sc["W"], sc["cell_size"], sc["origin"], sc["inflate"])
        for v, rad in R.elements(sc["rings"], sc["participants"], sc["include_participants"], sc["exclude_slot"])[0]:
            m = max(m, float(np.abs(v).max()), rad)
        assert m <= R.MAGNITUDE


@pytest.mark.parametrize("k", range(len(_RANDOM)))
def test_no_false_negative_and_false_positives_within_the_band(k):
    sc = _RANDOM[k]
    mask, status = R.occupancy(**S.spec_kwargs(sc))
    assert status == R.OK
    exact = _exact(sc)
    infl, band = Fraction(sc["inflate"]), Fraction(R.BAND)
    n_occ = n_band = 0
    for r in range(sc["H"]):
        for c in range(sc["W"]):
            inside = R.exact_within(exact[r][c], infl)
            if inside:
                assert mask[r, c] == 1, f"cell ({r}, {c}) lies within inflate and is reported free"
            if mask[r, c]:
                assert R.exact_within(exact[r][c], infl + band), f"cell ({r}, {c}) is occupied beyond inflate + BAND"
                n_band += not inside
            n_occ += int(mask[r, c])
    print(f"scene {k}: {n_occ} of {sc['H'] * sc['W']} cells occupied, {n_band} of them beyond inflate (within the band)")
    assert n_occ > 0   # (the scene says something)


@pytest.mark.parametrize("k", range(len(_CONTACT)), ids=[sc["name"] for sc in _CONTACT])
def test_contact_scenes_equal_the_exact_answer(k):
    sc = _CONTACT[k]
    mask, status = R.occupancy(**S.spec_kwargs(sc))
    assert status == R.OK
    exact = _exact(sc)
    infl = Fraction(sc["inflate"])
    want = np.array([[R.exact_within(exact[r][c], infl) for c in range(sc["W"])] for r in range(sc["H"])], np.uint8)
    assert (mask == want).all()
    assert bool(mask[sc["cell"]]) == sc["occupied"]


def test_the_build_defined_rows():
    ring = [(0, 0), (2, 0), (2, 2), (0, 2)]
    ego = (1.0, 1.0, 0.0, S.SHAPE_OBB, 4.0, 2.0, 1)
    nan_active = (float("nan"), 1.0, 0.0, S.SHAPE_OBB, 4.0, 2.0, 1)
    nan_idle = (float("nan"), 1.0, 0.0, S.SHAPE_OBB, 4.0, 2.0, 0)
    kw = dict(H=4, W=6, cell_size=1.0, origin=(-4.0, -1.0), inflate=0.0)
    # a listed participant with a non-finite pose: INVALID, every cell an obstacle
    mask, status = R.occupancy(rings=[ring], participants=[ego, nan_active], include_participants=True, exclude_slot=0, **kw)
    assert status == R.INVALID and mask.all()
    # excluded, inactive, or participants not listed at all: the pose is never looked at
    free, status = R.occupancy(rings=[ring], participants=[ego, nan_idle], include_participants=True, exclude_slot=0, **kw)
    assert status == R.OK and not free.all() and free.any()
    for parts, inc, exc in (([ego, nan_active], True, 1), ([ego, nan_active], False, -1)):
        mask, status = R.occupancy(rings=[ring], participants=parts, include_participants=inc, exclude_slot=exc, **kw)
        assert status == R.OK
    # exclude_slot = -1 lists the ego too; a ring of two vertices is ignored
    with_ego, _ = R.occupancy(rings=[ring], participants=[ego], include_participants=True, exclude_slot=-1, **kw)
    assert with_ego.sum() > free.sum()
    none, status = R.occupancy(rings=[[(0, 0), (2, 2)]], **kw)
    assert status == R.OK and not none.any()
    assert (R.weights(free, 2.5)[free == 0] == 2.5).all() and np.isinf(R.weights(free)[free == 1]).all()


def test_a_disc_is_an_obstacle_and_inflate_adds_to_its_radius():
    disc = (0.0, 0.0, 0.0, S.SHAPE_CIRCLE, 0.6, 1.0, 1)   # radius 1 / 2
    kw = dict(H=1, W=5, cell_size=0.5, origin=(0.0, 0.0), participants=[disc], include_participants=True)
    m0, _ = R.occupancy(inflate=0.0, **kw)    # faces of the cells: -0.25 | 0.25 | 0.75 | 1.25 | 1.75 | 2.25
    assert m0[0].tolist() == [1, 1, 0, 0, 0]
    m1, _ = R.occupancy(inflate=0.25, **kw)   # radius + inflate = 0.75: touches the cell that starts at 0.75
    assert m1[0].tolist() == [1, 1, 1, 0, 0]
