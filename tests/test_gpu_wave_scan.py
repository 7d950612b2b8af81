"""The step kernel's slot hand-out, alone: wave_excl_scan (csrc/t2d_collide.hip) gives every lane of a wave the sum of the
candidate counts of the lanes below it and the wave the sum of all 64 -- six DPP additions in registers.  compact_and_process
writes its queue at these offsets, so one wrong seam (the rows of 16 lanes of the row_shr steps, the half-wave of
row_bcast:31) would make two lanes write the same slot.  t2d_debug_wave_scan runs that function on one wave per vector of 64
counts; the reference is numpy.cumsum, exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def _cases():
    cases = {"all zero": np.zeros(64, np.int32), "every lane 1": np.ones(64, np.int32),
             "every lane 64": np.full(64, 64, np.int32),   # total 4096: above any queue capacity
             "alternating 0 and 3": np.tile(np.array([0, 3], np.int32), 32)}
    for lane in (0, 31, 32, 63):   # the row and half-wave seams of the DPP steps
        v = np.zeros(64, np.int32)
        v[lane] = 1
        cases[f"lane {lane} only"] = v
    rng = np.random.default_rng(20827)
    for k in range(200):
        cases[f"random {k}"] = rng.integers(0, 65, 64).astype(np.int32)
    return cases


@pytest.fixture(scope="module")
def scanned():
    """every case in ONE probe call, one wave each: name -> (counts, offsets, total)"""
    from tactics2d_amd import debug
    cases = _cases()
    counts = np.stack(list(cases.values()))
    off, total = debug.wave_scan(counts)
    assert off.shape == counts.shape and total.shape == (len(cases),)
    return {name: (counts[i], off[i], int(total[i])) for i, name in enumerate(cases)}


@pytest.mark.parametrize("name", ["all zero", "lane 0 only", "lane 31 only", "lane 32 only", "lane 63 only", "every lane 1",
                                  "every lane 64", "alternating 0 and 3"])
def test_named_vectors(scanned, name):
    cnt, off, total = scanned[name]
    incl = np.cumsum(cnt, dtype=np.int64)
    assert (off == incl - cnt).all(), f"{name}: offsets {off.tolist()}"
    assert total == int(incl[-1]), name


def test_every_lane_64_totals_4096(scanned):
    assert scanned["every lane 64"][2] == 4096


def test_random_vectors(scanned):
    n = 0
    for name, (cnt, off, total) in scanned.items():
        if not name.startswith("random"):
            continue
        incl = np.cumsum(cnt, dtype=np.int64)
        assert (off == incl - cnt).all(), f"{name}: counts {cnt.tolist()} offsets {off.tolist()}"
        assert total == int(incl[-1]), name
        n += 1
    assert n == 200


def test_single_vector_form():
    """a [64] input comes back as ([64], int)"""
    from tactics2d_amd import debug
    cnt = np.arange(64, dtype=np.int32)
    off, total = debug.wave_scan(cnt)
    assert (off == np.cumsum(cnt) - cnt).all() and total == 2016


def test_bad_arguments():
    from tactics2d_amd import debug
    with pytest.raises(ValueError):
        debug.wave_scan(np.zeros(63, np.int32))
    with pytest.raises(Exception):
        debug.wave_scan(np.zeros((0, 64), np.int32))   # n_waves = 0: T2D_ERR_INVALID
