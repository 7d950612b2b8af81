"""The device track generator's specification (tests/trackgen_ref.py) on the CPU: the committed fixture reproduces from it, it
agrees with the product's host class fed the same draws to one fp32 ulp, its streams are keyed as include/t2d.h says, and its
tracks have the geometry the algorithm guarantees.  (The kernel against the specification: tests/test_gpu_trackgen.py.)"""
import numpy as np
import pytest

import helpers as H
import trackgen_ref as R


@pytest.fixture(scope="module")
def fx():
    return H.load_npz("racing_trackgen.npz")


@pytest.fixture(scope="module")
def spec_tracks(oracle, fx):
    """the specification's track for each of the fixture's 8 full tracks, built once"""
    return {int(t): R.build(int(fx["seed"]), int(t)) for t in fx["full"]}


def test_the_fixture_reproduces_from_the_specification(fx, spec_tracks):
    assert len(fx["n_tile"]) == 64 and len(fx["full"]) == 8
    for t in [int(k) for k in fx["full"][:4]]:
        k = spec_tracks[t]
        for name in ("n_checkpoint", "n_tile", "attempt", "flags", "start_id"):
            assert int(fx[name][t]) == int(k[name]), (t, name)
        assert np.array_equal(fx["start_pose"][t].view(np.uint64), k["start_pose"].view(np.uint64))
        assert np.array_equal(fx["start_line"][t].view(np.uint32), k["start_line"].view(np.uint32))
        assert np.array_equal(fx["boundary"][t].view(np.uint32), k["boundary"].view(np.uint32))
        assert np.array_equal(fx[f"tiles_{t}"].view(np.uint32), k["tiles"].view(np.uint32))
        assert int(fx["crc"][t]) == R.crc(k["tiles"])


def test_the_fixture_holds_the_cases_the_kernel_must_meet(fx):
    """a winner at attempt 0, one in a later round of attempts, the smallest and the largest number of checkpoints, no flag"""
    att, ncp = fx["attempt"], fx["n_checkpoint"]
    assert (att == 0).any() and (att >= R.ROUND).any() and att.max() < R.MAX_ATTEMPTS
    assert (ncp == 10).any() and (ncp == 19).any() and ncp.min() >= 10 and ncp.max() <= 19
    assert not fx["flags"].any() and fx["n_tile"].min() >= 3 and fx["n_tile"].max() <= R.MAX_TILES
    full = [int(t) for t in fx["full"]]
    assert any(att[t] == 0 for t in full) and any(att[t] >= R.ROUND for t in full)


def test_the_specification_agrees_with_the_host_class_fed_the_same_draws(fx, spec_tracks):
    """tests/trackgen_ref.py against tactics2d_amd.generator.RacingTrackGenerator.generate(rng=...) with the winning attempt's
    draws, for all 8 full tracks: the same checkpoints, tiles and start straight; fp32 tiles equal or one ulp apart (libm and
    the deterministic trigonometry, BLAS's norm and the stated one differ in the last fp64 bits, which can flip an fp32
    rounding: <= 2^-13 m below 1024 m); start poses within 1e-9"""
    from tactics2d_amd.generator import RacingTrackGenerator
    seed = int(fx["seed"])
    gen = RacingTrackGenerator()
    for t, k in spec_tracks.items():
        draws = R.ReplayDraws(seed, t, int(k["attempt"]))
        track = gen.generate(rng=draws)
        assert draws.stream.count == R.attempt(seed, t, int(k["attempt"]))["draws"], "the host class took another path through the attempt"
        assert track.n_checkpoint == k["n_checkpoint"] and track.n_tile == k["n_tile"], t
        _, start_id = gen._get_start_point(track.n_checkpoint, _controls(gen, seed, t, int(k["attempt"])))
        assert start_id % track.n_checkpoint == k["start_id"], t
        pts = track.tiles.reshape(-1, 2)
        origin = (pts.min(axis=0) + pts.max(axis=0)) / 2
        t32 = np.float32(track.tiles - origin)
        assert np.abs(t32).max() < 1024.0
        ulps = np.abs(t32.view(np.int32).astype(np.int64) - k["tiles"].view(np.int32).astype(np.int64))
        same_sign = np.signbit(t32) == np.signbit(k["tiles"])
        assert (ulps[same_sign] <= 1).all() and (np.abs(t32 - k["tiles"])[~same_sign] <= 2.0 ** -13).all(), (t, int(ulps.max()))
        assert np.abs(t32 - k["tiles"]).max() <= 2.0 ** -13
        track.start_line = track.start_line - origin
        x, y, h = track.start_pose()
        want = k["start_pose"]
        assert abs(x - want[0]) <= 1e-9 and abs(y - want[1]) <= 1e-9 and abs(np.mod(h, 2 * np.pi) - want[2]) <= 1e-9, t


def _controls(gen, seed, t, a):
    _, control, ok = gen._get_checkpoints(R.ReplayDraws(seed, t, a))
    assert ok
    return control


def test_streams_of_different_keys_differ():
    keys = [(0, 0, 0), (0, 0, 1), (0, 1, 0), (1, 0, 0), (0, 1, 1), (1, 1, 1), (2**64 - 1, 0, 0), (0, 2**40, 0)]
    heads = [tuple(R.draw_at(R.stream_key(*k), j) for j in range(4)) for k in keys]
    assert len(set(heads)) == len(keys)
    states = {R.stream_key(0, t, a) for t in range(64) for a in range(R.MAX_ATTEMPTS)}
    assert len(states) == 64 * R.MAX_ATTEMPTS
    # no attempt's stream is another's shifted by a few draws (the counter advances by GAMMA per draw)
    shifted = {(s + j * R.GAMMA) & R.MASK for s in states for j in range(1, 4)}
    assert not states & shifted
    s = R.Stream(R.stream_key(3, 5, 7))
    assert [s.u() for _ in range(5)] == [R.draw_at(R.stream_key(3, 5, 7), j) for j in range(5)]
    assert all(0.0 <= R.draw_at(R.stream_key(9, t, 0), 0) < 1.0 for t in range(100))


def test_a_batch_split_anywhere_gives_the_same_tracks(fx, oracle):
    """record i of a batch that starts at first_track is record first_track + i of the fixture's batch, which starts at 0:
    integers, start pose, boundary and the tiles' crc, for batches cut at the front, in the middle and at the end -- and the
    same cut under another seed gives other tracks"""
    seed = int(fx["seed"])
    for first, n in ((0, 1), (1, 2), (37, 1), (62, 2)):
        part = R.build_batch(n, seed, first_track=first)
        assert len(part) == n
        for i, r in enumerate(part):
            t = first + i
            assert (r["attempt"], r["n_checkpoint"], r["n_tile"], r["flags"]) == tuple(int(fx[k][t]) for k in ("attempt", "n_checkpoint", "n_tile", "flags")), t
            assert R.crc(r["tiles"]) == fx["crc"][t], t
            assert np.array_equal(r["start_pose"], fx["start_pose"][t]) and np.array_equal(r["boundary"], fx["boundary"][t]), t
    assert R.build_batch(0, seed, first_track=5) == []
    other = R.build_batch(1, seed + 1, first_track=37)[0]
    assert R.crc(other["tiles"]) != fx["crc"][37]
    with pytest.raises(ValueError):
        R.build_batch(1, seed, first_track=-1)


def test_the_tracks_have_the_geometry_the_algorithm_guarantees(fx):
    for t in [int(k) for k in fx["full"]]:
        tiles = fx[f"tiles_{t}"].astype(np.float64)
        n = len(tiles)
        assert n == fx["n_tile"][t]
        # tile i = left[i], left[i + 1], right[i + 1], right[i]: the width is 5 at both ends
        assert np.abs(np.linalg.norm(tiles[:, 0] - tiles[:, 3], axis=1) - 5.0).max() < 1e-3
        assert np.abs(np.linalg.norm(tiles[:, 1] - tiles[:, 2], axis=1) - 5.0).max() < 1e-3
        # consecutive tiles share an edge, and the ring closes: the end of tile i is the start of tile (i + 1) % n, bit for bit
        nxt = np.roll(fx[f"tiles_{t}"], -1, axis=0)
        assert np.array_equal(fx[f"tiles_{t}"][:, 1], nxt[:, 0]) and np.array_equal(fx[f"tiles_{t}"][:, 2], nxt[:, 3])
        # centred: the bounding box of the vertices is symmetric about the origin (to fp32 rounding)
        pts = tiles.reshape(-1, 2)
        assert np.abs(pts.min(axis=0) + pts.max(axis=0)).max() < 1e-3
        b = fx["boundary"][t]
        assert b[0] <= pts[:, 0].min() and b[1] >= pts[:, 0].max() and b[2] <= pts[:, 1].min() and b[3] >= pts[:, 1].max()
        # the start line is the end of tile 0 and the start pose lies half a car behind it, pointing across it (the line is
        # the fp32 one here: each coordinate is within 2^-14 m of the fp64 value below 1024 m, their midpoint within 1e-4 m)
        assert np.array_equal(fx["start_line"][t], fx[f"tiles_{t}"][0, 1:3])
        x, y, h = fx["start_pose"][t]
        mid = fx["start_line"][t].astype(np.float64).mean(axis=0)
        assert abs(np.hypot(mid[0] - x, mid[1] - y) - R.CAR_LENGTH / 2) < 1e-4 and 0.0 <= h < 2 * np.pi
        assert abs(np.cos(h) * (mid[0] - x) + np.sin(h) * (mid[1] - y) - R.CAR_LENGTH / 2) < 1e-4
