"""Off-route detection for every participant in one launch (t2d_set_routes / t2d_set_routes_from_traj / t2d_off_route,
t2d_route.hip) against the restatement tests/route_ref.py.  No tolerance appears anywhere: distance bits and verdict bytes are
the restatement's, evaluated on the positions the device holds.

Bands (they keep a bit-identity test from passing on trivial data), checked with the restatement alone on the C oracle's CPU
rollouts before these tests were written (tests/test_off_route.py re-checks them on every CPU run).  Off-route share of the
active, routed participants after steps 1 .. 8 of the scene's random actions (sample_actions, default_rng(21)), thresholds
route_scenes.THRESHOLD (highway 0.2 m, roundabout 0.1 m, intersection 0.15 m), and the share whose nearest segment is not
segment 0:

    scene                         variant             off-route share, steps 1 .. 8     nearest segment != 0
    highway(64, 64, seed=2)       shared / per_env    0.348 .. 0.818                    (two-vertex routes: not asked)
    highway(64, 64, seed=2)       permuted            0.833 .. 0.952
    intersection(100, 32, seed=3) shared / per_env    0.321 .. 0.426                    1.000
    intersection(100, 32, seed=3) permuted            0.724 .. 0.786                    1.000
    mixed(96, 64, seed=6)         shared / per_env    0.270 .. 0.536                    0.651 .. 0.655
    mixed(96, 64, seed=6)         permuted            0.805 .. 0.883                    0.634 .. 0.639
    trace routes, mixed(48, 64, seed=6), 32 steps re-run with perturbed actions against the recording, threshold 0.05 m:
                                                      0.017 (step 1) .. 0.840 (step 32),      0.983 over the 32 steps
                                                      0.530 over the 32 steps together
    (the first step of a re-run is on the trace by construction, so this band is taken over the 32 steps together:
    tests/test_off_route.py::test_the_bands_of_the_gpu_trace_test_hold_on_the_cpu)

so every listed scene meets the bands with these thresholds and seeds.  The scene tests assert the bands after every step; the
trace test over its steps together.

Small pools with long traces take the form with several lanes per participant (every trace test here below 131 072 participants
does); test_the_small_pool_form_gives_the_bits_of_the_one_lane_path holds it against the one-lane kernel on the same data."""
import numpy as np
import pytest

import helpers as H
import route_ref as R
import route_scenes as RS

pytestmark = pytest.mark.gpu

TRACE_THRESHOLD = 0.05


def trace_scene():
    from tactics2d_amd import scenarios as S
    return S.mixed(48, 64, seed=6)


def perturb_actions(k, a0, a1):
    """the re-run's actions: the recording's plus noise (seeded by the step)"""
    rng = np.random.default_rng(1000 + k)
    return (a0 + rng.normal(0, 0.5, len(a0))).astype(np.float32), (a1 + rng.normal(0, 0.01, len(a1))).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ helpers
def _pool(sc):
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc.n_env, sc.A)
    sc.load(pool)
    return pool


def _xy_active(pool):
    from tactics2d_amd import layout as L
    return pool.download(L.F_X), pool.download(L.F_Y), ((pool.download(L.F_IDS) >> 16) & 0xff).astype(np.uint8)


def _same(got, want, what=""):
    gd, go = got
    wd, wo = want[0], want[1]
    gd, go = gd.reshape(-1), go.reshape(-1).astype(np.uint8)
    assert gd.dtype == np.float32 and wd.dtype == np.float32
    bad = (gd.view(np.uint32) != wd.view(np.uint32)) | (go != wo)
    assert not bad.any(), (what, int(bad.sum()), np.nonzero(bad)[0][:6].tolist(), gd[bad][:6], wd[bad][:6], go[bad][:6], wo[bad][:6])


def _bands(off, seg, routed, many_segments, what):
    share = float(off[routed].mean())
    moved = float((seg[routed] != 0).mean())
    print(f"{what}: off-route share {share:.4f}, nearest segment != 0 {moved:.4f}, routed {int(routed.sum())}")
    assert 0.02 < share < 0.98, (what, share)
    if many_segments:
        assert moved >= 0.25, (what, moved)


def _simple_pool(n_env, A, x, y, active=None):
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(n_env, A)
    pool.set_param_table(H.shape_rows())
    n = n_env * A
    z = np.zeros(n, np.float32)
    pool.reset(np.float32(x), np.float32(y), z, z, np.arange(n, dtype=np.uint8) % len(H.shape_rows()), active)
    return pool


def _trace_buffer(pool, routes_per_participant):
    """a trajectory of `pool` whose slots 0 .. n - 1 hold participant i's polyline (last_slot = n - 1); returns (buffer, first, last)"""
    from tactics2d_amd.history import _TrajBuffer
    S = max(len(r) for r in routes_per_participant)
    buf = _TrajBuffer(pool, S)
    cols = np.zeros((S, 6, pool.n), np.float32)
    last = np.zeros(pool.n, np.int32)
    for i, r in enumerate(routes_per_participant):
        r = np.float32(r)
        last[i] = len(r) - 1
        cols[:len(r), 0, i], cols[:len(r), 1, i] = r[:, 0], r[:, 1]
        cols[len(r):, 0, i], cols[len(r):, 1, i] = 1e6, -1e6      # (slots behind the window: must never be read as route)
    for k in range(S):
        buf.write(k, cols[k])
    return buf, np.zeros(pool.n, np.int32), last


# ------------------------------------------------------------------------------------------------------ known answers
def test_known_answers_through_both_route_kinds():
    kats = R.kats()
    n = len(kats)
    x, y = [k[2][0] for k in kats], [k[2][1] for k in kats]
    thr = np.float32([k[3] for k in kats])
    pool = _simple_pool(n, 1, x, y)
    try:
        want_d = np.float32([k[5] for k in kats]); want_o = np.uint8([k[4] for k in kats])
        for c, k in enumerate(kats):   # (the table's answers are the restatement's)
            d, off, _ = R.distance(k[1], k[2][0], k[2][1], k[3])
            assert d == want_d[c] and off == bool(want_o[c]), k[0]
        pool.set_routes([[np.float32(k[1])] for k in kats], np.arange(n), 0, thr)
        _same(pool.off_route_host(), (want_d, want_o), "set routes")
        buf, first, last = _trace_buffer(pool, [k[1] for k in kats])
        pool._ck(pool._lib.t2d_set_routes_from_traj(pool._h, buf._live(), buf.capacity, None, first.ctypes.data, last.ctypes.data, None,
                                                    thr.ctypes.data))
        pool.route_kind = "traces"
        _same(pool.off_route_host(), (want_d, want_o), "trace routes")
        # caller-owned destinations, on a stream of the caller's
        import torch
        d = torch.full((n,), -1.0, dtype=torch.float32, device="cuda")
        o = torch.full((n,), 7, dtype=torch.uint8, device="cuda")
        pool.off_route(d.data_ptr(), o.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        _same((d.cpu().numpy(), o.cpu().numpy()), (want_d, want_o), "caller-owned outputs")
        pool.clear_routes()
        buf.close()
    finally:
        pool.close()


def test_build_defined_rows_and_thresholds():
    """inactive participants, route_of = -1, NaN / inf positions: off = 0, distance = NaN; a NaN threshold is never exceeded, a
    negative one by every finite distance -- with both kinds of routes"""
    from tactics2d_amd import layout as L
    n_env, A = 3, 8
    n = n_env * A
    rng = np.random.default_rng(3)
    x, y = rng.uniform(-5, 25, n).astype(np.float32), rng.uniform(-5, 5, n).astype(np.float32)
    active = np.ones(n, np.uint8); active[[2, 9, 17]] = 0
    routes = [np.float32([[0, 0], [10, 0], [20, 3]]), np.float32([[0, 1], [20, 1]])]
    ro = (np.arange(n) % 2).astype(np.int32); ro[[3, 12]] = -1
    thr = rng.uniform(0.5, 4, n).astype(np.float32); thr[[4, 13]] = np.nan; thr[[5, 14]] = -1.0
    pool = _simple_pool(n_env, A, x, y, active)
    try:
        x[[6, 15]] = np.nan; y[7] = np.inf; x[16] = -np.inf
        pool.upload(L.F_X, x); pool.upload(L.F_Y, y)
        pool.set_routes([routes], None, ro, thr)
        want = R.evaluate_sets([routes], np.zeros(n_env, int), ro, A, x, y, thr, active)
        got = pool.off_route_host()
        _same(got, want, "sets")
        d, o = got[0].reshape(-1), got[1].reshape(-1)
        dead = [2, 9, 17, 3, 12, 6, 15, 7, 16]
        assert np.isnan(d[dead]).all() and not o[dead].any()
        assert not o[[4, 13]].any() and np.isfinite(d[[4, 13]]).all() and o[[5, 14]].all()
        assert 0 < o.sum() < n - len(dead)
        per = [routes[r] if r >= 0 else routes[0] for r in ro]
        buf, first, last = _trace_buffer(pool, per)
        own = np.where(ro < 0, -1, np.arange(n) % A).astype(np.int32)
        pool._ck(pool._lib.t2d_set_routes_from_traj(pool._h, buf._live(), buf.capacity, None, first.ctypes.data, last.ctypes.data,
                                                    own.ctypes.data, thr.ctypes.data))
        pool.route_kind = "traces"
        _same(pool.off_route_host(), want, "traces")
        pool.clear_routes()
        buf.close()
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------------ set routes on the scenes
@pytest.mark.parametrize("variant", ["shared", "per_env", "permuted"])
@pytest.mark.parametrize("name", ["highway", "intersection", "mixed"])
def test_set_routes_on_the_scenes(name, variant):
    sc = RS.scene(name)
    sets, soe, ro, thr = RS.build(sc, variant)
    pool = _pool(sc)
    try:
        if variant == "permuted":   # the geometry of the shared variant first, then the assignment alone
            s0, e0, r0, t0 = RS.build(sc, "shared")
            pool.set_routes(s0, e0, r0, t0)
            pool.set_route_assignment(ro, thr)
        else:
            pool.set_routes(sets, None if variant == "shared" else soe, ro, thr)
        rng = np.random.default_rng(21)
        for k in range(9):
            if k:
                pool.set_actions(*sc.sample_actions(rng))
                pool.step(sc.interval_ms)
                pool.off_route()
                got = pool.off_route_all()
            else:
                got = pool.off_route_host()
            x, y, active = _xy_active(pool)
            want = R.evaluate_sets(sets, soe, ro, sc.A, x, y, thr, active)
            _same(got, want, f"{name} {variant} step {k}")
            if k:
                _bands(want[1], want[2], (ro >= 0) & (active != 0), name != "highway", f"{name} {variant} step {k}")
    finally:
        pool.close()


def test_a_set_at_the_capacity_limit_and_one_beyond():
    """64 routes x 64 vertices = T2D_MAX_ROUTE_SET_VERTS is accepted and evaluated; one vertex more is T2D_ERR_GEOMETRY, names the
    limit and the set, and leaves the installed routes working"""
    from tactics2d_amd import _ffi, layout as L
    assert L.MAX_ROUTE_SET_VERTS == 4096
    rng = np.random.default_rng(8)
    n_env, A = 5, 64
    n = n_env * A
    routes = []
    for r in range(64):
        h = rng.uniform(0, 2 * np.pi) + np.cumsum(rng.normal(0, 0.3, 64))
        routes.append(np.float32(rng.uniform(-50, 50, 2) + np.cumsum(np.stack([np.cos(h), np.sin(h)], 1) * rng.uniform(1, 4, (64, 1)), 0)))
    small = [np.float32([[0, 0], [1, 1]])]
    x, y = rng.uniform(-80, 80, n).astype(np.float32), rng.uniform(-80, 80, n).astype(np.float32)
    ro = rng.permutation(n).astype(np.int32) % 64
    soe = np.int32([1, 0, 1, 1, 0])
    ro[np.repeat(soe == 0, A)] = 0
    thr = np.full(n, 20.0, np.float32)
    pool = _simple_pool(n_env, A, x, y)
    try:
        pool.set_routes([small, routes], soe, ro, thr)
        want = R.evaluate_sets([small, routes], soe, ro, A, x, y, thr, np.ones(n))
        _same(pool.off_route_host(), want, "4096 vertices")
        _bands(want[1], want[2], np.repeat(soe == 1, A), True, "capacity")
        with pytest.raises(_ffi.GeometryError) as ei:
            pool.set_routes([small, routes + [np.float32([[0, 0], [1, 0]])]], soe, ro, thr)
        assert ei.value.code == _ffi.ERR_GEOMETRY and "4096" in str(ei.value) and "set 1" in str(ei.value), str(ei.value)
        _same(pool.off_route_host(), want, "after the refusal")
    finally:
        pool.close()


# ------------------------------------------------------------------------------------------------------ trace routes
def test_trace_routes_of_a_recorded_rollout():
    """record 32 steps, restore, step again with perturbed actions: every participant against its own recorded trace after every
    step; then windows that start late / end early / are empty / hold one slot, and another agent's trace as the route"""
    from tactics2d_amd.history import DeviceTrajectory
    sc = trace_scene()
    n, A = sc.n, sc.A
    pool = _pool(sc)
    try:
        traj = DeviceTrajectory(pool, 0, capacity=33)
        traj.record(pool, 0)
        rng = np.random.default_rng(5)
        for k in range(32):
            pool.set_actions(*sc.sample_actions(rng))
            pool.step(sc.interval_ms)
            traj.record(pool, (k + 1) * sc.interval_ms)
        xy = traj.traces()
        assert xy.shape == (33, n, 2)
        pool.restore()
        traj.set_routes_from(pool, threshold=TRACE_THRESHOLD)
        thr = np.full(n, TRACE_THRESHOLD, np.float32)
        first, last = np.zeros(n, np.int32), np.full(n, 32, np.int32)
        own, ident = np.arange(n) % A, np.arange(sc.n_env)
        x, y, active = _xy_active(pool)
        got = pool.off_route_host()
        _same(got, R.evaluate_traces(xy, first, last, ident, own, A, x, y, thr, active), "at the start")
        assert (got[0].reshape(-1)[active != 0] == 0).all() and not got[1].any()   # everybody starts on its own trace
        rng = np.random.default_rng(5)
        offs, segs = [], []
        for k in range(32):
            pool.set_actions(*perturb_actions(k, *sc.sample_actions(rng)))
            pool.step(sc.interval_ms)
            pool.off_route()
            x, y, active = _xy_active(pool)
            want = R.evaluate_traces(xy, first, last, ident, own, A, x, y, thr, active)
            _same(pool.off_route_all(), want, f"re-run step {k}")
            live = active != 0
            offs.append(want[1][live].mean()); segs.append((want[2][live] != 0).mean())
        print("off-route share per step", " ".join(f"{v:.3f}" for v in offs))
        print(f"over the 32 steps: off-route share {np.mean(offs):.4f}, nearest segment != 0 {np.mean(segs):.4f}")
        assert 0.02 < np.mean(offs) < 0.98 and np.mean(segs) >= 0.25
        # windows of every kind + another agent's trace + nobody's
        rng = np.random.default_rng(9)
        kind = rng.integers(0, 5, n)
        first[kind == 1] = rng.integers(2, 25, (kind == 1).sum())
        last[kind == 2] = rng.integers(2, 25, (kind == 2).sum())
        first[kind == 3] = last[kind == 3] = rng.integers(1, 30, (kind == 3).sum())   # one slot: no polyline
        first[kind == 4], last[kind == 4] = 1, 0                                        # empty
        ro = ((np.arange(n) % A + 1) % A).astype(np.int32)
        ro[rng.uniform(size=n) < 0.1] = -1
        thr = rng.uniform(0.05, 3.0, n).astype(np.float32)
        pool.set_routes_from(traj, windows=(first, last), route_of=ro, threshold=thr)
        want = R.evaluate_traces(xy, first, last, ident, ro, A, x, y, thr, active)
        got = pool.off_route_host()
        _same(got, want, "windows")
        j = np.arange(n) // A * A + np.maximum(ro, 0)
        none = (ro < 0) | (last[j] - first[j] < 1)
        assert none.sum() > n // 5 and np.isnan(got[0].reshape(-1)[none]).all() and not got[1].reshape(-1)[none].any()
        _bands(want[1], want[2], ~none & (active != 0), True, "windows, another agent's trace")
        # re-recording a bound slot changes the route: nothing was copied
        traj._buf.record(20)
        xy2 = traj.traces()
        assert not np.array_equal(xy2[20], xy[20])
        _same(pool.off_route_host(), R.evaluate_traces(xy2, first, last, ident, ro, A, x, y, thr, active), "after re-recording slot 20")
        pool.clear_routes()
        traj.close()
    finally:
        pool.close()


def test_a_library_source_shuffled_and_replayed_participants_on_their_own_trace():
    """the source belongs to a library pool of another size, src_env shuffled; replayed participants (MODEL_REPLAY) checked against
    their own trace sit on it at every on-grid step: distance 0 exactly, never off; integrated ones are compared as usual"""
    from test_gpu_replay import _window_source
    from tactics2d_amd import layout as L
    from tactics2d_amd.history import ReplaySource
    from tactics2d_amd.participant import replayed_shape_row
    from tactics2d_amd.pool import ParticipantPool
    rng = np.random.default_rng(31)
    n_env, A, n_src, period, n_slots = 40, 8, 7, 40, 64
    n = n_env * A
    st, _, _, _ = _window_source(rng, n_src, A, n_slots)
    first, last = np.zeros(n_src * A, np.int32), np.full(n_src * A, n_slots - 1, np.int32)
    first[3], last[5] = 6, 20
    rows = H.shape_rows(False)
    rows = np.concatenate([rows[:2], np.stack([replayed_shape_row(r[L.P_SHAPE], r[L.P_LENGTH], r[L.P_WIDTH]) for r in rows[:2]])])
    tid = np.where(np.arange(n) % A < 2, np.arange(n) % 2, 2 + np.arange(n) % 2).astype(np.uint8)   # agents 0, 1 integrated
    src_env = rng.integers(0, n_src, n_env).astype(np.int32)
    pool = ParticipantPool(n_env, A)
    try:
        src = ReplaySource.from_arrays(pool, st, first, last, 0, period)
        assert src.device_buffer().pool is not pool
        pool.set_param_table(rows)
        pool.set_status_config(max_step=100000)
        flat = st.reshape(n_slots, n_src * A, 6)
        j = np.repeat(src_env, A) * A + np.arange(n) % A
        start = flat[0][j]
        start[:, :2] += rng.normal(0, 0.5, (n, 2)).astype(np.float32) * (tid < 2)[:, None]
        pool.reset(start[:, 0], start[:, 1], start[:, 2], start[:, 3], tid)
        pool.replay_bind(src, src_env)
        pool.replay_apply()
        src.set_routes_from(pool, threshold=0.0)     # (src_env: the binding's; windows: the source's)
        traces = src.traces()
        assert len(traces) == n_src * A and len(traces[3]) == n_slots - 6 and len(traces[5]) == 21
        xy = flat[:, :, :2]
        thr = np.zeros(n, np.float32)
        own = np.arange(n) % A
        seen_replayed = 0
        for k in range(12):
            if k:
                pool.set_actions(rng.uniform(-1, 1, n).astype(np.float32), rng.normal(0, 0.05, n).astype(np.float32))
                pool.step(2 * period)
            x, y, active = _xy_active(pool)
            want = R.evaluate_traces(xy, first, last, src_env, own, A, x, y, thr, active)
            got = pool.off_route_host()
            _same(got, want, f"step {k}")
            rep = (tid >= 2) & (active != 0)
            seen_replayed += int(rep.sum())
            assert (got[0].reshape(-1)[rep] == 0).all() and not got[1].reshape(-1)[rep].any(), k
            assert got[1].reshape(-1)[tid < 2].mean() > 0.5      # (threshold 0: the integrated ones are off their source's trace)
        assert seen_replayed > 6 * n // 2
        assert (_xy_active(pool)[2][(j == 5) & (tid >= 2)] == 0).all()   # (source participant 5 left at slot 20: inactive, NaN rows)
        pool.clear_routes()
        pool.replay_unbind()
        src.close()
    finally:
        pool.close()


def test_the_small_pool_form_gives_the_bits_of_the_one_lane_path():
    """1 env x 4 participants on a 512-slot trace (64 lanes per participant, the minimum taken over (d2, segment index)) against
    the same four participants and traces tiled into a pool of 131 072 participants, which takes the one-lane kernel: the same
    bits, and both the restatement's.  The traces cross themselves and stand still for stretches, so equal minima on different
    lanes occur: the first one in vertex order must win."""
    from tactics2d_amd.history import _TrajBuffer
    from tactics2d_amd.pool import ParticipantPool
    rng = np.random.default_rng(12)
    A, n_slots, big_env = 4, 512, 32768
    h = np.cumsum(rng.normal(0, 0.25, (n_slots, A)), 0) + rng.uniform(0, 2 * np.pi, A)
    step = rng.uniform(0.2, 1.0, (n_slots, A)) * (rng.uniform(size=(n_slots, A)) > 0.15)     # (stationary stretches)
    xy = np.cumsum(np.stack([step * np.cos(h), step * np.sin(h)], -1), 0).astype(np.float32)  # [512, 4, 2]
    xy[300:, 1] = xy[299::-1, 1][:212]          # participant 1 drives back along its own trace: every distance is met twice
    first, last = np.int32([0, 0, 40, 0]), np.int32([511, 511, 470, 511])
    results = []
    for n_env in (1, big_env):
        n = n_env * A
        reps = n // A
        # positions: near the traces, different in every env of the big pool except env 0, which equals the small pool's
        base = xy[rng.integers(0, n_slots, A), np.arange(A)] if n_env == 1 else None
        if n_env == 1:
            pos0 = (base + np.float32([[0.3, -0.2], [0.0, 0.5], [1.0, 1.0], [0.0, 0.0]])).astype(np.float32)
            pos = pos0
        else:
            more = xy[rng.integers(0, n_slots, n), np.arange(n) % A] + rng.normal(0, 0.5, (n, 2))
            pos = more.astype(np.float32)
            pos[:A] = pos0
        pool = _simple_pool(n_env, A, pos[:, 0], pos[:, 1])
        try:
            buf = _TrajBuffer(pool, n_slots)
            for k in range(n_slots):
                cols = np.zeros((6, n), np.float32)
                cols[0], cols[1] = np.tile(xy[k, :, 0], reps), np.tile(xy[k, :, 1], reps)
                buf.write(k, cols)
            thr = np.full(n, 0.4, np.float32)
            f, l = np.tile(first, reps), np.tile(last, reps)
            pool._ck(pool._lib.t2d_set_routes_from_traj(pool._h, buf._live(), n_slots, None, f.ctypes.data, l.ctypes.data, None,
                                                        thr.ctypes.data))
            pool.route_kind = "traces"
            got = pool.off_route_host()
            trace = np.tile(xy, (1, reps, 1))
            want = R.evaluate_traces(trace, f, l, np.arange(n_env), np.arange(n) % A, A, pos[:, 0], pos[:, 1], thr, np.ones(n))
            _same(got, want, f"{n_env} env(s)")
            results.append((got[0].reshape(-1)[:A].copy(), got[1].reshape(-1)[:A].copy(), want[2][:A].copy()))
            if n_env > 1:
                _bands(want[1], want[2], np.ones(n, bool), True, "one lane per participant, 512-slot traces")
            pool.clear_routes()
            buf.close()
        finally:
            pool.close()
    (d1, o1, s1), (d2, o2, s2) = results
    assert d1.tobytes() == d2.tobytes() and o1.tobytes() == o2.tobytes() and (s1 == s2).all()
    print("small pool:", d1, o1, "nearest segments", s1)
    assert d1[3] == 0 and s1[1] < 300          # on a vertex; the earlier of the two passes of participant 1 wins


# ------------------------------------------------------------------------------------------------------ errors
def test_every_refusal_returns_its_code_and_leaves_the_previous_routes_working():
    from tactics2d_amd import _ffi
    from tactics2d_amd.history import _TrajBuffer
    from tactics2d_amd.pool import ParticipantPool
    from tactics2d_amd.traffic import routes_to_csr
    n_env, A = 4, 4
    n = n_env * A
    rng = np.random.default_rng(2)
    x, y = rng.uniform(-5, 15, n).astype(np.float32), rng.uniform(-5, 5, n).astype(np.float32)
    routes = [np.float32([[0, 0], [10, 0]]), np.float32([[0, 2], [5, 2], [10, 3]])]
    thr = np.full(n, 1.0, np.float32)
    ro = (np.arange(n) % 2).astype(np.int32)
    i32 = lambda a: np.ascontiguousarray(a, np.int32)

    def refused(code, text, fn):
        with pytest.raises(_ffi.T2DError) as ei:
            fn()
        assert ei.value.code == code and text in str(ei.value), (code, text, str(ei.value))

    def raw(pool, so, vo, xy, soe, ro_, th=thr):
        p = lambda a: None if a is None else a.ctypes.data
        pool._ck(pool._lib.t2d_set_routes(pool._h, len(so) - 1, p(so), p(vo), p(xy), p(soe), p(ro_), p(th)))

    fresh = ParticipantPool(n_env, A)
    try:
        refused(_ffi.ERR_STATE, "must precede t2d_off_route", lambda: fresh.off_route())
        refused(_ffi.ERR_STATE, "t2d_set_route_assignment", lambda: fresh.set_route_assignment(ro, thr))
        fresh.set_routes([routes], None, ro, thr)
        refused(_ffi.ERR_STATE, "t2d_reset", lambda: fresh.off_route())             # no parameter table, no reset
        fresh.set_param_table(H.shape_rows())
        refused(_ffi.ERR_STATE, "t2d_reset", lambda: fresh.off_route())
    finally:
        fresh.close()

    pool = _simple_pool(n_env, A, x, y)
    other = _simple_pool(2, A + 1, np.zeros(2 * (A + 1)), np.zeros(2 * (A + 1)))
    try:
        refused(_ffi.ERR_STATE, "t2d_off_route_buffers", lambda: pool.off_route_buffers())
        pool.set_routes([routes], None, ro, thr)
        want = R.evaluate_sets([routes], np.zeros(n_env, int), ro, A, x, y, thr, np.ones(n))
        so, vo, xy = routes_to_csr([routes])
        ok = lambda what: _same(pool.off_route_host(), want, what)
        ok("installed")
        refused(_ffi.ERR_INVALID, "decreases", lambda: raw(pool, i32([0, 2, 1]), vo, xy, None, ro))
        refused(_ffi.ERR_INVALID, "start at 0", lambda: raw(pool, i32([1, 2]), vo, xy, None, ro))
        refused(_ffi.ERR_INVALID, "vertices", lambda: raw(pool, so, i32([0, 1, 5]), xy, None, ro))       # a one-vertex route
        refused(_ffi.ERR_INVALID, "vertices", lambda: raw(pool, so, i32([0, 3, 2]), xy, None, ro))       # non-monotone
        refused(_ffi.ERR_INVALID, "set_of_env[2]", lambda: raw(pool, so, vo, xy, i32([0, 0, 1, 0]), ro))
        refused(_ffi.ERR_INVALID, "set_of_env[0]", lambda: raw(pool, so, vo, xy, i32([-1, 0, 0, 0]), ro))
        bad = ro.copy(); bad[5] = 2
        refused(_ffi.ERR_INVALID, "route_of[5]", lambda: raw(pool, so, vo, xy, None, bad))
        refused(_ffi.ERR_INVALID, "route_of[5]", lambda: pool.set_route_assignment(bad, None))
        bad[5] = -2
        refused(_ffi.ERR_INVALID, "route_of[5]", lambda: pool.set_route_assignment(bad, None))
        ok("after the refused set routes")
        # trace routes
        buf = _TrajBuffer(pool, 8)
        foreign = _TrajBuffer(other, 8)
        for k in range(8):
            buf.write(k, np.zeros((6, n), np.float32) + k)

        def traj(b, n_slots, se=None, first=None, last=None, ro_=None):
            p = lambda a: None if a is None else a.ctypes.data
            pool._ck(pool._lib.t2d_set_routes_from_traj(pool._h, b._live(), n_slots, p(se), p(first), p(last), p(ro_), p(thr)))

        refused(_ffi.ERR_INVALID, "max_agents", lambda: traj(foreign, 8, i32([0, 1, 0, 1])))
        refused(_ffi.ERR_INVALID, "n_slots", lambda: traj(buf, 9))
        refused(_ffi.ERR_INVALID, "n_slots", lambda: traj(buf, 0))
        refused(_ffi.ERR_INVALID, "src_env[1]", lambda: traj(buf, 8, i32([0, 4, 0, 0])))
        w0, w1 = np.zeros(n, np.int32), np.full(n, 7, np.int32)
        w1[3] = 8
        refused(_ffi.ERR_INVALID, "source participant 3", lambda: traj(buf, 8, None, w0, w1))
        w1[3], w0[2] = 7, -1
        refused(_ffi.ERR_INVALID, "source participant 2", lambda: traj(buf, 8, None, w0, w1))
        refused(_ffi.ERR_INVALID, "both window arrays", lambda: traj(buf, 8, None, w0, None))
        bad = (np.arange(n) % A).astype(np.int32); bad[6] = A
        refused(_ffi.ERR_INVALID, "route_of[6]", lambda: traj(buf, 8, None, None, None, bad))
        ok("after the refused trace routes")
        w0[2], w1[2] = 5, 4     # first > last is legal: no route
        traj(buf, 8, None, w0, w1)
        pool.route_kind = "traces"
        got = pool.off_route_host()
        assert np.isnan(got[0].reshape(-1)[2]) and np.isfinite(got[0].reshape(-1)[[0, 1, 3]]).all()
        refused(_ffi.ERR_STATE, "still replay", lambda: buf.close())          # a bound trajectory outlives its binding
        bad[6] = A
        refused(_ffi.ERR_INVALID, "route_of[6]", lambda: pool.set_route_assignment(bad, None))
        pool.set_routes([routes], None, ro, thr)      # one kind at a time: installing sets releases the trajectory
        ok("sets again")
        buf.close()
        foreign.close()
        pool.clear_routes()
        refused(_ffi.ERR_STATE, "must precede t2d_off_route", lambda: pool.off_route())
    finally:
        other.close()
        pool.close()


# ------------------------------------------------------------------------------------------------------ launches
def test_only_off_route_launches_the_kernel_and_the_step_form_does_not_move():
    """kernel id 9 of t2d_profile_read: 0 launches after t2d_step, t2d_step_n, t2d_integrate and t2d_collide, with and without
    routes; exactly one per t2d_off_route, and per step() / check_status() of a manager with a route installed"""
    from tactics2d_amd import layout as L, scenarios as S
    from tactics2d_amd.traffic import BatchedScenarioManager, OffRoute
    sc = S.highway(32, 64, seed=2)
    pool = _pool(sc)
    try:
        rng = np.random.default_rng(1)
        pool.set_actions(*sc.sample_actions(rng))
        forms = (pool.step_form(1), pool.step_form(8))

        def stepping_calls():
            pool.profile_enable(True)
            pool.step(sc.interval_ms); pool.step_n(8, sc.interval_ms); pool.integrate(sc.interval_ms); pool.collide()
            n9 = pool.profile_read(L.PROFILE_OFF_ROUTE)[1]
            others = sum(pool.profile_read(k)[1] for k in range(9))
            return n9, others

        n9, others = stepping_calls()
        assert n9 == 0 and others > 0
        sets, soe, ro, thr = RS.build(sc, "shared")
        pool.set_routes(sets, None, ro, thr)
        assert (pool.step_form(1), pool.step_form(8)) == forms
        n9, others2 = stepping_calls()
        assert n9 == 0 and others2 == others
        pool.off_route(); pool.off_route()
        ms, n9 = pool.profile_read(L.PROFILE_OFF_ROUTE)
        assert n9 == 2 and ms > 0
        pool.profile_enable(False)
    finally:
        pool.close()

    m = BatchedScenarioManager(sc.n_env, sc.A, max_step=2000, step_size=sc.interval_ms)
    try:
        sc.load(m.pool)
        det = OffRoute(0.2, m)
        with pytest.raises(ValueError):
            det.update()
        m.pool.profile_enable(True)
        m.step(*sc.sample_actions(rng))                       # no route installed yet: no launch
        assert m.pool.profile_read(L.PROFILE_OFF_ROUTE)[1] == 0
        det.reset(route_sets=sets, route_of=ro)
        m.pool.profile_enable(True)
        m.step(*sc.sample_actions(rng))
        m.check_status()
        assert m.pool.profile_read(L.PROFILE_OFF_ROUTE)[1] == 2
        off_all, d_ego = det.update(ego_only=False), det.distance()   # (read from the launch behind the step: no further one)
        assert m.pool.profile_read(L.PROFILE_OFF_ROUTE)[1] == 2
        x, y, active = _xy_active(m.pool)
        want = R.evaluate_sets(sets, soe, ro, sc.A, x, y, np.full(sc.n, 0.2, np.float32), active)
        _same((det.distance(ego_only=False), off_all), want, "manager")
        assert off_all.shape == (sc.n_env, sc.A) and det.update().shape == (sc.n_env,) and d_ego.shape == (sc.n_env,)
        assert 0 < off_all.mean() < 1
        # the reference's form: one polyline for everybody
        det.reset([(-210.0, 1.875), (0.0, 1.875), (210.0, 1.875)])
        got = det.update(ego_only=False)
        want = R.evaluate_sets([[np.float32([(-210.0, 1.875), (0.0, 1.875), (210.0, 1.875)])]], np.zeros(sc.n_env, int),
                               np.zeros(sc.n, int), sc.A, x, y, np.full(sc.n, 0.2, np.float32), active)
        _same((det.distance(ego_only=False), got), want, "one polyline")
    finally:
        m.close()
