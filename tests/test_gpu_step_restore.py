"""The fused auto-reset of the step kernel (csrc/t2d_collide.hip).  Where an env is a wave (64-participant envs, the scalar status
epilogue) the restore sits behind ONE scalar branch on the epilogue's verdict: a wave whose env goes on neither fetches the
restore's pointers nor meets at a sync nor reads s_done; envs narrower than a wave (A = 32 here) keep the path through s_done.

Pools of 5 and 9 envs (a last workgroup with waves that own no env) of the mixed scene, fast integrator, fragments of 6 steps,
max_step = 3: every env exceeds its time in step 4 and goes on from the snapshot.  One env's ego stands inside a static obstacle,
so that env is done in EVERY step.  The status configuration is per pool, so the env that never finishes lives in a second pool
with max_step = 0 (no time limit), where the reference run shows envs without any verdict in six steps.  With a SingleTrackDrift
row in the type table the wheel speeds are part of the snapshot and are restored (such a pool steps launch by launch: its drift
kernel runs ahead of every step launch, so the chained form is checked without the row).

Three runs, bit for bit:
    reference   auto-reset OFF: t2d_step, download, then t2d_restore(done envs only) -- separate launches;
    per step    auto-reset on, one t2d_step per step: state, wheel speeds, counters and cnt_na after EVERY step equal the
                reference's after its restore; status, reward, flags and env words equal the reference's before its restore;
    fragment    auto-reset on, one t2d_step_n of 6 steps (the chained form): end state and the six records.
The status chain (status word and reward of every env and step) is held against oracle.status_ex on the run's own flags.
last_valid, max_iou and min_dist have no download field; without IoU events the epilogue never moves them from the values the
restore writes (0, -inf, the snapshot's distance), so cnt_na (T2D_F_CNT_NO_ACTION) is the one detector word observable here."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
N_STEPS = 6
SCENARIO_TIME_EXCEEDED, TRAFFIC_COLLISION_STATIC = 3, 3   # include/t2d.h: T2D_SCENARIO_TIME_EXCEEDED, T2D_TRAFFIC_COLLISION_STATIC


def _drift_row():
    from tactics2d_amd.physics import SingleTrackDrift
    return SingleTrackDrift(lf=1.262, lr=1.375, mass=1620.0, mass_height=0.7245, steer_range=(-0.524, 0.524),
                            speed_range=(-16.67, 69.44), accel_range=(-11.0, 3.121)).param_row()


def _scene(n_env, A, max_step, drift):
    """the mixed scene (env e: highway / roundabout / intersection by e mod 3); the ego (agent 0) of the last env that has a
    static obstacle is put inside it: the roundabout's island (centre 0, 0) or a building of the intersection (centre 14, 14)"""
    from tactics2d_amd import scenarios as S
    sc = S.mixed(n_env, A, seed=5)
    stuck = max(e for e in range(n_env) if e % 3 != 0)
    c = 0.0 if stuck % 3 == 1 else 14.0
    sc.x[stuck * A] = c
    sc.y[stuck * A] = c
    sc.speed[stuck * A] = 0.0
    sc.status.update(max_step=max_step)
    if drift:
        sc.rows = np.concatenate([sc.rows, _drift_row()[None]])
    return sc, stuck


def _ring(sc):
    rng = np.random.default_rng(19)
    sets = [sc.sample_actions(rng) for _ in range(N_STEPS)]
    return np.stack([s[0] for s in sets]), np.stack([s[1] for s in sets])


def _state_fields(drift):
    from tactics2d_amd import layout as L
    return (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY, L.F_IDS, L.F_CNT_STEP, L.F_FRAME_MS, L.F_CNT_NO_ACTION) + \
        ((L.F_OMEGA_F, L.F_OMEGA_R) if drift else ())


def _verdict_fields():
    from tactics2d_amd import layout as L
    return (L.F_FLAGS, L.F_ENV_FLAGS, L.F_STATUS, L.F_REWARD)


def _pool(sc, drift, auto_reset, chaining):
    """a pool at the scene's start.  drift: wheel speeds 3 + i / 7 go into the snapshot and are overwritten afterwards, so
    that a restored participant shows"""
    from tactics2d_amd import layout as L
    from tactics2d_amd.pool import ParticipantPool
    pool = ParticipantPool(sc.n_env, sc.A)
    pool.set_param_table(sc.rows)
    pool.set_static_geometry(sc.static, sc.boundary, sc.boundary_valid)
    pool.set_lane_geometry(sc.lanes)
    pool.set_status_config(**sc.status)
    pool.reset(sc.x, sc.y, sc.heading, sc.speed, sc.type_id, sc.active)
    if drift:
        w = (3.0 + np.arange(sc.n) / 7.0).astype(np.float32)
        pool.upload(L.F_OMEGA_F, w)
        pool.upload(L.F_OMEGA_R, -w)
    pool.snapshot()
    if drift:
        pool.upload(L.F_OMEGA_F, np.full(sc.n, 100.0, np.float32))
        pool.upload(L.F_OMEGA_R, np.full(sc.n, 200.0, np.float32))
    pool.set_integrator_variant("fast")
    pool.set_auto_reset(auto_reset)
    pool.set_split_step(False)
    pool.set_step_chaining(chaining)
    return pool


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _check_restore(oracle, n_env, A, max_step, drift):
    import torch
    from tactics2d_amd import layout as L
    dev = torch.device("cuda", 0)
    sc, stuck = _scene(n_env, A, max_step, drift)
    r0, r1 = _ring(sc)
    a0 = torch.from_numpy(r0).to(dev).contiguous()
    a1 = torch.from_numpy(r1).to(dev).contiguous()
    label = f"{n_env} x {A} max_step {max_step} drift {drift}"

    def bind(pool, k):
        pool.bind_actions(a0.data_ptr() + 4 * sc.n * k, a1.data_ptr() + 4 * sc.n * k)

    # ---- reference: separate launches, the restore through t2d_restore
    ref = _pool(sc, drift, False, 0)
    want = []
    try:
        assert ref.step_form(1) == ("unfused" if drift else "step"), ref.step_form(1)
        for k in range(N_STEPS):
            bind(ref, k)
            ref.step(sc.interval_ms)
            verdict = {f: ref.download(f) for f in _verdict_fields()}
            ref.restore(done_only=True)
            want.append((verdict, {f: ref.download(f) for f in _state_fields(drift)}))
    finally:
        ref.close()

    # ---- the scene does what it is here for (judged on the reference run and the oracle, not on the code under test)
    st = np.stack([w[0][L.F_STATUS] for w in want])                     # [step, env, 4]
    done = (st[:, :, 2] | st[:, :, 3]) != 0
    assert done[:, stuck].all() and (st[:, stuck, 1] == TRAFFIC_COLLISION_STATIC).all(), (label, st[:, stuck].tolist())
    if max_step > 0:   # an env without a verdict in its first max_step steps exceeds its time in the next one
        fresh = ~done[:max_step].any(0)
        assert fresh.any() and (st[max_step, fresh, 0] == SCENARIO_TIME_EXCEEDED).all() and done[max_step, fresh].all(), label
    else:
        assert (~done.any(0)).any(), f"{label}: no env goes through the fragment without a verdict"

    # ---- the status chain against the oracle, on the reference run's flags
    cfg = oracle.make_config(**sc.status)
    ep = oracle.EpisodeState(n_env)
    cnt = np.zeros(n_env, np.int32); frame = np.zeros(n_env, np.int32)
    chain = []
    for k in range(N_STEPS):
        verdict, state = want[k]
        # (status_ex reads the ego's pose only for IoU events, which are off: the start poses will do)
        ost, orw, _ = oracle.status_ex(cfg, A, verdict[L.F_FLAGS], sc.interval_ms, cnt, frame, sc.rows, sc.x, sc.y, sc.heading,
                                       sc.type_id, ep)
        chain.append((ost.copy(), orw.copy()))
        assert np.array_equal(ost, verdict[L.F_STATUS]), (label, k)
        assert np.abs(orw.astype(np.float64) - verdict[L.F_REWARD]).max() <= 2e-6, (label, k)   # (one fp32 ulp of the time-penalty table)
        d = (ost[:, 2] | ost[:, 3]) != 0
        cnt[d] = 0; frame[d] = 0
        ep.reset_envs(d)
        assert np.array_equal(state[L.F_CNT_STEP], cnt) and np.array_equal(state[L.F_FRAME_MS], frame), (label, k)
        assert np.array_equal(state[L.F_CNT_NO_ACTION], ep.cnt_na), (label, k)

    # ---- auto-reset on, one launch per step: everything after every step
    per = _pool(sc, drift, True, 0)
    try:
        for k in range(N_STEPS):
            bind(per, k)
            per.step(sc.interval_ms)
            verdict, state = want[k]
            for f in _verdict_fields():
                assert np.array_equal(_bits(per.download(f)), _bits(verdict[f])), f"{label}: step {k}, field {f}"
            for f in _state_fields(drift):
                g = per.download(f)
                bad = np.flatnonzero(g.view(np.uint32) != state[f].view(np.uint32))
                assert bad.size == 0, f"{label}: step {k}, field {f} differs in {bad.size} places, first {bad[:8].tolist()}"
        per_final = {f: per.download(f) for f in _state_fields(drift) + _verdict_fields()}
        per_record = per.download(L.F_RECORD)
    finally:
        per.close()
    for k in range(N_STEPS):   # the records: {reward bits, status word} of every env and step
        word = chain[k][0].astype(np.uint32) @ np.uint32([1, 1 << 8, 1 << 16, 1 << 24])
        assert np.array_equal(per_record[k, :, 1].view(np.uint32), word.astype(np.uint32)), (label, k)
        assert np.array_equal(per_record[k, :, 0].view(np.uint32), want[k][0][L.F_REWARD].view(np.uint32)), (label, k)

    # ---- auto-reset on, one fragment
    frag = _pool(sc, drift, True, 2)
    try:
        form = frag.step_form(N_STEPS)
        assert form == ("unfused" if drift else "chain"), form
        bind(frag, 0)
        frag.step_n(N_STEPS, sc.interval_ms, sc.n)
        frag.sync()
        for f in _state_fields(drift) + _verdict_fields():
            assert np.array_equal(_bits(frag.download(f)), _bits(per_final[f])), f"{label}: fragment ({form}), field {f}"
        assert np.array_equal(frag.download(L.F_RECORD)[:N_STEPS], per_record[:N_STEPS]), f"{label}: fragment ({form}), records"
    finally:
        frag.close()


@pytest.mark.parametrize("drift", [False, True], ids=["", "drift_row"])
@pytest.mark.parametrize("max_step", [3, 0])
@pytest.mark.parametrize("A", [64, 32])
@pytest.mark.parametrize("n_env", [5, 9])
def test_restore_after_done_steps(oracle, n_env, A, max_step, drift):
    _check_restore(oracle, n_env, A, max_step, drift)


def test_finished_env_in_the_last_partly_invalid_workgroup(oracle):
    """70 envs of 64: 18 workgroups of four waves, the last with envs 68 and 69 and two waves without an env; env 68 is the one
    that is done in every step"""
    sc, stuck = _scene(70, 64, 3, False)
    assert stuck == 68 and stuck // 4 == (70 - 1) // 4
    _check_restore(oracle, 70, 64, 3, False)
