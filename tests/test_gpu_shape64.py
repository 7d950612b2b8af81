"""The W64 twins of the plain step and the plain chained step: collide_kernel<..., W64> has the shape of the
metric pool compiled in -- envs of 64 participants, four per workgroup of 256 threads, a wave = an env -- and, in the chained
twins, the env's number and base index in scalar registers.  It is the same step: every output must equal, bit for bit, what the generic instantiation leaves behind on
the same pool (t2d_debug_set_step_shape64(pool, 0) keeps a pool on the generic one; t2d_debug_last_step_shape tells which ran).
(Reference: traffic/scenario_manager.py:63-98, one Python loop whatever the number of participants.)

Pool sizes: the smallest at which the plan takes W64 in each form on a device of 256 CUs -- 513 envs for one launch per step (up
to 512 envs the geometry layout puts two envs or one into a workgroup, so that every CU gets one: those pools keep the generic
form), 2201 envs = 551 workgroups, more than two per CU, for the chained form -- with n_env = 1 mod 4, so that the last workgroup
holds three waves past the pool."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

_scenes = {}


def _scene(name):
    from tactics2d_amd import scenarios as S
    if name not in _scenes:
        _scenes[name] = {"small": lambda: S.mixed(513, 64, seed=5), "big": lambda: S.mixed(2201, 64, seed=9),
                         "highway": lambda: S.highway(513, 64, seed=5)}[name]()
    return _scenes[name]


def _fields():
    from tactics2d_amd import layout as L
    return (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY, L.F_APPLIED0, L.F_APPLIED1, L.F_IDS, L.F_FLAGS, L.F_ENV_FLAGS,
            L.F_CNT_STEP, L.F_FRAME_MS, L.F_STATUS, L.F_REWARD, L.F_RECORD, L.F_IOU)


def _pool(sc, variant, shape64, chaining=1, split=True):
    from tactics2d_amd import debug as D
    p = D.pool(sc.n_env, sc.A)
    sc.load(p)
    p.set_integrator_variant(variant)
    p.set_auto_reset(True)
    p.set_step_chaining(chaining)
    p.set_split_step(split)
    D.set_step_shape64(p, shape64)
    return p


def _action_ring(sc, n_steps, seed=4, spoil=None):
    torch = pytest.importorskip("torch")
    rng = np.random.default_rng(seed)
    sets = [sc.sample_actions(rng) for _ in range(n_steps)]
    if spoil is not None:
        for s in sets:
            s[0][spoil] = np.nan
    dev = torch.device("cuda", 0)
    return (torch.from_numpy(np.stack([s[0] for s in sets])).to(dev).contiguous(),
            torch.from_numpy(np.stack([s[1] for s in sets])).to(dev).contiguous())


def _both(sc, variant, schedule, form, spoil=None, **pool_kw):
    """the same seeded action ring through a W64 pool and a pool kept on the generic instantiation; `schedule` = the calls, 1 = a
    t2d_step, n > 1 = a t2d_step_n fragment of n.  Every field and every record slot is compared after every call."""
    from tactics2d_amd import debug as D, layout as L
    n_steps = sum(schedule)
    a0, a1 = _action_ring(sc, n_steps, spoil=spoil)
    pools = [_pool(sc, variant, on, **pool_kw) for on in (True, False)]
    try:
        done = 0
        for c in schedule:
            got = []
            for p, want_shape in zip(pools, (64, 0)):
                assert p.step_form(c) == form, (p.step_form(c), form)
                p.bind_actions(a0.data_ptr() + 4 * sc.n * done, a1.data_ptr() + 4 * sc.n * done)
                if c == 1:
                    p.step(sc.interval_ms)
                else:
                    p.step_n(c, sc.interval_ms, sc.n)
                assert D.last_step_shape() == want_shape, (c, D.last_step_kernel(), D.last_step_shape())
                got.append([p.download(f) for f in _fields()])
            done += c
            for f, g, w in zip(_fields(), *got):
                assert np.array_equal(g, w, equal_nan=True), (f, done, int((g != w).sum()))
        rec = got[0][_fields().index(L.F_RECORD)].reshape(L.RECORD_RING, sc.n_env, 2)
        return rec[:n_steps, :, 1], got[0]
    finally:
        for p in pools:
            p.close()


@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_one_launch_steps_of_the_w64_form_equal_the_generic_form(variant):
    sc = _scene("small")   # (one workgroup per env is this pool's default: split off brings it to the plain step)
    status, _ = _both(sc, variant, (1,) * 12, "step", split=False)
    ended = (status >> 16).astype(bool)   # terminated or truncated
    print(f"episodes ended in {ended.mean():.3f} of the env-steps")
    assert ended.any(), "no episode ended: the restore of finished envs was not exercised"


@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_chained_fragments_of_the_w64_form_equal_the_generic_form(variant):
    sc = _scene("big")
    status, _ = _both(sc, variant, (3, 3, 5, 5), "chain")
    ended = (status >> 16).astype(bool)
    print(f"episodes ended in {ended.mean():.3f} of the env-steps")
    assert ended.any(), "no episode ended: the restore of finished envs was not exercised"


def _awkward():
    """64-wide envs with empty slots, and a NaN x, an infinite heading and a NaN action in single lanes"""
    import copy
    sc = copy.deepcopy(_scene("small"))
    act = sc.active.reshape(sc.n_env, sc.A)
    act[:, 61:] = 0          # every env: three empty slots at the end
    act[2, 5:40:3] = 0       # ... one env with holes
    act[4, 1:] = 0           # ... one env with the ego alone
    live = np.flatnonzero(sc.active)
    nan_x, inf_h, nan_a = (int(live[live // sc.A == e][3]) for e in (1, 3, 512))   # (512: the last workgroup's only env)
    sc.x[nan_x] = np.nan
    sc.heading[inf_h] = np.inf
    return sc, nan_x, nan_a


@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_awkward_envs_one_launch_per_step(variant):
    sc, nan_x, nan_a = _awkward()
    _, last = _both(sc, variant, (1,) * 6, "step", spoil=nan_a, split=False)
    x = last[0]
    assert np.isnan(x[nan_x]) and not np.isfinite(x[nan_a]), "the non-finite lanes did not stay non-finite"


@pytest.mark.parametrize("variant", ["exact", "fast"])
def test_awkward_envs_chained(variant):
    """(chained on request: the pool is too small for the plan to chain it)"""
    sc, nan_x, nan_a = _awkward()
    _, last = _both(sc, variant, (3, 5, 3), "chain", spoil=nan_a, chaining=2, split=False)
    assert np.isnan(last[0][nan_x])


def _narrowed(sc):
    """the scene with so many (far away) static polygons per env that four envs no longer fit a workgroup's record, and two do"""
    import copy
    from tactics2d_amd import mapgeom
    out = copy.deepcopy(sc)
    for per_env in range(24, 400, 8):
        q = np.arange(per_env, dtype=np.float32)
        sq = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
        one = (sq[None] + np.stack([3000 + 3 * q, np.full_like(q, 3000)], 1)[:, None]).reshape(-1, 2)
        n = sc.n_env * per_env
        out.static = (np.arange(sc.n_env + 1, dtype=np.int32) * per_env, np.arange(n + 1, dtype=np.int32) * 4, np.tile(one, (sc.n_env, 1)))
        b = mapgeom.geometry_budget(sc.n_env, sc.A, out.static, out.lanes)   # (of ONE env: a wave of this pool)
        if 4 * b["dwords_needed"] > 1.2 * b["dwords_budget"] and 2 * b["dwords_needed"] < 0.9 * b["dwords_budget"]:
            return out
    raise AssertionError("no polygon count leaves room for two envs and not for four")


def test_the_plan_takes_w64_for_full_64_wide_envs_four_per_workgroup_only():
    from tactics2d_amd import debug as D, scenarios as S
    rng = np.random.default_rng(0)

    def shapes(sc, **kw):
        p = _pool(sc, "fast", True, **kw)
        try:
            a0, a1 = sc.sample_actions(rng)
            p.set_actions(a0, a1)
            forms = (p.step_form(1), p.step_form(4))
            p.step(sc.interval_ms)
            one = (D.last_step_kernel(), D.last_step_shape())
            p.step_n(4, sc.interval_ms, 0)
            return forms, one, (D.last_step_kernel(), D.last_step_shape())
        finally:
            p.close()

    hw = _scene("highway")
    forms, one, many = shapes(hw)   # the pool's defaults: the plain step takes W64; a fragment goes to the PIPE form, which has no twin
    assert forms == ("step", "loop_pipe") and one == ("(true, 1, false)", 64) and many[1] == 0, (forms, one, many)
    forms, one, many = shapes(hw, chaining=2)   # ... chained on request
    assert forms == ("step", "chain") and one == ("(true, 1, false)", 64) and many == ("(true, 1, false, true)", 64), (forms, one, many)
    for sc in (S.highway(513, 63, seed=5), S.intersection(1025, 32, seed=8), S.highway(97, 64, seed=5)):   # envs that do not fill a wave; one env per workgroup
        forms, one, many = shapes(sc, chaining=2, split=False)
        assert forms == ("step", "chain") and one == ("(true, 1, false)", 0) and many == ("(true, 1, false, true)", 0), (sc.A, forms, one, many)
    narrow = _narrowed(hw)   # a record that narrows the workgroup to two envs
    forms, one, many = shapes(narrow, chaining=2, split=False)
    assert forms == ("step", "chain") and one == ("(true, 1, false)", 0) and many == ("(true, 1, false, true)", 0), (forms, one, many)
