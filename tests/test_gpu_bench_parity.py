"""The line bench.py times, held to the oracle at the size it is timed at.

bench.py steps the metric scene (4096 envs x 64 participants) with the fast integrator through t2d_step_n fragments of 32,
auto-reset on.  At that size the fast variant runs the RESUMMED kinematic step (the pool fills the GPU), which the exact
tests of smaller scenes never reach.  Here bench.py's own objects (build_scene, Runner) are stepped one fused launch at a
time and every step is checked against the oracle teacher-forced from the pool's own fp32 state:
  * flags and env flags of every env the step did not end == oracle.collide on the pool's stored poses;
  * the step's record (status bytes, reward) == oracle.status on those flags and the pre-step counters;
  * an env the step ended holds its snapshot bit for bit (state, ids, counters), its status that of the terminal step;
  * the state == oracle.integrate within the bounds of the fast variant (tests/test_gpu_configs.py, metric size);
and a second Runner stepped through t2d_step_n (32, then 2, 7, 31) equals the one-step pool bit for bit at every fragment
end -- so every step of the timed line is pinned, not only the fragment ends.  Last, the outputs bench.py --dump-outputs
writes are held to the oracle's flags."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAGMENTS = (32, 2, 7, 31)   # bench.py --fragment's default, then mixed lengths
BENCH_FORM = "chain"         # what t2d_step_form names for the metric pool's fragments of 32
ACTION_SEED = 1000           # bench.py's Runner of rank 0
STATE_SAMPLE_ENVS = 1024     # the stressed run checks the state of a fixed sample of envs (flags and status: every env)


def _metric_scene(stressed):
    import bench
    sc = bench.build_scene("metric", 4096, 64, seed=0)
    if not stressed:
        return sc
    # tests/test_gpu_configs.py's stress jitter of the metric scene, and a time limit that ends every episode within six
    # steps: the auto-reset restores envs many times inside every fragment
    sc = copy.copy(sc)
    rng = np.random.default_rng(17)
    sc.x = (sc.x + rng.normal(0, 3.0, sc.n)).astype(np.float32)
    sc.y = (sc.y + rng.normal(0, 3.0, sc.n)).astype(np.float32)
    sc.heading = np.mod(sc.heading + rng.normal(0, 0.3, sc.n), 2 * np.pi).astype(np.float32)
    sc.status = dict(sc.status, max_step=5)
    return sc


def _sync():
    import torch
    torch.cuda.synchronize()


def _state(pool):
    from tactics2d_amd import layout as L
    return [pool.download(f) for f in (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY)]


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8).reshape(a.shape[0], -1) if a.ndim else a.view(np.uint8)


def _all_fields(pool, first_step, n_steps):
    """every per-participant and per-env field, and the record slots of steps [first_step, first_step + n_steps)"""
    from tactics2d_amd import layout as L
    fields = (L.F_X, L.F_Y, L.F_HEADING, L.F_SPEED, L.F_VX, L.F_VY, L.F_APPLIED0, L.F_APPLIED1, L.F_IDS, L.F_FLAGS,
              L.F_ENV_FLAGS, L.F_CNT_STEP, L.F_FRAME_MS, L.F_STATUS, L.F_REWARD, L.F_IOU, L.F_CNT_NO_ACTION)
    out = {f: pool.download(f) for f in fields}
    rec = pool.download(L.F_RECORD)
    for k in range(first_step, first_step + n_steps):
        out[("record", k)] = rec[k % L.RECORD_RING]
    return out


class _Checker:
    """one fused step of a Runner held to the oracle (see the module docstring)"""

    def __init__(self, O, run, state_envs):
        from tactics2d_amd import layout as L
        self.O, self.run, self.sc = O, run, run.scene
        sc = self.sc
        self.a0, self.a1 = run.a0.cpu().numpy(), run.a1.cpu().numpy()
        _sync()
        self.snap = _state(run.pool) + [run.pool.download(L.F_IDS)]
        model = sc.rows[sc.type_id, L.P_MODEL].astype(int)
        act = sc.active.astype(bool)
        self.kin = act & (model != L.MODEL_DYNAMICS)
        self.dyn = act & (model == L.MODEL_DYNAMICS)
        self.cfg = O.make_config(**sc.status)
        assert not (sc.status.get("check_arrival") or sc.status.get("check_no_action") or sc.status.get("shaped_reward"))
        self.state_parts = np.zeros(sc.n, bool)
        self.state_parts.reshape(sc.n_env, sc.A)[state_envs] = True
        self.env_steps = self.ended = self.state_checked = self.dyn_checked = 0
        self.seen = {b: np.zeros(sc.n, bool) for b in (L.FLAG_COLLISION_DYNAMIC | L.FLAG_COLLISION_STATIC,
                                                        L.FLAG_OUT_BOUND, L.FLAG_OFF_LANE)}

    def step(self):
        from tactics2d_amd import layout as L
        O, run, sc = self.O, self.run, self.sc
        pool = run.pool
        E, A = sc.n_env, sc.A
        _sync()
        pre = _state(pool)
        cnt, frame = pool.download(L.F_CNT_STEP), pool.download(L.F_FRAME_MS)
        s = run.k % len(self.a0)                        # the action set Runner.steps_single binds for this step
        run.steps_single(1)
        _sync()
        post = _state(pool)
        ids, flags, env_flags = pool.download(L.F_IDS), pool.download(L.F_FLAGS), pool.download(L.F_ENV_FLAGS)
        rec = pool.download(L.F_RECORD)[(pool.step_count() - 1) % L.RECORD_RING]
        st_rec = np.ascontiguousarray(rec[:, 1]).view(np.uint8).reshape(E, 4)
        rw_rec = np.ascontiguousarray(rec[:, 0]).view(np.float32)
        ended = (st_rec[:, 2] | st_rec[:, 3]) != 0
        live = ~ended
        live_p = np.repeat(live, A)
        tag = f"step {pool.step_count()}"

        # flags of every env the step did not end: the oracle's event step on the pool's own fp32 poses
        wf, we = O.collide(sc.rows, E, A, post[0], post[1], post[2], sc.type_id, sc.active, sc.static, sc.boundary,
                           sc.boundary_valid, sc.lanes, 1)
        bad = (wf != flags) & live_p
        assert not bad.any(), (tag, "flags", int(bad.sum()), np.nonzero(bad)[0][:8])
        assert np.array_equal(we[live], env_flags[live]), (tag, "env flags", int((we[live] != env_flags[live]).sum()))
        # the step's record: the oracle's status chain on those flags and the pre-step counters
        c, fr = cnt.copy(), frame.copy()
        wst, wrw = O.status(self.cfg, E, A, flags, sc.interval_ms, c, fr)
        assert np.array_equal(wst, st_rec), (tag, "status", int((wst != st_rec).any(1).sum()))
        assert np.abs(wrw.astype(np.float64) - rw_rec).max() <= 2e-6, (tag, "reward")
        assert np.array_equal(pool.download(L.F_STATUS), st_rec), (tag, "status field")
        assert np.array_equal(_bits(pool.download(L.F_REWARD)), _bits(rw_rec)), (tag, "reward field")
        assert np.array_equal(pool.download(L.F_CNT_STEP), np.where(ended, 0, c)), tag
        assert np.array_equal(pool.download(L.F_FRAME_MS), np.where(ended, 0, fr)), tag
        # envs the step ended: back at the snapshot, bit for bit
        end_p = ~live_p
        for k, (g, w) in enumerate(zip(post + [ids], self.snap)):
            assert np.array_equal(_bits(g[end_p]), _bits(w[end_p])), (tag, "restored field", k)
        assert np.array_equal(ids[live_p], self.snap[6][live_p]), tag
        # state: the oracle teacher-forced from the pool's pre-step state, within the fast variant's bounds
        m = self.state_parts & live_p
        O.set_trig(1)
        try:
            o = O.integrate(sc.rows, *(a[m] for a in pre), self.a0[s][m], self.a1[s][m], sc.type_id[m], sc.active[m],
                            sc.interval_ms)
        finally:
            O.set_trig(0)
        kin, dyn = self.kin[m], self.dyn[m] & (np.abs(pre[3][m]) >= 1.0)
        for col in range(4):
            got = post[col][m].astype(np.float64)
            d = np.abs(got - o[:, col])
            if col == 2:
                d = np.minimum(d, 2 * np.pi - d)
            bound = 0.5 * np.spacing(np.abs(post[col][m])) + 1e-8 if col < 2 else 1e-6
            assert (d[kin] <= (bound[kin] if col < 2 else bound)).all(), (tag, "state", col, float(d[kin].max()))
            # dynamics: the 1e-5 contract on top of the fp32 store (half an ulp is 7.6e-6 at 128 m, 1.5e-5 at 256 m)
            d_dyn = d - 0.5 * np.spacing(np.abs(post[col][m]))
            assert (d_dyn[dyn] <= 1e-5).all(), (tag, "dynamics state", col, float(d_dyn[dyn].max()))
        self.dyn_checked += int(dyn.sum())
        self.env_steps += E
        self.ended += int(ended.sum())
        self.state_checked += int(m.sum())
        for b, seen in self.seen.items():
            seen |= (flags & b) != 0


def _bench_runners(stressed):
    import torch
    import bench
    dev = torch.device("cuda", 0)
    sc = _metric_scene(stressed)
    single = bench.Runner(sc, dev, "fast", seed=ACTION_SEED)
    chain = bench.Runner(sc, dev, "fast", seed=ACTION_SEED)
    return sc, single, chain


@pytest.mark.parametrize("stressed", [False, True], ids=["bench_scene", "stressed"])
def test_the_benchmarked_step_against_the_oracle_at_metric_size(oracle, stressed):
    sc, single, chain = _bench_runners(stressed)
    oracle.set_threads(min(16, os.cpu_count() or 1))
    try:
        form = chain.pool.step_form(FRAGMENTS[0])
        assert form == BENCH_FORM, f"the timed region's fragments of {FRAGMENTS[0]} take the form {form!r}, not {BENCH_FORM!r}"
        all_envs = np.arange(sc.n_env)
        envs = np.sort(np.random.default_rng(8).choice(sc.n_env, STATE_SAMPLE_ENVS, replace=False)) if stressed else all_envs
        check = _Checker(oracle, single, envs)
        for frag in FRAGMENTS:
            first = single.pool.step_count()
            assert chain.pool.step_count() == first
            single.k = chain.k = 0    # step j of a fragment reads action set j of the ring (Runner.steps_chain): so does the single pool
            chain.steps_chain(frag, frag)
            for _ in range(frag):
                check.step()
            _sync()
            a, b = _all_fields(chain.pool, first, frag), _all_fields(single.pool, first, frag)
            for f in a:
                assert np.array_equal(_bits(a[f]), _bits(b[f])), (f"fragment of {frag} from step {first}", f,
                                                                 int((_bits(a[f]) != _bits(b[f])).any(-1).sum()))
    finally:
        oracle.set_threads(1)
        single.close()
        chain.close()
    counts = {name: int(check.seen[b].sum()) for name, b in zip(("collision", "out_of_bound", "off_lane"), check.seen)}
    print(f"metric scene ({'stressed' if stressed else 'as bench.py steps it'}): form {form!r} for fragments of {FRAGMENTS[0]}; "
          f"{check.env_steps} env-steps checked ({check.ended} ended an episode), {check.state_checked} participant states "
          f"against the oracle ({check.dyn_checked} of them dynamics at |v| >= 1 m/s); participants with each event bit: {counts}")
    assert all(v >= 100 for v in counts.values()), counts
    assert check.ended >= 0.01 * check.env_steps, (check.ended, check.env_steps)


def test_the_dumped_outputs_of_the_plain_line_against_the_oracle(oracle, tmp_path):
    """bench.py's plain line at the metric size with --dump-outputs: the flags it wrote are the oracle's event step on the
    poses it wrote, for every env not ended by the last timed step"""
    import bench
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "4096", "--steps", "40",
                          "--warmup", "8", "--clock-warm", "100", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr[-1500:]
    line = json.loads(out.stdout.strip().splitlines()[-1])
    assert line["steps"] == 40
    d = {k: np.load(tmp_path / (k + ".npy")) for k in ("x", "y", "heading", "flags", "status")}
    sc = bench.build_scene("metric", 4096, 64, 0)
    assert d["x"].shape == (sc.n,) and d["status"].shape == (sc.n_env, 4)
    oracle.set_threads(min(16, os.cpu_count() or 1))
    try:
        wf, _ = oracle.collide(sc.rows, sc.n_env, sc.A, d["x"], d["y"], d["heading"], sc.type_id, sc.active, sc.static,
                               sc.boundary, sc.boundary_valid, sc.lanes, 1)
    finally:
        oracle.set_threads(1)
    live = np.repeat((d["status"][:, 2] == 0) & (d["status"][:, 3] == 0), sc.A)
    assert live.mean() > 0.5
    bad = (wf != d["flags"].astype(np.uint32)) & live
    assert not bad.any(), (int(bad.sum()), np.nonzero(bad)[0][:8])
    assert (d["flags"][live] != 0).mean() > 0.05
