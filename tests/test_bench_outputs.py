"""bench.py's plain line and --dump-outputs: what the last timed step computed, written as .npy files that two builds run
with the same arguments can be compared by.  The dump logic runs on the CPU against a fake pool; the GPU test runs the
plain line twice and requires identical outputs."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tactics2d_amd import layout as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATE = ("x", "y", "heading", "speed")
ALL = STATE + ("vx", "vy", "applied_accel", "applied_steer")
FULL_ONLY = ("alternates", "value_without_clock_ramp", "configs", "next_rows", "closed_loop", "strong")


class FakePool:
    """download / step_count as ParticipantPool has them: participant field f holds 1000 f + its index, the record of
    step s holds reward s + env / 1000 and status bytes (s, env, 0, 1) mod 256"""

    def __init__(self, n_env, A, steps):
        self.n_env, self.n, self.steps = n_env, n_env * A, steps

    def step_count(self):
        return self.steps

    def download(self, field):
        if field == L.F_RECORD:
            rec = np.zeros((L.RECORD_RING, self.n_env, 2), np.uint32)
            for s in range(self.steps - L.RECORD_RING, self.steps):
                e = np.arange(self.n_env)
                rec[s % L.RECORD_RING, :, 0] = (s + e / 1000.0).astype(np.float32).view(np.uint32)
                st = np.stack([np.full_like(e, s), e, 0 * e, 0 * e + 1], 1).astype(np.uint8)
                rec[s % L.RECORD_RING, :, 1] = st.view(np.uint32).reshape(-1)
            return rec
        return (1000 * field + np.arange(self.n)).astype(L.FIELD_DTYPES[field])


def _load(d, names):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in names}


@pytest.mark.parametrize("outputs,names", [("all", ALL), ("state", STATE)])
def test_dump_writes_the_last_steps_state_flags_and_records(tmp_path, outputs, names):
    import bench
    pool = FakePool(6, 4, steps=130)
    bench.dump_outputs(pool, str(tmp_path), outputs)
    want = set(names) | {"flags", "reward", "status"}
    assert {f[:-4] for f in os.listdir(tmp_path)} == want
    got = _load(tmp_path, want)
    assert all(a.dtype in (np.float32, np.float64) for a in got.values())
    assert np.array_equal(got["x"], np.arange(24, dtype=np.float32) + 1000 * L.F_X)
    assert np.array_equal(got["flags"], np.arange(24, dtype=np.float64) + 1000 * L.F_FLAGS)
    e = np.arange(6)
    assert np.array_equal(got["reward"], (129 + e / 1000.0).astype(np.float32))        # step 129 = the last one taken
    assert np.array_equal(got["status"], np.stack([0 * e + 129, e, 0 * e, 0 * e + 1], 1).astype(np.float32))


def test_dump_above_the_limit_is_one_fixed_sample_for_every_field(tmp_path, monkeypatch):
    import bench
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 200_000)
    pool = FakePool(512, 16, steps=70)
    for d in ("a", "b"):
        bench.dump_outputs(pool, str(tmp_path / d), "all")
    a, b = (_load(tmp_path / d, ALL + ("flags", "reward", "status")) for d in ("a", "b"))
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in os.listdir(tmp_path / "a")) <= 200_000
    idx = a["x"].astype(np.int64) - 1000 * L.F_X
    assert 0 < idx.size < 512 * 16 and np.all(np.diff(idx) > 0)
    assert np.array_equal(a["flags"], idx + 1000.0 * L.F_FLAGS)            # the same participants in every array
    assert np.array_equal(a["status"][:, 1], np.round((a["reward"] - 69) * 1000) % 256)   # the same envs in both
    assert all(np.array_equal(a[k], b[k]) for k in a)                      # and the same sample each time


def test_bench_has_the_full_and_dump_outputs_options():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--help"], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-1500:]
    assert "--full" in out.stdout and "--dump-outputs" in out.stdout


@pytest.mark.gpu
def test_plain_line_is_lean_and_its_outputs_repeat(tmp_path):
    """two plain runs with the same arguments: exactly --steps timed steps, the headline keys, none of --full's
    measurements, and bit-identical dumped outputs"""
    lines = []
    for d in ("a", "b"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--envs", "1024", "--steps", "40",
                              "--warmup", "8", "--clock-warm", "100", "--dump-outputs", str(tmp_path / d)],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-1500:]
        lines.append(json.loads(out.stdout.strip().splitlines()[-1]))
    for line in lines:
        assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"} <= set(line)
        assert line["steps"] == 40 and line["ms_per_step"] > 0 and line["value"] > 0
        assert "cpu_baseline" not in line and all(line[k] is None for k in FULL_ONLY)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b")) and {n[:-4] for n in names} == set(ALL) | {"flags", "reward", "status"}
    a, b = (_load(tmp_path / d, [n[:-4] for n in names]) for d in ("a", "b"))
    assert a["x"].shape == (1024 * 64,) and a["status"].shape == (1024, 4)
    for k in a:
        assert a[k].dtype in (np.float32, np.float64) and a[k].tobytes() == b[k].tobytes(), k
