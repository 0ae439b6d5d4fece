"""-m gpu: `bench.py --dump-outputs DIR` -- the arrays the last timed step computed, the same in every run with the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bench
from mimrl_amd import _lib, layout, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out, prewarm_ms, steps, deterministic):
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("MIMRL_DETERMINISTIC", None)
    if deterministic:        # fixed-point accumulation instead of float atomics: bit-identical run to run
        env["MIMRL_DETERMINISTIC"] = "1"
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--steps", str(steps), "--warmup", "2", "--prewarm-ms", str(prewarm_ms),
           "--profile-steps", "0", "--no-cpu-baseline", "--no-extra", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def _load(d):
    return {f: np.load(d / f) for f in sorted(os.listdir(d))}


@pytest.mark.gpu
def test_bench_dump_outputs_are_bit_identical_in_the_deterministic_build(tmp_path):
    """Runs with different numbers of untimed pre-warm steps and of timed steps write the same files, bit for bit: the last timed
    step starts from a fixed seeded state.  Float32 arrays, 64 MB at most."""
    a = _bench(tmp_path / "a", 0, 3, True)
    b = _bench(tmp_path / "b", 300, 5, True)
    assert a["steps"] == 3 and b["steps"] == 5 and a["prewarm_steps"] == 0 and b["prewarm_steps"] > 0
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert list(da) == list(db)
    assert {"scalars.npy", "pred.npy", "feats.npy", "param.W_t.weight.npy", "adam_m.W_t.weight.npy", "adam_v.W_t.weight.npy"} <= set(da)
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in da) <= 64 << 20
    for f, x in da.items():
        assert x.dtype == np.float32 and np.isfinite(x).all(), f
        assert np.array_equal(x, db[f]), f
    s = da["scalars.npy"]
    assert s[_lib.S1_LOSS] == a["stage1_loss"] and s[_lib.S2_LOSS] == a["stage2_loss"]


@pytest.mark.gpu
def test_plain_run_measures_the_headline_only():
    """Without --full the run starts no child process, no eager profile and no CPU baseline: the line carries the headline and the
    roofline of the timed region's launch stamps, none of the figures --full adds."""
    env = dict(os.environ, PYTHONPATH=ROOT)
    env.pop("MIMRL_DETERMINISTIC", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "10", "--warmup", "2"], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert d["config"]["full"] is False and d["steps"] == 10 and d["losses_finite"]
    assert abs(d["value"] - 1e3 / d["ms_per_step"]) < 1e-6 * d["value"]
    assert d["cpu_baseline"] is None and d["phases"] == {}
    assert not {"ms_per_step_sequential", "ms_per_step_fresh_batch", "cfg3", "deterministic_build", "extras_error"} & set(d)
    assert d["roofline"]["launches_timed"] == 2 * 10


@pytest.mark.gpu
def test_bench_dump_outputs_agree_to_rounding_in_the_default_build(tmp_path):
    """The timed build (float atomics): two runs agree to rounding in every dumped array, measured against the array's own scale
    (measured at most 1e-6; from the initial state, where some outputs are pure rounding residue and Adam's first step is lr * sign(g),
    it was 0.2 -- bench.seeded_dump_state).  The step did move the parameters.  --steps is the number of timed steps: two
    recurrence-backward launches per step in the in-graph launch stamps."""
    opt, _ = bench.workload("cfg2")
    a = _bench(tmp_path / "a", 0, 20, False)
    b = _bench(tmp_path / "b", 100, 30, False)
    assert a["roofline"]["launches_timed"] == 2 * 20 and b["roofline"]["launches_timed"] == 2 * 30
    da, db = _load(tmp_path / "a"), _load(tmp_path / "b")
    assert list(da) == list(db)
    for f, x in da.items():
        scale = float(np.abs(x).max())
        assert scale > 0, f
        assert float(np.abs(x - db[f]).max()) <= 1e-5 * scale, f
    shapes = layout.named_shapes(opt, 768, 74, 35)
    w0 = synth.portable_state(shapes, 0)["W_t.weight"]
    assert np.abs(da["param.W_t.weight.npy"] - w0).mean() > 1e-2 * opt.learning_rate
