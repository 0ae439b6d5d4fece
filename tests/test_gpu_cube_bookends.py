"""-m gpu: the forward tail's bookends inside the fused CubeMLP blocks (csrc/cube_fused.hip PRE / HEAD modes: block 0 builds its tile from the
encoder outputs, the last block ends in the head) against the same work as launches of their own (tail_pre_kernel, head_fwd_kernel).  Both
forms call the row helpers of csrc/cube_bookends.h and reorder no floating-point operation, so the bar is BIT IDENTITY: the temporal means,
F_F, the prediction, both stages' scalar blocks and the whole main / critic parameter buckets after one two-stage step (the mode bench.py
runs: bf16, shared prefix, device-drawn anchors), and F_F / means / prediction of an eval-mode forward pass, eager and captured.
The comparison runs in the deterministic build (float atomics in the weight-gradient kernels of the default build reorder additions from run to
run, tests/test_gpu_step.py::test_gradients_reproducible), which is a property of the process: one worker process does all cases, two engines
per case in that process (the setting is read per handle)."""
import json
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

SHAPES = ["T5_L8_ragged", "T50_two_blocks", "T50_one_block", "T50_two_blocks_p0"]
ITEMS = ["step_feats", "step_pred", "stage1_scalars", "stage2_scalars", "main_params", "critic_params", "eval_feats", "eval_pred"]
_RUN = {}


def _results(tmp_path_factory):
    if not _RUN:
        d = tmp_path_factory.mktemp("bookends")
        env = dict(os.environ, PYTHONPATH=ROOT, MIMRL_DETERMINISTIC="1")
        for name in [n for n in env if n.startswith("MIMRL_") and n != "MIMRL_DETERMINISTIC"]:
            env.pop(name)
        r = subprocess.run([sys.executable, os.path.join(HERE, "cube_bookends_worker.py"), str(d / "r.json")], env=env, capture_output=True, text=True,
                           timeout=600)
        _RUN["r"] = r
        _RUN["res"] = json.load(open(d / "r.json")) if r.returncode == 0 and "BOOKENDS_DONE" in r.stdout else None
    r = _RUN["r"]
    assert _RUN["res"] is not None, r.stdout[-2000:] + r.stderr[-3000:]
    return _RUN["res"]


@pytest.mark.parametrize("use_graph", [False, True])
@pytest.mark.parametrize("shape", SHAPES)
def test_bookends_bit_identical(shape, use_graph, tmp_path_factory):
    case = _results(tmp_path_factory)[f"{shape}|{int(use_graph)}"]
    print(shape, use_graph, {k: (v["equal"], v["maxdiff"], v["absmax"]) for k, v in case.items()})
    assert sorted(case) == sorted(ITEMS)
    for k in ITEMS:
        v = case[k]
        assert v["finite"] and v["n"] > 0 and v["absmax"] > 0, (k, v)
        assert v["equal"], f"{k}: folded vs separate launches differ by {v['maxdiff']:.3e} (scale {v['absmax']:.3e})"
