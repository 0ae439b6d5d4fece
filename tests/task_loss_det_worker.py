"""Run under MIMRL_DETERMINISTIC=1 by tests/test_gpu_task_loss.py (the library is chosen at import, so the deterministic build gets its own
process).  usage: task_loss_det_worker.py <out.npz>
Three two-stage steps through mimrl_two_stage_step with graphs at the cfg1_sep shape (the deterministic build runs them as its sequential
schedule: no stage-2 prefetch there, so the stage boundary is not fused), one fresh engine per run:  mae_default (no setter call), mae_explicit (set_task_loss(MAE)), mae_switched (MAE -> MSE -> MAE before the first
step), ccc_a and ccc_b (two CCC runs).  Per run: the scalars of every step and both parameter buckets after the last, into <out.npz>."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mimrl_amd import _lib                               # noqa: E402
from mimrl_amd.engine import HipEngine                   # noqa: E402
from tests.helpers import case, load_golden, oracle_params   # noqa: E402

K = _lib.TASK_LOSSES
RUNS = {"mae_default": [], "mae_explicit": [K["MAE"]], "mae_switched": [K["MAE"], K["MSE"], K["MAE"]], "ccc_a": [K["CCC"]], "ccc_b": [K["CCC"]]}


def run(kinds):
    c, opt, batch, banks = case("cfg1_sep")
    anchors = load_golden("cfg1_sep")["anchors"]
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], use_graph=True)
    eng.load_params(oracle_params(opt, c["seed"]))
    eng.set_batch(*batch)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    eng.set_stage2_prefetch(1)
    for k in kinds:
        eng.set_task_loss(k)
    sc = []
    for it in range(3):
        eng.set_anchors(1, anchors[it, 0])
        eng.set_anchors(2, anchors[it, 1])
        eng.step()
        torch.cuda.synchronize()
        sc.append(eng.read_scalars().copy())
    out = {"scalars": np.stack(sc), "main": eng.main["p"].cpu().numpy().copy(), "crit": eng.crit["p"].cpu().numpy().copy()}
    eng.close()
    return out


def main():
    assert _lib.DETERMINISTIC and _lib.load().mimrl_deterministic() == 1, "not the deterministic build"
    res = {}
    for name, kinds in RUNS.items():
        for k, v in run(kinds).items():
            res[f"{name}_{k}"] = v
    assert _lib.load().mimrl_deterministic() == 1, "an accumulation left the order-independent path"
    np.savez(sys.argv[1], **res)
    print("ok", len(res))


if __name__ == "__main__":
    main()
