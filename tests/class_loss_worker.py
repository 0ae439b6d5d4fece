"""Run under MIMRL_DETERMINISTIC=1 by tests/test_gpu_class_loss.py (the library is chosen at import, so the deterministic build gets its
own process).  usage: class_loss_worker.py <out.npz> det | head
det:  two runs of three captured two-stage steps at tiny_cls7_ce (fp32), a fresh engine each: the scalars of every step and both
      parameter buckets after the last, as a_* / b_*.
head: ONE engine in bf16 mode (the fused CubeMLP blocks) at tiny_cls7_ce under whatever MIMRL_NO_FUSED_TAIL_PRE the parent set -- unset: the
      head is the last block's epilogue (HEAD mode of cube_fwd_fused_kernel); 2: head_fwd_kernel, a launch of its own.  One two-stage
      step, then an eval-mode forward pass: predictions, features, scalars, parameter buckets."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mimrl_amd import _lib                               # noqa: E402
from mimrl_amd.engine import HipEngine                   # noqa: E402
from tests import class_loss_ref as CL                   # noqa: E402
from tests.helpers import load_golden, oracle_params     # noqa: E402

NAME = "tiny_cls7_ce"


def engine(precision):
    c, opt, batch, banks = CL.cls_case(NAME)
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision=precision, use_graph=True)
    assert eng.task_loss == _lib.CLASS_LOSSES["CE"] and eng.pred.shape == (c["B"], 7)
    eng.load_params(oracle_params(opt, c["seed"]))
    eng.set_batch(*batch)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    eng.set_stage2_prefetch(1)
    return eng


def steps(eng, n):
    anchors = load_golden(NAME)["anchors"]
    sc = []
    for it in range(n):
        eng.set_anchors(1, anchors[it, 0], exact_ties=True)
        eng.set_anchors(2, anchors[it, 1], exact_ties=True)
        eng.step()
        torch.cuda.synchronize()
        sc.append(eng.read_scalars().copy())
    return np.stack(sc)


def main():
    assert _lib.DETERMINISTIC and _lib.load().mimrl_deterministic() == 1, "not the deterministic build"
    res = {}
    if sys.argv[2] == "det":
        for run in "ab":
            eng = engine("fp32")
            res[run + "_scalars"] = steps(eng, 3)
            res[run + "_main"], res[run + "_crit"] = eng.main["p"].cpu().numpy().copy(), eng.crit["p"].cpu().numpy().copy()
            eng.close()
    else:
        eng = engine("bf16")
        res["step_scalars"] = steps(eng, 1)
        res["step_pred"], res["step_feats"] = eng.pred.cpu().numpy().copy(), eng.feats.cpu().numpy().copy()
        res["main"], res["crit"] = eng.main["p"].cpu().numpy().copy(), eng.crit["p"].cpu().numpy().copy()
        eng.forward(train=False)
        torch.cuda.synchronize()
        res["eval_pred"], res["eval_feats"] = eng.pred.cpu().numpy().copy(), eng.feats.cpu().numpy().copy()
        eng.close()
    assert _lib.load().mimrl_deterministic() == 1, "an accumulation left the order-independent path"
    np.savez(sys.argv[1], **res)
    print("ok", len(res))


if __name__ == "__main__":
    main()
