"""Run under MIMRL_DETERMINISTIC=1 by tests/test_gpu_wide_batch.py (the library is chosen at import, so the deterministic build gets its own
process).  usage: wide_batch_det_worker.py <out.npz>
Two two-stage steps at B = 2048 (separable critic, small T and feature dims, host-provided anchors), one fresh engine per run: graph_a and
graph_b with captured graphs, eager without.  Per run: the scalars of every step and both parameter buckets after the last, into <out.npz>."""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from mimrl_amd import _lib                               # noqa: E402
from tests.test_gpu_wide_batch import _engine, _wide_case   # noqa: E402


def run(use_graph):
    c, opt, batch, banks, anchors = _wide_case()
    eng, _ = _engine(c, opt, batch, banks, use_graph=use_graph)
    sc = []
    for _ in range(2):
        eng.set_anchors(1, anchors[0])
        eng.set_anchors(2, anchors[1])
        eng.step()
        torch.cuda.synchronize()
        sc.append(eng.read_scalars().copy())
    out = {"scalars": np.stack(sc), "main": eng.main["p"].cpu().numpy().copy(), "crit": eng.crit["p"].cpu().numpy().copy()}
    eng.close()
    return out


def main():
    assert _lib.DETERMINISTIC and _lib.load().mimrl_deterministic() == 1, "not the deterministic build"
    res = {}
    for name, graph in (("graph_a", True), ("graph_b", True), ("eager", False)):
        for k, v in run(graph).items():
            res[f"{name}_{k}"] = v
    assert _lib.load().mimrl_deterministic() == 1, "an accumulation left the order-independent path"
    np.savez(sys.argv[1], **res)
    print("ok", len(res))


if __name__ == "__main__":
    main()
