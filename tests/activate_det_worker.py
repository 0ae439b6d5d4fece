"""Worker of tests/test_gpu_activate.py (one process, the deterministic build: the library is chosen at import).  usage: <out.json>
  det      : one --activate elu probe_cube case (tiny_odd, bf16 fused kernels, the zones point) on two fresh engines: is every returned tensor
             bit-identical run to run?  (and a gelu run: other numbers, so the activation code reached the kernels)
  bookends : tests/cube_bookends_worker.py's folded-vs-separate-launches comparison, its own code, with --activate elu instead of gelu."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from mimrl_amd import _lib  # noqa: E402
from mimrl_amd.engine import HipEngine  # noqa: E402
from tests import cube_bookends_worker as W  # noqa: E402
from tests.golden.configs import CONFIGS, make_opt  # noqa: E402
from tests.test_gpu_activate import probe_inputs, zones_params  # noqa: E402
from tests.test_gpu_fused_oracle import perturbed_params  # noqa: E402

SHAPES = ["T5_L8_ragged", "T50_two_blocks"]


def probe(act):
    c = CONFIGS["tiny_odd"]
    opt = make_opt(c)
    opt.activate = act
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision="bf16")
    eng.load_params(zones_params(perturbed_params(opt, c["seed"])))
    out, dx = eng.probe_cube(*probe_inputs(c["B"], opt.time_len, opt.d_outs[-1][0], opt.d_outs[-1][1]))
    torch.cuda.synchronize()
    res = {"out": out.cpu().numpy().copy(), "dx": dx.cpu().numpy().copy(),
           **{n: v.cpu().numpy().copy() for n, v in eng.grads.items() if n.startswith("mlp_encoder.")}}
    eng.close()
    return res


def main():
    assert _lib.DETERMINISTIC and _lib.load().mimrl_deterministic() == 1, "not the deterministic build"
    a, b, gelu = probe("elu"), probe("elu"), probe("gelu")
    unequal = [n for n in a if not np.array_equal(a[n], b[n])]
    det = {"deterministic": int(_lib.load().mimrl_deterministic()), "tensors": len(a), "equal": not unequal, "unequal": unequal[:8],
           "finite": bool(all(np.isfinite(v).all() for v in a.values())),
           "grad_absmax": float(max(np.abs(v).max() for n, v in a.items() if n not in ("out", "dx"))),
           "differs_from_gelu": bool(not np.array_equal(a["out"], gelu["out"]) and not np.array_equal(a["dx"], gelu["dx"]))}
    print("det", det, flush=True)

    workload = W.bench.workload

    def elu_workload(name):
        opt, n = workload(name)
        opt.activate = "elu"
        return opt, n
    W.bench.workload = elu_workload
    bookends = {}
    for shape in SHAPES:
        for graph in (False, True):
            x, y = W.run(shape, graph, False), W.run(shape, graph, True)
            bookends[f"{shape}|{int(graph)}"] = {
                k: {"equal": bool(np.array_equal(x[k], y[k])), "finite": bool(np.isfinite(x[k]).all() and np.isfinite(y[k]).all()), "n": int(x[k].size),
                    "absmax": float(np.abs(x[k]).max()), "maxdiff": float(np.abs(x[k].astype(np.float64) - y[k].astype(np.float64)).max())} for k in x}
            print(shape, graph, {k: v["equal"] for k, v in bookends[f"{shape}|{int(graph)}"].items()}, flush=True)
    W.bench.workload = workload
    json.dump({"det": det, "bookends": bookends}, open(sys.argv[1], "w"), indent=1)
    print("ACTIVATE_DONE")


if __name__ == "__main__":
    main()
