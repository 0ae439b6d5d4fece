"""Worker of tests/test_gpu_cube_bookends.py (one process, the deterministic build): per shape and graph mode TWO engines in this process --
the default one, whose fused CubeMLP blocks build their tile from the encoder outputs and end in the head, and one created under
MIMRL_NO_FUSED_TAIL_PRE=2 (tail_pre / head_fwd as launches of their own; the setting is read when a handle is created) -- with the same seed,
synthetic inputs and banks; one two-stage step in the mode bench.py runs, then one forward pass in eval mode.  Writes, per case, which of the
compared arrays are bit-identical and the largest difference of those that are not."""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402
from mimrl_amd import _lib, synth  # noqa: E402
from mimrl_amd.engine import HipEngine  # noqa: E402

B, N = 32, 1284
# name: (T, time_len, blocks [hidden = out], ragged, dropout)
SHAPES = {
    "T5_L8_ragged": (5, 8, [[8, 3, 128], [4, 3, 128]], True, 0.1),           # T < L zero rows, T mod 4 != 0
    "T50_two_blocks": (50, 50, [[50, 3, 128], [10, 3, 128]], False, 0.1),    # the workload's tile shape; head fused at R = 30
    "T50_one_block": (50, 50, [[50, 3, 128]], False, 0.1),                   # last block R = 150 (NMT = 3): head stays a launch, PRE on
    "T50_two_blocks_p0": (50, 50, [[50, 3, 128], [10, 3, 128]], False, 0.0), # the p = 0 path of the dropout scale
}
KNOB = "MIMRL_NO_FUSED_TAIL_PRE"


def run(shape, graph, separate):
    T, L, blocks, ragged, drop = SHAPES[shape]
    opt, _ = bench.workload("cfg1")
    opt.batch_size, opt.time_len = B, L
    opt.d_hiddens, opt.d_outs = [list(b) for b in blocks], [list(b) for b in blocks]
    opt.res_project = [True] * len(blocks)
    opt.dropout = [drop] * 4
    if separate:
        os.environ[KNOB] = "2"
    else:
        os.environ.pop(KNOB, None)
    eng = HipEngine(opt, 768, 74, 35, seq_len=T, bank_capacity=N, precision="bf16", use_graph=graph, seed=1, device_anchors=True)
    os.environ.pop(KNOB, None)
    eng.load_params(synth.default_state([(n, tuple(v.shape)) for n, v in eng.params.items()], 0))
    eng.set_batch(*synth.synthetic_batch(B, T, seed=0, ragged=ragged))
    banks = synth.synthetic_banks(N, seed=0)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    eng.set_stage2_prefetch(True)
    out = {}
    eng.step()
    torch.cuda.synchronize()
    s = eng.read_scalars().copy()
    out["step_feats"] = eng.feats.cpu().numpy().copy()
    out["step_pred"] = eng.pred.cpu().numpy().copy()
    out["stage1_scalars"] = s[:32].copy()
    out["stage2_scalars"] = s[32:64].copy()
    out["main_params"] = eng.main["p"].cpu().numpy().copy()
    out["critic_params"] = eng.crit["p"].cpu().numpy().copy()
    eng.forward(train=False)
    torch.cuda.synchronize()
    out["eval_feats"] = eng.feats.cpu().numpy().copy()
    out["eval_pred"] = eng.pred.cpu().numpy().copy()
    eng.close()
    return out


def main():
    assert _lib.DETERMINISTIC, "run with MIMRL_DETERMINISTIC=1: the default build's float atomics are not bit-reproducible from run to run"
    res = {}
    for shape in SHAPES:
        for graph in (False, True):
            a, b = run(shape, graph, False), run(shape, graph, True)
            case = {}
            for k in a:
                fin = bool(np.isfinite(a[k]).all() and np.isfinite(b[k]).all())
                case[k] = {"equal": bool(np.array_equal(a[k], b[k])), "finite": fin, "n": int(a[k].size), "absmax": float(np.abs(a[k]).max()),
                           "maxdiff": float(np.abs(a[k].astype(np.float64) - b[k].astype(np.float64)).max())}
            res[f"{shape}|{int(graph)}"] = case
            print(shape, graph, {k: (v["equal"], v["maxdiff"]) for k, v in case.items()}, flush=True)
    json.dump(res, open(sys.argv[1], "w"), indent=1)
    print("BOOKENDS_DONE")


if __name__ == "__main__":
    main()
