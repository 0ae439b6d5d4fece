#!/usr/bin/env python3
"""Golden fixtures of the regression task losses (--loss MSE / RMSE / SIMSE / CCC, Solver.py:172-192) by IMPORTING THE REAL REFERENCE
(dev container only).  Uses the stubs and helpers of make_golden.py and writes new files only:

    python tests/golden/make_golden_losses.py      # units_losses.npz, tiny_sep_{mse,rmse,simse,ccc}.npz, epoch_tail_ccc.npz

(a) units_losses.npz: value and autograd gradient of the loss object the reference's Solver.get_task_loss returns, for seeded pred / y
    vectors (B in 2, 7, 128, 1024; one constant pred, where CCC's variance is 0; one zero residual, where RMSE's gradient is NaN).
(b) tiny_sep_<loss>.npz: make_golden.gen() on tiny_sep's config with that task loss in place of nn.L1Loss.
(c) epoch_tail_ccc.npz: make_golden.gen_epoch() on epoch_tail's config through the reference's own Solver with --loss CCC.
"""
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from tests.golden import make_golden as MG  # noqa: E402  (imports the reference with its stubs)

LOSSES = ("MAE", "MSE", "RMSE", "SIMSE", "CCC")
UNIT_CASES = (("b2", 2), ("b7", 7), ("b128", 128), ("b1024", 1024), ("const128", 128), ("zero7", 7))


def reference_solver():
    """The reference's Solver module, with the stubs of make_golden.gen_epoch (tensorboard, local loaders, the BERT tokenizer)."""
    sys.modules.setdefault("torch.utils.tensorboard", types.SimpleNamespace(
        SummaryWriter=lambda *a, **k: types.SimpleNamespace(add_scalar=lambda *a, **k: None, close=lambda: None)))
    sys.modules.setdefault("DataLoaderLocal", types.SimpleNamespace(mosi_r2c_7=None, pom_r2c_7=None, r2c_2=None, r2c_7=None,
                                                                    LocalDataset=None))
    import transformers
    transformers.BertTokenizer.from_pretrained = classmethod(lambda cls, *a, **k: None)
    import Solver as RS  # reference
    return RS


def reference_loss(RS, name):
    """Solver.get_task_loss of the reference for --loss `name` (it reads self.opt.loss only)."""
    return RS.Solver.get_task_loss(types.SimpleNamespace(opt=types.SimpleNamespace(loss=name)))


def unit_vectors(tag, B):
    g = np.random.Generator(np.random.PCG64(1000 + B))
    y = g.uniform(-3, 3, size=B).astype(np.float32)
    if tag.startswith("const"):
        pred = np.full(B, 0.37, np.float32)
    elif tag.startswith("zero"):
        pred = y.copy()
    else:
        pred = (0.6 * y + g.standard_normal(B)).astype(np.float32)
    return pred, y


def gen_units(RS):
    out = {}
    for tag, B in UNIT_CASES:
        pred, y = unit_vectors(tag, B)
        out[f"{tag}_pred"], out[f"{tag}_y"] = pred, y
        for name in LOSSES:
            fn = reference_loss(RS, name)
            p = torch.from_numpy(pred).requires_grad_(True)
            loss = fn(p.reshape(-1), torch.from_numpy(y).reshape(-1))        # Solver.py:334-335
            loss.backward()
            out[f"{tag}_{name}_loss"] = np.float32(loss.item())
            out[f"{tag}_{name}_grad"] = p.grad.numpy().copy()
    path = os.path.join(HERE, "units_losses.npz")
    np.savez_compressed(path, **out)
    print(f"units_losses: wrote {path} ({os.path.getsize(path)/1024:.1f} KiB)")


def gen_steps(RS, base="tiny_sep"):
    """make_golden.gen with the reference's task loss object where it builds nn.L1Loss (Solver.py:181-182 for MAE)."""
    real = torch.nn.L1Loss
    for name in LOSSES[1:]:
        fn = reference_loss(RS, name)
        torch.nn.L1Loss = lambda *a, **k: fn
        try:
            MG.gen(f"{base}_{name.lower()}", MG.CONFIGS[base])
        finally:
            torch.nn.L1Loss = real


def gen_epoch_loss(RS, base="epoch_tail", name="CCC"):
    """make_golden.gen_epoch with --loss `name` on the reference's command line."""
    import Parameters as RP  # reference
    real = RP.parse_args

    def parse_args():
        i = sys.argv.index("--loss")
        sys.argv[i + 1] = name
        return real()

    RP.parse_args = parse_args
    try:
        MG.gen_epoch(f"{base}_{name.lower()}", MG.EPOCH_CONFIGS[base])
    finally:
        RP.parse_args = real


if __name__ == "__main__":
    os.chdir("/tmp")
    RS = reference_solver()
    which = sys.argv[1:] or ["units", "steps", "epoch"]
    if "units" in which:
        gen_units(RS)
    if "steps" in which:
        gen_steps(RS)
    if "epoch" in which:
        gen_epoch_loss(RS)
