#!/usr/bin/env python3
"""Golden fixtures of --task classification (--loss CE / Focal / BCE, --num_class 1 | 2 | 7; Parameters.py:22-23,55, Solver.py:172-178,
324-333) by IMPORTING THE REAL REFERENCE (dev container only).  Uses the stubs and helpers of make_golden.py / make_golden_losses.py and
writes new files only:

    python tests/golden/make_golden_cls.py      # units_cls.npz, tiny_cls{2_ce,7_ce,7_focal,2_bce,1_bce}.npz, epoch_tail_cls2.npz

(a) units_cls.npz: value and autograd gradient of the loss object the reference's Solver.get_task_loss returns, applied with the reshape /
    one-hot logic of Solver.py:324-333, for the seeded logits / labels of tests.class_loss_ref.unit_vectors.
(b) tiny_cls*.npz: make_golden.gen() on tiny_sep's shape with num_class set, the reference's loss object where it builds nn.L1Loss, and
    class-index labels (mimrl_amd.synth.class_labels) in the batch and in the label bank.
(c) epoch_tail_cls2.npz: make_golden.gen_epoch() on epoch_tail's sizes through the reference's own Solver with
    --task classification --num_class 2 --loss CE; the scores of Solver.get_score_from_result are recorded as ep<e>_<split>_acc / _f1.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import torch  # noqa: E402

from tests.golden import make_golden_losses as ML  # noqa: E402  (first: it imports make_golden, which puts the reference in front of sys.path)
from tests.golden import make_golden as MG  # noqa: E402  (imports the reference with its stubs)
from mimrl_amd import synth  # noqa: E402
from tests import class_loss_ref as CL  # noqa: E402


def gen_units(RS):
    out = {}
    for tag, (B, C, _) in CL.UNIT_CASES.items():
        x, y = CL.unit_vectors(tag)
        out[f"{tag}_logits"], out[f"{tag}_y"] = x, y
        for name in CL.losses_for(C):
            v, g = CL.value_and_grad(name, x, y, fn=ML.reference_loss(RS, name))
            out[f"{tag}_{name}_loss"], out[f"{tag}_{name}_grad"] = np.float32(v), g
    path = os.path.join(HERE, "units_cls.npz")
    np.savez_compressed(path, **out)
    print(f"units_cls: wrote {path} ({os.path.getsize(path)/1024:.1f} KiB)")


def gen_steps(RS):
    real_l1, real_opt, real_q = torch.nn.L1Loss, MG.make_opt, MG.quantize_labels
    for name, (base, C, loss) in CL.CLS_CONFIGS.items():
        fn = ML.reference_loss(RS, loss)
        torch.nn.L1Loss = lambda *a, _fn=fn, _C=C, _loss=loss, **k: (lambda p, y: CL.apply(_fn, p, y, _loss, _C))

        def make_opt(c, _C=C, _loss=loss):
            opt = real_opt(c)
            opt.num_class, opt.task, opt.loss = _C, "classification", _loss
            return opt

        def class_labels(c, batch, banks, _C=C):
            t, a, v, y = batch
            banks = dict(banks)
            banks["C"] = synth.class_labels(banks["C"], _C)
            return (t, a, v, synth.class_labels(y, _C)), banks

        MG.make_opt, MG.quantize_labels = make_opt, class_labels
        try:
            MG.gen(name, MG.CONFIGS[base])
        finally:
            torch.nn.L1Loss, MG.make_opt, MG.quantize_labels = real_l1, real_opt, real_q


def gen_epoch_cls(RS, base="epoch_tail", name="epoch_tail_cls2", C=2, loss="CE"):
    """make_golden.gen_epoch with the classification flags on the reference's command line and class-index labels in the loaders.  The
    labels stay float32 -- the reference's kNN product sampler (Model.py:97) cannot take an int64 label bank -- so one more stub: the
    CE object of Solver.get_task_loss gets its targets cast to int64, which is what nn.CrossEntropyLoss needs of them."""
    import Parameters as RP  # reference
    real_parse, real_data, real_score, real_loss = RP.parse_args, MG.epoch_data, RS.Solver.get_score_from_result, RS.Solver.get_task_loss
    scores = []

    def parse_args():
        sys.argv[sys.argv.index("--loss") + 1] = loss
        sys.argv += ["--task", "classification", "--num_class", str(C)]
        return real_parse()

    def epoch_data(c):
        return {k: (t, a, v, synth.class_labels(y, C)) for k, (t, a, v, y) in real_data(c).items()}

    def get_score(self, predictions, targets):
        s = real_score(self, predictions, targets)
        scores.append(s)
        return dict(s, mae=np.nan, corr=np.nan)          # (gen_epoch reads the regression keys)

    def get_task_loss(self):
        fn = real_loss(self)
        return lambda p, t: fn(p, t.long())

    RP.parse_args, MG.epoch_data, RS.Solver.get_score_from_result, RS.Solver.get_task_loss = parse_args, epoch_data, get_score, get_task_loss
    try:
        MG.gen_epoch(name, MG.EPOCH_CONFIGS[base])
    finally:
        RP.parse_args, MG.epoch_data, RS.Solver.get_score_from_result, RS.Solver.get_task_loss = real_parse, real_data, real_score, real_loss
    path = os.path.join(HERE, f"{name}.npz")
    out = dict(np.load(path))
    for k in [k for k in out if k.endswith(("_mae", "_corr"))]:
        del out[k]
    assert len(scores) == 3 * MG.EPOCH_CONFIGS[base]["epochs"]
    for i, s in enumerate(scores):                        # call order: train, valid, test of every epoch
        tag = f"ep{i // 3}_{('train', 'valid', 'test')[i % 3]}"
        out[tag + "_acc"], out[tag + "_f1"] = np.float64(s[f"{C}-class_acc"]), np.float64(s[f"{C}-f1"])
    np.savez_compressed(path, **out)
    print(f"{name}: scores " + " ".join(f"{k}={float(out[k]):.4f}" for k in sorted(out) if k.endswith(("_acc", "_f1"))))


if __name__ == "__main__":
    os.chdir("/tmp")
    RS = ML.reference_solver()
    which = sys.argv[1:] or ["units", "steps", "epoch"]
    if "units" in which:
        gen_units(RS)
    if "steps" in which:
        gen_steps(RS)
    if "epoch" in which:
        gen_epoch_cls(RS)
