"""The classification task losses of --task classification (CE, Focal, BCE; Solver.py:172-178 applied with the reshapes of :324-333) restated
in torch for the oracle side of the tests: pinned to the reference's own loss objects by tests/golden/units_cls.npz
(test_class_loss_host.py).  ``patch_oracle`` puts one in the place of the oracle's MAE; ``cls_case`` is tests.helpers.case for the
classification step fixtures of tests/golden/make_golden_cls.py (class-index labels in the batch and in the label bank)."""
import numpy as np
import torch
import torch.nn.functional as F

from mimrl_amd import synth
from tests.golden.configs import CONFIGS, make_opt

KINDS = {"CE": 5, "Focal": 6, "BCE": 7}

# step fixtures: name -> (configuration whose shape it takes, num_class, --loss)
CLS_CONFIGS = {
    "tiny_cls2_ce": ("tiny_sep", 2, "CE"),
    "tiny_cls7_ce": ("tiny_sep", 7, "CE"),
    "tiny_cls7_focal": ("tiny_sep", 7, "Focal"),
    "tiny_cls2_bce": ("tiny_sep", 2, "BCE"),
    "tiny_cls1_bce": ("tiny_sep", 1, "BCE"),
}

# unit cases of units_cls.npz: tag -> (B, C, kind of logits)
UNIT_CASES = {
    "b2c2": (2, 2, "normal"), "b7c7": (7, 7, "normal"), "b128c2": (128, 2, "normal"), "b128c7": (128, 7, "normal"),
    "b1024c7": (1024, 7, "normal"), "b7c1": (7, 1, "normal"), "b128c1": (128, 1, "normal"),
    "eq128c7": (128, 7, "equal"), "eq128c2": (128, 2, "equal"),
    "big128c7": (128, 7, "big"), "big128c2": (128, 2, "big"), "big128c1": (128, 1, "big"),
    "sure128c7": (128, 7, "sure"),
}


# Where the band of the op tests (rtol 1e-5, gradient atol 1e-5 x the largest gradient entry) is narrower than the reference's OWN fp32
# rounding: measured spread max |fixture - float64 restatement of the same formula| over the gradient.  sure128c7 / CE: the softmax of a
# true class ahead by 20 is 1 - 3e-11, which fp32 rounds to 1 -- the reference's gradient there is exactly 0, float64 gives -3e-11 to
# -8.83e-11 (the largest gradient entry of the case is 1.6e-11).  Every other case and loss lies inside 0.2 of the band.  The tests add
# 4 x the spread (fp32 reduction order) to the gradient atol.
GRAD_SPREAD = {("sure128c7", "CE"): 8.83e-11}


def grad_atol(tag, name, want_g):
    return 1e-5 * float(np.abs(want_g).max()) + 1e-12 + 4.0 * GRAD_SPREAD.get((tag, name), 0.0)


def losses_for(C):
    """The losses the reference accepts at C classes (Solver.py:324-337)."""
    return (("CE", "Focal") if C >= 2 else ()) + (("BCE",) if C <= 2 else ())


def unit_vectors(tag):
    """Seeded logits [B, C] and class indices [B] (float32) of a unit case: 'equal' every logit the same, 'big' logits scaled to +-80,
    'sure' the true class ahead of every other logit by 20 (Focal's (1 - p) is then ~0)."""
    B, C, kind = UNIT_CASES[tag]
    g = np.random.Generator(np.random.PCG64(2000 + 17 * B + C))
    y = g.integers(0, max(C, 2), size=B).astype(np.float32)
    x = g.standard_normal((B, C)).astype(np.float32)
    if kind == "equal":
        x = np.full((B, C), 0.25, np.float32)
    elif kind == "big":
        x = (x / np.abs(x).max() * 80.0).astype(np.float32)
    elif kind == "sure":
        x = np.clip(x, -1.0, 1.0)
        x[np.arange(B), y.astype(np.int64)] = x.max(1) + 20.0
    return x, y


def apply(fn, logits, y, name, C):
    """``fn`` (logits, target) on the operands Solver.py:324-333 builds for --loss ``name`` at ``C`` classes."""
    if name in ("CE", "Focal"):
        return fn(logits.reshape(-1, C), y.reshape(-1).long())
    if C == 2:
        return fn(logits.reshape(-1, C), F.one_hot(y.reshape(-1).long(), num_classes=C).to(logits.dtype))
    return fn(logits.reshape(-1), y.reshape(-1).to(logits.dtype))


def ce(x, t):
    return (torch.logsumexp(x, 1) - x.gather(1, t.reshape(-1, 1)).reshape(-1)).mean()


def focal(x, t):
    """Utils.py:638-649: the focal factor on the batch-mean cross entropy."""
    c = ce(x, t)
    return (1 - torch.exp(-c)) ** 2 * c


def bce(x, t):
    return (torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))).mean()


LOSSES = {"CE": ce, "Focal": focal, "BCE": bce}


def value_and_grad(name, logits, y, dtype=torch.float32, fn=None):
    x = torch.as_tensor(logits).to(dtype).clone().requires_grad_(True)
    C = x.shape[1]
    loss = apply(fn or LOSSES[name], x, torch.as_tensor(y), name, C)
    loss.backward()
    return loss.item(), x.grad.numpy().copy()


def task_loss(name, C):
    """The oracle's signature (pred [B, C], labels of any shape) -> scalar."""
    return lambda pred, labels: apply(LOSSES[name], pred, labels, name, C)


def patch_oracle(monkeypatch, name, C):
    import oracle.mimrl_ref
    monkeypatch.setattr(oracle.mimrl_ref, "task_loss_mae", task_loss(name, C))


def cls_opt(base, C, loss):
    opt = make_opt(CONFIGS[base])
    opt.num_class, opt.task, opt.loss = C, "classification", loss
    return opt


def cls_case(name, dtype=torch.float32):
    """tests.helpers.case for a classification step fixture: the base configuration's inputs with class-index labels."""
    base, C, loss = CLS_CONFIGS[name]
    c = CONFIGS[base]
    t, a, v, y = synth.synthetic_batch(c["B"], c["T"], seed=c["seed"], ragged=c.get("ragged", False))
    banks = dict(synth.synthetic_banks(c["N"], seed=c["seed"]))
    y, banks["C"] = synth.class_labels(y, C), synth.class_labels(banks["C"], C)
    batch = tuple(torch.from_numpy(x).to(dtype) for x in (t, a, v, y))
    return c, cls_opt(base, C, loss), batch, {k: torch.from_numpy(val).to(dtype) for k, val in banks.items()}
