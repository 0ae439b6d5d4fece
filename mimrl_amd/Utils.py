"""Flag parsers and tiny helpers of the hot path (reference: Utils.py:226-248, 297-298, 307-311)."""
import argparse
import logging
import os

import torch


def str2bool(v: str) -> bool:
    t = v.strip().lower()
    if t in {"yes", "true", "t", "y", "1"}:
        return True
    if t in {"no", "false", "f", "n", "0"}:
        return False
    raise argparse.ArgumentTypeError("Boolean value expected." + v)


def str2bools(v: str):
    """'1-0-1' -> [True, False, True]"""
    return [str2bool(x) for x in v.split("-")]


def str2floats(v: str):
    """'0.1-0.2' -> [0.1, 0.2]"""
    return [float(x) for x in v.split("-")]


def str2listoffints(v: str):
    """'50-3-128=10-3-128' -> [[50,3,128],[10,3,128]]"""
    return [[int(x) for x in blk.split("-")] for blk in v.split("=")]


def get_mask_from_sequence(sequence: torch.Tensor, dim: int) -> torch.Tensor:
    """True where a row is all-zero (padding); Utils.py:297-298."""
    return sequence.abs().sum(dim=dim) == 0


def to_gpu(x, on_cpu: bool = False, gpu_id=None):
    """Utils.py:307-311."""
    if torch.cuda.is_available() and not on_cpu:
        x = x.cuda(gpu_id)
    return x


def set_logger(log_path: str):
    logger = logging.getLogger()
    logger.setLevel(logging.DEBUG)
    if not logger.handlers:
        os.makedirs(os.path.dirname(log_path) or ".", exist_ok=True)
        fh = logging.FileHandler(log_path)
        fh.setFormatter(logging.Formatter("%(asctime)s:%(levelname)s: %(message)s"))
        sh = logging.StreamHandler()
        sh.setFormatter(logging.Formatter("%(message)s"))
        logger.addHandler(fh)
        logger.addHandler(sh)


def log_message(message: str):
    logging.log(msg=message, level=logging.DEBUG)


# --loss (Solver.py:172-192): the regression task losses, fp32 torch on the host (Solver.compute_loss); the device computes the same
# (csrc/task_loss.h).  pred and y are flattened to [B] first (Solver.py:334-335).
def rmse_loss(pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return ((pred - y) ** 2).mean() ** 0.5


def simse_loss(pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    n = y.numel()
    return (y - pred).sum().pow(2) / (n * n)


def ccc_loss(pred: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    mp, my = pred.mean(), y.mean()
    cov = ((pred - mp) * (y - my)).mean()
    vy, vp = ((y - my) ** 2).mean(), ((pred - mp) ** 2).mean()
    return 1.0 - 2.0 * cov / (vy + vp + (my - mp) ** 2 + 1e-10)


# --task classification (Solver.py:172-178): logits [B, C] with int64 class indices [B] (CE, Focal), or logits and float targets of one
# shape (BCE; Solver.compute_loss builds them as Solver.py:327-333 does).
def ce_loss(logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.cross_entropy(logits, y)


def focal_loss(logits: torch.Tensor, y: torch.Tensor) -> torch.Tensor:
    """Utils.py:638-649 (gamma 2): the focal factor sits on the batch-MEAN cross entropy, not on each row's."""
    ce = torch.nn.functional.cross_entropy(logits, y)
    return (1 - torch.exp(-ce)) ** 2 * ce


def bce_loss(logits: torch.Tensor, t: torch.Tensor) -> torch.Tensor:
    return torch.nn.functional.binary_cross_entropy_with_logits(logits, t)


TASK_LOSS_FUNCTIONS = {
    "MAE": lambda p, y: (p - y).abs().mean(),
    "MSE": lambda p, y: ((p - y) ** 2).mean(),
    "RMSE": rmse_loss,
    "SIMSE": simse_loss,
    "CCC": ccc_loss,
    "CE": ce_loss,
    "Focal": focal_loss,
    "BCE": bce_loss,
}


def weighted_f1(targets, predictions) -> float:
    """F1 per class present in targets or predictions, averaged with the class's share of the targets as weight (what
    sklearn.metrics.f1_score(average='weighted') computes; a class nobody predicted scores 0).  Solver.py:352."""
    import numpy as np
    t, p = np.asarray(targets).reshape(-1), np.asarray(predictions).reshape(-1)
    total = 0.0
    for c in np.union1d(t, p):
        tp = float(np.sum((t == c) & (p == c)))
        den = float(np.sum(t == c) + np.sum(p == c))
        total += np.sum(t == c) * (2.0 * tp / den if den > 0 else 0.0)
    return float(total / len(t)) if len(t) else 0.0
