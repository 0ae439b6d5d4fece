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


def weighted_f1_from_confusion(M) -> float:
    """Weighted F1 of an integer confusion matrix M [C, C], rows = truth, columns = prediction: F1 per class, averaged with the class's
    share of the rows as weight (sklearn.metrics.f1_score(average='weighted'); a class neither present nor predicted adds nothing, a class
    nobody predicted scores 0).  0.0 for an empty matrix."""
    import numpy as np
    M = np.asarray(M)
    total, n = 0.0, int(M.sum())
    for c in range(M.shape[0]):
        tp, support = float(M[c, c]), int(M[c, :].sum())
        den = float(support + int(M[:, c].sum()))
        total += support * (2.0 * tp / den if den > 0 else 0.0)
    return float(total / n) if n else 0.0


def weighted_f1(targets, predictions) -> float:
    """``weighted_f1_from_confusion`` of the classes present in targets or predictions.  Solver.py:352."""
    import numpy as np
    t, p = np.asarray(targets).reshape(-1), np.asarray(predictions).reshape(-1)
    classes = np.union1d(t, p)
    M = np.zeros((len(classes), len(classes)), np.int64)
    np.add.at(M, (np.searchsorted(classes, t), np.searchsorted(classes, p)), 1)
    return weighted_f1_from_confusion(M)


# The regression score table of Utils.py:118-175 (calc_metrics), by its keys, in its order.
REGRESSION_SCORE_KEYS = ("mae", "corr", "7-class_acc", "5-class_acc", "2(pos/neg)-class_acc", "2(nneg/neg)-class_acc",
                         "2(pos/neg)-class_f1", "2(nneg/neg)-class_f1")


def _binary_scores(M):
    """(accuracy, weighted F1) of a 2 x 2 confusion (cells 2 * truth + prediction); (nan, nan) without rows."""
    import numpy as np
    M = np.asarray(M, np.int64).reshape(2, 2)
    n = int(M.sum())
    return (float(M[0, 0] + M[1, 1]) / n, weighted_f1_from_confusion(M)) if n else (float("nan"), float("nan"))


def _regression_table(mae, corr, n, hits7, hits5, pn, nn):
    a_pn, f_pn = _binary_scores(pn)
    a_nn, f_nn = _binary_scores(nn)
    return dict(zip(REGRESSION_SCORE_KEYS, (mae, corr, float(hits7) / n, float(hits5) / n, a_pn, a_nn, f_pn, f_nn)))


def regression_scores(predictions, targets) -> dict:
    """calc_metrics (Utils.py:118-175) on float64 copies of the values: MAE, Pearson correlation (0.0 when either side is constant),
    Acc-7 / Acc-5 (round half to even of the values clipped to +-3 / +-2), and accuracy and weighted F1 of the two sign splits --
    pos/neg over the rows with a non-zero label (truth y > 0, prediction p > 0; nan without such a row, where the reference crashes),
    nneg/neg over all rows (y >= 0, p >= 0).  A NaN prediction misses every accuracy and makes mae and corr NaN."""
    import numpy as np
    p, t = np.asarray(predictions).reshape(-1).astype(np.float64), np.asarray(targets).reshape(-1).astype(np.float64)
    with np.errstate(invalid="ignore"):
        mae = float(np.abs(p - t).mean())
        sp, st = p.std(), t.std()
        corr = 0.0 if sp == 0 or st == 0 else float(np.corrcoef(p, t)[0, 1])
        hits = [int(np.sum(np.round(np.clip(p, -c, c)) == np.round(np.clip(t, -c, c)))) for c in (3.0, 2.0)]
    bad = np.isnan(p)
    confs = []
    for truth, pred, rows in ((t > 0, p > 0, t != 0), (t >= 0, p >= 0, np.ones(len(t), bool))):
        pred = np.where(bad, ~truth, pred)
        confs.append(np.bincount((2 * truth + pred)[rows].astype(np.int64), minlength=4))
    return _regression_table(mae, corr, len(t), hits[0], hits[1], confs[0], confs[1])


def score_from_block(block, num_class, task) -> dict:
    """The score dict of ``Solver.get_score_from_result`` from a score block read back to the host (include/mimrl.h: MIMRL_SC_*, mirrored
    as ``_lib.SC_*``; 8-byte slots, doubles below SC_N and int64 from there on).  Regression: mae = sum |p - y| / n, corr =
    C_py / sqrt(M2_p M2_y) (0.0 when either M2 is 0), accuracies from the counters, F1 from the two 2 x 2 confusions.  Classification:
    accuracy and weighted F1 of the [Ceff, Ceff] confusion over the counted rows (a row with a label outside [0, Ceff) is in SC_IGNORED only)."""
    import numpy as np
    from . import _lib as L
    raw = np.ascontiguousarray(np.asarray(block).reshape(-1))
    if raw.dtype.itemsize != 8 or raw.size != L.SCORE_SLOTS:
        raise ValueError(f"a score block is {L.SCORE_SLOTS} 8-byte slots, got {raw.size} of {raw.dtype}")
    d, i = raw.view(np.float64), raw.view(np.int64)
    n = int(i[L.SC_N])
    if task == "classification":
        C = int(num_class)
        ce = max(C, 2)
        M = i[L.SC_CONF:L.SC_CONF + ce * ce].reshape(ce, ce)
        return {f"{C}-class_acc": float(np.trace(M)) / n if n else float("nan"), f"{C}-f1": weighted_f1_from_confusion(M)}
    if n <= 0:
        raise ValueError("score block without rows")
    with np.errstate(invalid="ignore"):
        m2p, m2y = d[L.SC_M2_P], d[L.SC_M2_Y]
        corr = 0.0 if m2p == 0 or m2y == 0 else float(np.clip(d[L.SC_C_PY] / np.sqrt(m2p) / np.sqrt(m2y), -1.0, 1.0))
    return _regression_table(float(d[L.SC_SUM_ABS]) / n, corr, n, int(i[L.SC_ACC7]), int(i[L.SC_ACC5]),
                             i[L.SC_PN:L.SC_PN + 4], i[L.SC_NN:L.SC_NN + 4])
