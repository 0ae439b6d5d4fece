"""Shared by the score tests (tests/test_scores_host.py, tests/test_gpu_scores.py) and the fixture generator
(tests/golden/make_golden_scores.py): the committed input pairs, a score block built in NumPy by the documented slot layout
(include/mimrl.h: MIMRL_SC_*; Chan's merge, batch by batch, as the kernel does it), and the comparison of two score dicts."""
import numpy as np

from mimrl_amd import Utils, _lib as L

# predictions and labels (fp32) at the half-to-even cases, on and beyond the clips, and at both zeros
EDGE = np.array([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0, -2.0, 3.0, -3.0, 3.7, -3.7, 0.0, -0.0, 0.49999997, 1.2], np.float32)
BAND = 1e-10          # mae / corr of a double accumulation of <= 4099 rows: more than 100 n 2^-53
COUNT_KEYS = Utils.REGRESSION_SCORE_KEYS[2:]


def crafted_pair():
    """64 rows: every EDGE value as a label against four predictions -- itself, its neighbour in EDGE, its negative, and itself moved by
    0.3 -- so that the labels 0.0 and -0.0 meet predictions 0.0, -0.0 and both signs."""
    y = np.repeat(EDGE, 4)
    p = np.stack([EDGE, np.roll(EDGE, 1), -EDGE, EDGE + np.float32(0.3)], 1).reshape(-1)
    return p.astype(np.float32), y.astype(np.float32)


def random_pair(n=64, seed=7):
    """Labels on the MOSI grid (multiples of 0.2 in [-3, 3]), predictions = 0.6 label + noise (std >= 0.5 each side, |corr| <= 0.9)."""
    g = np.random.Generator(np.random.PCG64(seed))
    y = (g.integers(-15, 16, size=n) / 5.0).astype(np.float32)
    p = (0.6 * y + 0.9 * g.standard_normal(n)).astype(np.float32)
    return p, y


def tiled_pair(n, seed):
    """n rows for the operator tests: the crafted rows, tiled, in the first half (as many as fit), random rows behind; shuffled."""
    cp, cy = crafted_pair()
    k = n // 2
    rp, ry = random_pair(n - k, seed)
    p, y = np.concatenate([np.resize(cp, k), rp]), np.concatenate([np.resize(cy, k), ry])
    perm = np.random.Generator(np.random.PCG64(seed + 1)).permutation(n)
    return p[perm].astype(np.float32), y[perm].astype(np.float32)


def regression_counts(p, y):
    """The int64 slots of a regression block for fp32 arrays p, y, in NumPy: {slot: value}."""
    p, y = np.asarray(p, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
    out = {L.SC_N: len(p)}
    with np.errstate(invalid="ignore"):
        out[L.SC_ACC7] = int(np.sum(np.round(np.clip(p, -3, 3)) == np.round(np.clip(y, -3, 3))))
        out[L.SC_ACC5] = int(np.sum(np.round(np.clip(p, -2, 2)) == np.round(np.clip(y, -2, 2))))
        bad = np.isnan(p)
        for slot, truth, pred, rows in ((L.SC_PN, y > 0, p > 0, y != 0), (L.SC_NN, y >= 0, p >= 0, np.ones(len(y), bool))):
            pred = np.where(bad, ~truth, pred)                       # a NaN prediction is the class the truth is not
            for k in range(4):
                out[slot + k] = int(np.sum(rows & (2 * truth.astype(int) + pred.astype(int) == k)))
    return out


def numpy_block(batches):
    """A regression score block after the calls `batches` = [(p, y), ...]: per batch the mean first, then the centred sums, merged into
    the running moments with Chan's pairwise formula -- float64 throughout, the documented slot layout."""
    blk = np.zeros(L.SCORE_SLOTS, np.float64)
    d, i = blk, blk.view(np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        for p, y in batches:
            p, y = np.asarray(p, np.float32).astype(np.float64), np.asarray(y, np.float32).astype(np.float64)
            b = len(p)
            mp, my = p.sum() / b, y.sum() / b
            qp, qy, qc, sa = ((p - mp) ** 2).sum(), ((y - my) ** 2).sum(), ((p - mp) * (y - my)).sum(), np.abs(p - y).sum()
            a = int(i[L.SC_N])
            if a == 0:
                d[L.SC_MEAN_P], d[L.SC_MEAN_Y], d[L.SC_M2_P], d[L.SC_M2_Y], d[L.SC_C_PY], d[L.SC_SUM_ABS] = mp, my, qp, qy, qc, sa
            else:
                tot, dp, dy = a + b, mp - d[L.SC_MEAN_P], my - d[L.SC_MEAN_Y]
                w = a * b / tot
                d[L.SC_MEAN_P] += dp * (b / tot)
                d[L.SC_MEAN_Y] += dy * (b / tot)
                d[L.SC_M2_P] += qp + dp * dp * w
                d[L.SC_M2_Y] += qy + dy * dy * w
                d[L.SC_C_PY] += qc + dp * dy * w
                d[L.SC_SUM_ABS] += sa
            for slot, v in regression_counts(p, y).items():
                i[slot] += v
    return blk


def class_block(logits, y, C):
    """The int64 slots of a classification block in NumPy: rint of the label, logit > 0 or the first maximal logit."""
    logits, y = np.asarray(logits, np.float32).reshape(len(y), -1), np.asarray(y, np.float32)
    ce = max(C, 2)
    blk = np.zeros(L.SCORE_SLOTS, np.float64)
    i = blk.view(np.int64)
    t = np.rint(y)
    ok = (t >= 0) & (t < ce)
    pred = (logits[:, 0] > 0).astype(np.int64) if C == 1 else logits.argmax(1)
    M = np.zeros((ce, ce), np.int64)
    np.add.at(M, (t[ok].astype(np.int64), pred[ok]), 1)
    i[L.SC_CONF:L.SC_CONF + ce * ce] = M.reshape(-1)
    i[L.SC_N], i[L.SC_IGNORED] = int(ok.sum()), int((~ok).sum())
    return blk


def assert_scores(got, want, band=BAND, what=""):
    """Same keys in the same order; count-derived keys to 1e-12, mae / corr within `band`; NaN where the other side is NaN."""
    assert list(got) == list(want), (what, list(got), list(want))
    for k in want:
        tol = band if k in ("mae", "corr") else 1e-12
        g, w = float(got[k]), float(want[k])
        if np.isnan(w) or np.isinf(w):
            assert (np.isnan(g) and np.isnan(w)) or g == w, (what, k, g, w)
        else:
            assert abs(g - w) <= tol, f"{what} {k}: {g!r} vs {w!r} (|diff| {abs(g - w):.3e} > {tol:g})"
