"""CPU: the regression score table (mae, corr, Acc-7, Acc-5, the two Acc-2 and the two F1 of Utils.py:118-175) on the host -- against the
reference's own calc_metrics (tests/golden/scores_ref.npz), against scikit-learn, and through a score block built in NumPy by the slot
layout the device kernel fills (include/mimrl.h: MIMRL_SC_*, mimrl_op_score_accum)."""
import os
import re
import types

import numpy as np
import pytest

from mimrl_amd import Utils, _lib
from mimrl_amd.Solver import Solver
from tests import scores_ref as SR
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["mae", "corr", "7-class_acc", "5-class_acc", "2(pos/neg)-class_acc", "2(nneg/neg)-class_acc", "2(pos/neg)-class_f1",
        "2(nneg/neg)-class_f1"]
SIZES = [1, 63, 64, 65, 255, 257, 2048, 4099]           # the sizes of the device operator test


def solver(task="regression", num_class=1):
    sol = Solver.__new__(Solver)
    sol.opt = types.SimpleNamespace(task=task, num_class=num_class)
    return sol


def score(p, y, **kw):
    return solver(**kw).get_score_from_result(np.asarray(p).reshape(-1, 1), np.asarray(y).reshape(-1, 1))


def test_key_order_and_fixture_inputs():
    assert list(Utils.REGRESSION_SCORE_KEYS) == KEYS
    p, y = SR.random_pair()
    s = score(p, y)
    assert list(s) == KEYS and all(isinstance(v, float) for v in s.values())
    g = load_golden("scores_ref")
    for tag, (p, y) in (("random", SR.random_pair()), ("crafted", SR.crafted_pair())):
        assert np.array_equal(g[tag + "_pred"], p) and np.array_equal(g[tag + "_y"], y) and len(p) == 64 and p.dtype == np.float32
        assert np.array_equal(np.signbit(g[tag + "_pred"]), np.signbit(p)) and np.array_equal(np.signbit(g[tag + "_y"]), np.signbit(y))
    p, y = SR.crafted_pair()
    for v in (0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 2.0, -2.0, 3.0, -3.0, 3.7, -3.7):
        assert (p == v).any() and (y == v).any(), v
    for a in (p, y):                                                       # both zeros, by sign bit
        assert ((a == 0) & ~np.signbit(a)).any() and ((a == 0) & np.signbit(a)).any()
    y = SR.random_pair()[1]
    assert np.abs(y).max() <= 3 and np.allclose(y * 5, np.round(y * 5), atol=1e-5)


@pytest.mark.parametrize("tag", ["random", "crafted"])
def test_host_scores_equal_the_reference(tag):
    g = load_golden("scores_ref")
    s = score(g[tag + "_pred"], g[tag + "_y"])
    assert list(s) == KEYS
    for k, want in zip(KEYS, g[tag + "_scores"]):
        assert abs(s[k] - float(want)) <= 1e-12, (k, s[k], float(want))


@pytest.mark.parametrize("tag", ["random", "crafted"])
def test_host_scores_equal_scikit_learn(tag):
    from sklearn.metrics import accuracy_score, f1_score
    p32, y32 = SR.random_pair(97, 11) if tag == "random" else SR.crafted_pair()
    s = score(p32, y32)
    p, y = p32.astype(np.float64), y32.astype(np.float64)
    nz = y != 0
    want = {"mae": np.abs(p - y).mean(), "corr": np.corrcoef(p, y)[0, 1],
            "7-class_acc": np.mean(np.round(np.clip(p, -3, 3)) == np.round(np.clip(y, -3, 3))),
            "5-class_acc": np.mean(np.round(np.clip(p, -2, 2)) == np.round(np.clip(y, -2, 2))),
            "2(pos/neg)-class_acc": accuracy_score(y[nz] > 0, p[nz] > 0), "2(nneg/neg)-class_acc": accuracy_score(y >= 0, p >= 0),
            "2(pos/neg)-class_f1": f1_score(y[nz] > 0, p[nz] > 0, average="weighted"),
            "2(nneg/neg)-class_f1": f1_score(y >= 0, p >= 0, average="weighted")}
    for k in KEYS:
        assert abs(s[k] - float(want[k])) <= 1e-12, (k, s[k], want[k])


def test_mae_and_corr_keep_their_values():
    """The two keys of before: mae = mean |p - t| and corr = np.corrcoef on float64 copies, corr = 0.0 when either side is constant."""
    p, y = SR.random_pair(50, 3)
    s = score(p, y)
    assert s["mae"] == float(np.abs(p.astype(np.float64) - y.astype(np.float64)).mean())
    assert s["corr"] == float(np.corrcoef(p.astype(np.float64), y.astype(np.float64))[0, 1])
    assert score(np.full(9, 0.37, np.float32), y[:9])["corr"] == 0.0 and score(p[:9], np.full(9, -1.2, np.float32))["corr"] == 0.0
    assert score(p[:1], y[:1])["corr"] == 0.0


def test_weighted_f1_from_confusion_equals_weighted_f1():
    from sklearn.metrics import f1_score
    g = np.random.Generator(np.random.PCG64(5))
    for C in range(1, 9):
        for trial in range(3):
            n = 40 + 7 * trial
            t, p = g.integers(0, C, size=n), g.integers(0, max(C - trial % 2, 1), size=n)     # (odd trials: the last class is never predicted)
            M = np.zeros((C, C), np.int64)
            np.add.at(M, (t, p), 1)
            a, b = Utils.weighted_f1_from_confusion(M), Utils.weighted_f1(t, p)
            assert abs(a - b) <= 1e-15 and abs(a - f1_score(t, p, average="weighted")) <= 1e-12, (C, trial, a, b)
    assert Utils.weighted_f1_from_confusion(np.zeros((2, 2), np.int64)) == 0.0 and Utils.weighted_f1([], []) == 0.0


def test_no_non_zero_label():
    """The reference crashes here (an empty index array); the two pos/neg keys are nan, the rest finite."""
    p = np.array([0.3, -0.2, 0.0, 1.0], np.float32)
    y = np.array([0.0, -0.0, 0.0, 0.0], np.float32)
    s = score(p, y)
    assert list(s) == KEYS
    for k in KEYS:
        assert np.isnan(s[k]) == (k in ("2(pos/neg)-class_acc", "2(pos/neg)-class_f1")), (k, s[k])
    assert s["2(nneg/neg)-class_acc"] == 0.75 and s["corr"] == 0.0
    SR.assert_scores(Utils.score_from_block(SR.numpy_block([(p, y)]), 1, "regression"), s)


def test_nan_and_inf_predictions():
    p, y = SR.random_pair(40, 9)
    clean = score(p, y)
    bad = p.copy()
    bad[5] = np.nan
    s = score(bad, y)
    assert np.isnan(s["mae"]) and np.isnan(s["corr"])
    keep = np.arange(40) != 5
    rest = score(p[keep], y[keep])
    for k in ("7-class_acc", "5-class_acc", "2(nneg/neg)-class_acc"):       # the NaN row is a miss: the other rows' hits over 40 rows
        assert abs(s[k] - rest[k] * 39 / 40) <= 1e-12, k
    assert y[5] != 0 and abs(s["2(pos/neg)-class_acc"] * int((y != 0).sum()) - rest["2(pos/neg)-class_acc"] * int((y[keep] != 0).sum())) <= 1e-9
    SR.assert_scores(Utils.score_from_block(SR.numpy_block([(bad, y)]), 1, "regression"), s)
    inf = p.copy()
    inf[7] = np.inf
    s = score(inf, y)
    assert s["mae"] == np.inf and np.isnan(s["corr"]) and np.isfinite(s["7-class_acc"])
    assert clean["7-class_acc"] - 1 / 40 - 1e-12 <= s["7-class_acc"] <= clean["7-class_acc"] + 1 / 40 + 1e-12
    SR.assert_scores(Utils.score_from_block(SR.numpy_block([(inf, y)]), 1, "regression"), s)


@pytest.mark.parametrize("n", SIZES)
def test_score_from_block_reproduces_the_dict(n):
    """A block built in NumPy by the documented slot layout (one call, and the same rows in three calls merged by Chan's formula) gives the
    dict of get_score_from_result: counts to 1e-12, mae / corr within the band the device test uses -- so a float64 Chan merge stays
    inside it; the inputs are as well conditioned as that test asks (std >= 0.5, |corr| <= 0.9)."""
    p, y = SR.tiled_pair(n, 100 + n)
    want = score(p, y)
    if n >= 63:
        assert p.std() >= 0.5 and y.std() >= 0.5 and abs(want["corr"]) <= 0.9
    blk = SR.numpy_block([(p, y)])
    assert blk.view(np.int64)[_lib.SC_N] == n
    SR.assert_scores(Utils.score_from_block(blk, 1, "regression"), want, what=f"n={n}")
    SR.assert_scores(Utils.score_from_block(blk.view(np.int64), 1, "regression"), want, what=f"n={n} as int64")
    if n >= 3:
        cuts = [0, n // 4, n // 4 + 1, n]
        parts = [(p[a:b], y[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
        SR.assert_scores(Utils.score_from_block(SR.numpy_block(parts), 1, "regression"), want, what=f"n={n} in three calls")


def test_accumulated_block_of_the_device_test_sizes():
    """65 + 1 + 257 rows, the call sequence of the device accumulation test."""
    p, y = SR.tiled_pair(323, 5)
    parts = [(p[:65], y[:65]), (p[65:66], y[65:66]), (p[66:], y[66:])]
    SR.assert_scores(Utils.score_from_block(SR.numpy_block(parts), 1, "regression"), score(p, y))


def test_score_from_block_refuses_other_shapes():
    with pytest.raises(ValueError, match="8-byte slots"):
        Utils.score_from_block(np.zeros(_lib.SCORE_SLOTS, np.float32), 1, "regression")
    with pytest.raises(ValueError, match="8-byte slots"):
        Utils.score_from_block(np.zeros(_lib.SCORE_SLOTS - 1), 1, "regression")
    with pytest.raises(ValueError, match="without rows"):
        Utils.score_from_block(np.zeros(_lib.SCORE_SLOTS), 1, "regression")


@pytest.mark.parametrize("C", [1, 2, 7, 8])
def test_classification_dict_keeps_two_keys(C):
    g = np.random.Generator(np.random.PCG64(40 + C))
    n = 75
    t = g.integers(0, max(C, 2), size=n).astype(np.float32)
    logits = g.standard_normal((n, C)).astype(np.float32)
    s = solver("classification", C).get_score_from_result(logits, t.reshape(-1, 1))
    assert sorted(s) == sorted([f"{C}-class_acc", f"{C}-f1"]) and len(s) == 2
    blk = SR.class_block(logits, t, C)
    got = Utils.score_from_block(blk, C, "classification")
    assert list(got) == list(s)
    for k in s:
        assert abs(got[k] - s[k]) <= 1e-12, (k, got[k], s[k])


def test_library_exports_score_accum():
    lib = _lib.load()
    assert hasattr(lib, "mimrl_op_score_accum") and "mimrl_op_score_accum" in _lib.EXPORTS
    assert len(lib.mimrl_op_score_accum.argtypes) == 6
    header = open(os.path.join(ROOT, "include", "mimrl.h")).read()
    assert re.search(r"\bint mimrl_op_score_accum\s*\(void\* stream, int num_class, const float\* pred, const float\* y, int n, void\* acc\);", header)
    assert set(_lib.EXPORTS) == set(re.findall(r"\b(mimrl_[a-z0-9_]+)\s*\(", header))
    assert lib.mimrl_abi_version() == 6
    slots = dict((n, int(v)) for n, v in re.findall(r"MIMRL_SC_([A-Z0-9_]+) = (\d+)", header))
    mine = {k[3:]: v for k, v in vars(_lib).items() if k.startswith("SC_")}
    assert slots == mine and len(slots) == 13
    assert int(re.search(r"MIMRL_SCORE_SLOTS = (\d+)", header).group(1)) == _lib.SCORE_SLOTS == _lib.SC_CONF + _lib.MAX_CLASSES ** 2


def test_score_accum_refusals_need_no_device():
    """The argument checks come before any device work: -1 and a message naming the argument."""
    import ctypes as C
    lib = _lib.load()
    buf = (C.c_double * _lib.SCORE_SLOTS)()
    a = C.cast(buf, C.c_void_p)
    for args, word in (((9, a, a, 4, a), "num_class"), ((-1, a, a, 4, a), "num_class"), ((0, a, a, 0, a), "rows"),
                       ((0, a, a, (1 << 20) + 1, a), "rows"), ((0, None, a, 4, a), "null"), ((0, a, None, 4, a), "null"),
                       ((0, a, a, 4, None), "null")):
        assert lib.mimrl_op_score_accum(None, *args) == -1, args
        assert word in lib.mimrl_last_error().decode(), (args, lib.mimrl_last_error())
