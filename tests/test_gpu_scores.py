"""-m gpu: mimrl_op_score_accum (csrc/score_ops.hip) -- one workgroup folds a batch of predictions into a block of running score
statistics -- against NumPy float64 on the same fp32 arrays, and the paths that use it: HipEngine.score_accum, Solver.train / evaluate,
Solver.step with track_score, and the epoch log of the CLI."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mimrl_amd import Utils, _lib
from mimrl_amd.Solver import Solver
from tests import scores_ref as SR
from tests.epoch_helpers import epoch_case
from tests.helpers import oracle_params
from tests.test_scores_host import KEYS, SIZES, score, solver

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INT = slice(_lib.SC_N, _lib.SCORE_SLOTS)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def new_block():
    return torch.zeros(_lib.SCORE_SLOTS, dtype=torch.float64, device="cuda")


def accum(acc, num_class, pred, y):
    """One call on the current stream; pred / y numpy fp32 -> the device tensors (kept alive by the caller's sync in read())."""
    p, t = torch.from_numpy(np.ascontiguousarray(pred)).cuda(), torch.from_numpy(np.ascontiguousarray(y)).cuda()
    rc = _lib.load().mimrl_op_score_accum(C.c_void_p(torch.cuda.current_stream().cuda_stream), num_class, ptr(p), ptr(t), len(y), ptr(acc))
    assert rc == 0, _lib.load().mimrl_last_error()
    return p, t


def read(acc):
    torch.cuda.synchronize()
    return acc.cpu().numpy()


def assert_counts(blk, want, what=""):
    i = blk.view(np.int64)
    for slot, v in want.items():
        assert int(i[slot]) == int(v), f"{what}: int64 slot {slot} = {int(i[slot])}, NumPy {int(v)}"


def assert_moments(blk, p, y, what):
    """mae and corr of the device block within SR.BAND of the NumPy float64 evaluation (printed first)."""
    got, want = Utils.score_from_block(blk, 1, "regression"), score(p, y)
    print(f"{what}: |mae diff| {abs(got['mae'] - want['mae']):.3e} |corr diff| {abs(got['corr'] - want['corr']):.3e} (band {SR.BAND:g})")
    SR.assert_scores(got, want, what=what)


@pytest.mark.parametrize("n", SIZES)
def test_regression_op_equals_numpy(n):
    p, y = SR.tiled_pair(n, 100 + n)
    acc = new_block()
    keep = accum(acc, 0, p, y)
    blk = read(acc)
    assert_counts(blk, SR.regression_counts(p, y), f"n={n}")
    assert np.all(blk.view(np.int64)[_lib.SC_IGNORED:] == 0)
    assert_moments(blk, p, y, f"n={n}")
    del keep


@pytest.mark.parametrize("bad", [np.nan, np.inf])
def test_nan_and_inf_predictions(bad):
    p, y = SR.tiled_pair(257, 31)
    p[[3, 70, 200]] = bad                           # three waves
    assert (y[[3, 70, 200]] != 0).any()
    acc = new_block()
    keep = accum(acc, 0, p, y)
    blk = read(acc)
    assert_counts(blk, SR.regression_counts(p, y), f"pred {bad}")
    got, want = Utils.score_from_block(blk, 1, "regression"), score(p, y)
    assert np.isnan(want["corr"]) and (np.isnan(want["mae"]) if np.isnan(bad) else want["mae"] == np.inf)
    SR.assert_scores(got, want, what=f"pred {bad}")
    del keep


def test_accumulation_reset_and_reproducibility():
    p, y = SR.tiled_pair(323, 5)
    cuts = [(0, 65), (65, 66), (66, 323)]
    blocks = []
    for rep in range(2):
        acc = new_block()
        keep = [accum(acc, 0, p[a:b], y[a:b]) for a, b in cuts]
        blocks.append(read(acc))
        del keep
    assert blocks[0].tobytes() == blocks[1].tobytes(), "two identical call sequences differ in their bits"
    assert_counts(blocks[0], SR.regression_counts(p, y), "65 + 1 + 257 rows")
    assert_moments(blocks[0], p, y, "65 + 1 + 257 rows")
    acc.zero_()                                      # reset: the next call starts from nothing
    keep = accum(acc, 0, p[:65], y[:65])
    again = read(acc)
    fresh = new_block()
    keep2 = accum(fresh, 0, p[:65], y[:65])
    assert again.tobytes() == read(fresh).tobytes()
    assert_counts(again, SR.regression_counts(p[:65], y[:65]), "after the reset")
    del keep, keep2


def class_case(C, n, seed):
    g = np.random.Generator(np.random.PCG64(seed))
    ce = max(C, 2)
    t = g.integers(0, ce, size=n)
    x = g.standard_normal((n, C)).astype(np.float32)
    y = (t + g.choice([-1e-3, 0.0, 1e-3], size=n)).astype(np.float32)              # labels as floats k +- 1e-3
    if C >= 2:
        for r in range(0, n, 5):                                                    # tied maxima: the first index wins
            a, b = sorted(g.choice(C, size=2, replace=False))
            x[r, a] = x[r, b] = np.float32(x[r].max() + 1.0)
        if n > 2:
            x[2] = 0.25                                                             # every logit equal: class 0
    else:
        x[::7] = 0.0                                                                # logit 0 is not > 0: class 0
    if n >= 65:
        y[[4, 33, 64]] = [ce, -1.0, np.nan]                                         # outside [0, Ceff): ignored
        y[10] = ce - 0.6                                                            # rint(ce - 0.6) = ce - 1: in range
    return x, y


@pytest.mark.parametrize("n", [1, 65, 2048])
@pytest.mark.parametrize("Cn", [1, 2, 7, 8])
def test_classification_op_equals_numpy(Cn, n):
    x, y = class_case(Cn, n, 300 + 10 * Cn + n)
    ce = max(Cn, 2)
    acc = new_block()
    keep = accum(acc, Cn, x, y)
    blk = read(acc)
    want = SR.class_block(x, y, Cn)
    gi, wi = blk.view(np.int64), want.view(np.int64)
    assert np.array_equal(gi[INT], wi[INT]), (gi[INT], wi[INT])
    assert np.all(blk[:_lib.SC_N] == 0), "the double slots are not touched"
    assert gi[_lib.SC_IGNORED] == (3 if n >= 65 else 0) and gi[_lib.SC_N] + gi[_lib.SC_IGNORED] == n
    if Cn >= 2 and n >= 65:
        M = gi[_lib.SC_CONF:_lib.SC_CONF + ce * ce].reshape(ce, ce)
        assert M.sum() == n - 3 and np.triu(M, 1).sum() > 0 and np.tril(M, -1).sum() > 0
    t = np.rint(y)
    ok = (t >= 0) & (t < ce)
    host = solver("classification", Cn).get_score_from_result(x[ok], y[ok].reshape(-1, 1))
    got = Utils.score_from_block(blk, Cn, "classification")
    assert list(got) == list(host)
    for k in host:
        assert abs(got[k] - host[k]) <= 1e-12, (k, got[k], host[k])
    del keep


def test_refusals_leave_the_block_untouched():
    lib = _lib.load()
    acc = torch.full((_lib.SCORE_SLOTS,), -7.25, dtype=torch.float64, device="cuda")
    sentinel = read(acc).tobytes()
    p, y = torch.zeros(8, device="cuda"), torch.zeros(8, device="cuda")
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    cases = [((9, ptr(p), ptr(y), 8, ptr(acc)), "num_class"), ((-1, ptr(p), ptr(y), 8, ptr(acc)), "num_class"),
             ((0, ptr(p), ptr(y), 0, ptr(acc)), "rows"), ((0, ptr(p), ptr(y), (1 << 20) + 1, ptr(acc)), "rows"),
             ((0, None, ptr(y), 8, ptr(acc)), "null"), ((0, ptr(p), None, 8, ptr(acc)), "null"), ((0, ptr(p), ptr(y), 8, None), "null")]
    for args, word in cases:
        assert lib.mimrl_op_score_accum(s, *args) == -1, args
        assert word in lib.mimrl_last_error().decode(), (args, lib.mimrl_last_error())
        assert read(acc).tobytes() == sentinel, args


def as_datas(batch):
    t, a, v, y = batch
    ones = torch.ones(a.shape[0], a.shape[1], dtype=torch.long)
    return (None, a, v, None, None, y.reshape(-1, 1), t, torch.zeros_like(ones), ones, None, None)


@pytest.fixture(scope="module")
def tail_solver():
    """A Solver on epoch_tail (train 36 = 4 x 8 + 4, valid 12 = 8 + 4: a partial last batch, so two handles feed one block)."""
    import copy
    c, opt, sets, _ = epoch_case("epoch_tail")
    o = copy.copy(opt)
    o.task_name, o.seed, o.epochs_num, o.save_best_features = "pytest_scores", 0, 1, False
    o.precision, o.no_graph, o.host_anchors = "fp32", False, True
    loaders = tuple([as_datas(b) for b in sets[k]] for k in ("train", "valid", "test")) + (768, 74, 35)
    sol = Solver(o, loaders)
    sol.model.load_state_dict(oracle_params(opt, c["seed"]))
    yield sol
    sol.engine.close()


def test_solver_train_and_evaluate_score_from_the_block(tail_solver):
    sol = tail_solver
    r = sol.train(0, sol.train_loader, [], [], [], [], [])
    assert list(r[3]) == KEYS and all(np.isfinite(v) for v in r[3].values()), r[3]
    assert list(sol._tails) == [4]
    banks = r[4:]
    for k in ("7-class_acc", "5-class_acc", "2(nneg/neg)-class_acc"):          # both handles fed the block: shares of all 36 rows
        assert abs(r[3][k] * 36 - round(r[3][k] * 36)) < 1e-9, (k, r[3][k])
    for ld, rows in ((sol.valid_loader, 12), (sol.test_loader, 8)):
        e = sol.evaluate(ld, *banks)
        assert e[3].shape == (rows, 1) and e[4].shape == (rows, 1)
        want = sol.get_score_from_result(e[3], e[4])
        print({k: abs(e[2][k] - want[k]) for k in ("mae", "corr")})
        SR.assert_scores(e[2], want, what=f"evaluate over {rows} rows")


def test_step_tracks_a_score_only_on_request(tail_solver):
    sol = tail_solver
    assert sol.track_score is False
    batches = [d for d in sol.train_loader if len(d[5]) == 8]
    sol.step(batches[0])
    assert sol._step_score is None
    with pytest.raises(_lib.MimrlError, match="track_score"):
        sol.read_score()
    sol.track_score = True
    preds = [sol.step(d)[3].clone() for d in batches[:4]]
    got = sol.read_score()
    p = torch.cat(preds).cpu().numpy().reshape(-1)
    y = torch.cat([d[5] for d in batches[:4]]).numpy().reshape(-1)
    assert len(p) == 32
    SR.assert_scores(got, sol.get_score_from_result(p, y), what="four steps")
    one = sol.step(batches[1])[3].clone()                     # read_score() reset the block
    SR.assert_scores(sol.read_score(reset=False), sol.get_score_from_result(one.cpu().numpy(), batches[1][5].numpy()), what="after the reset")
    two = sol.step(batches[2])[3].clone()                     # reset=False kept it
    both = (torch.cat([one, two]).cpu().numpy(), torch.cat([batches[1][5], batches[2][5]]).numpy())
    SR.assert_scores(sol.read_score(), sol.get_score_from_result(*both), what="two steps")
    sol.track_score = False


def test_main_cli_logs_the_score_table(tmp_path):
    """`python Main.py --dataset synthetic` for two epochs of regression: every key in the validation / test items of both epoch lines."""
    cmd = [sys.executable, os.path.join(ROOT, "Main.py"), "--dataset", "synthetic", "--synthetic_n", "100", "--batch_size", "16",
           "--time_len", "12", "--d_hiddens", "12-3-128=4-3-128", "--d_outs", "12-3-128=4-3-128", "--bias", "--res_project", "1-1",
           "--dropout", "0.0-0.0-0.0-0.0", "--dropout_mlp", "0.0-0.0-0.0", "--epochs_num", "2", "--stage1_n", "1",
           "--task_name", "cli_scores", "--gradient_clip", "1.5", "--learning_rate", "1e-3"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = (tmp_path / "TaskRuning" / "cli_scores" / "Running.log").read_text()
    assert "Training complete." in log and "nan" not in log.lower()
    for key in ("Val_7-class_acc:[", "Val_2(pos/neg)-class_f1:[", "Test_5-class_acc:[", "Train_mae:["):
        assert log.count(key) == 2, key
    assert "Best Valid Score mae:[" in log
