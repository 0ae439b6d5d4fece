"""CPU: --task classification on the Python surface (--loss CE / Focal / BCE with --num_class; Parameters.py:22-23,55, Solver.py:172-178,
324-356) -- the flag-to-kind mapping and its refusals, the restated losses against the reference's own loss objects
(tests/golden/units_cls.npz), the numpy scores against scikit-learn, the native layout of a [num_class, D] classifier, the synthetic
class labels, and a stand-alone sanitized host program on the layout entry points."""
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest
import torch

from mimrl_amd import Parameters, Utils, _lib, layout, synth
from tests import class_loss_ref as CL
from tests.golden.configs import CONFIGS, make_opt
from tests.helpers import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(tag, name) for tag, (B, C, _) in CL.UNIT_CASES.items() for name in CL.losses_for(C)]


def opt(loss, task="classification", num_class=1):
    return types.SimpleNamespace(loss=loss, task=task, num_class=num_class)


def test_task_loss_code_maps_the_classification_losses():
    assert _lib.CLASS_LOSSES == CL.KINDS == {"CE": 5, "Focal": 6, "BCE": 7}
    assert _lib.TASK_LOSSES == {"MAE": 0, "MSE": 1, "RMSE": 2, "SIMSE": 3, "CCC": 4}
    for C in (2, 7, 8):
        assert _lib.task_loss_code(opt("CE", num_class=C)) == 5
        assert _lib.task_loss_code(opt("Focal", num_class=C)) == 6
    for C in (1, 2):
        assert _lib.task_loss_code(opt("BCE", num_class=C)) == 7


def test_task_loss_code_refusals():
    for loss in ("CE", "Focal", "BCE"):                                   # a classification loss without --task classification
        with pytest.raises(NotImplementedError, match="--task classification"):
            _lib.task_loss_code(opt(loss, task="regression", num_class=2))
        with pytest.raises(NotImplementedError, match="classification"):
            _lib.task_loss_code(types.SimpleNamespace(loss=loss))
    for loss in ("CE", "Focal"):
        for C in (0, 1, 9):
            with pytest.raises(NotImplementedError, match="num_class"):
                _lib.task_loss_code(opt(loss, num_class=C))
    for C in (0, 3, 7):                                                   # Solver.py:336-337
        with pytest.raises(NotImplementedError, match="BCE needs --num_class 1 or 2"):
            _lib.task_loss_code(opt("BCE", num_class=C))
    for loss in _lib.TASK_LOSSES:                                         # a regression loss on a classification head
        with pytest.raises(NotImplementedError, match="regression loss"):
            _lib.task_loss_code(opt(loss, num_class=1))
        with pytest.raises(NotImplementedError, match="regression loss"):
            _lib.task_loss_code(opt(loss, task="regression", num_class=2))
        assert _lib.task_loss_code(opt(loss, task="regression", num_class=1)) == _lib.TASK_LOSSES[loss]


def test_task_loss_code_data_parallel():
    """CE and BCE are means of per-row terms; Focal couples the batch (the focal factor sits on the batch-mean cross entropy)."""
    assert _lib.task_loss_code(opt("CE", num_class=7), world=4) == 5
    assert _lib.task_loss_code(opt("BCE", num_class=2), world=4) == 7
    assert _lib.task_loss_code(opt("Focal", num_class=7), world=1) == 6
    with pytest.raises(NotImplementedError, match="couples the whole batch"):
        _lib.task_loss_code(opt("Focal", num_class=7), world=2)


def test_header_declares_the_class_loss_kinds_and_the_cfg_tail():
    h = open(os.path.join(ROOT, "include", "mimrl.h")).read()
    found = dict((n, int(v)) for n, v in re.findall(r"MIMRL_CLASS_LOSS_([A-Z]+) = (\d+)", h))
    assert found == {k.upper(): v for k, v in _lib.CLASS_LOSSES.items()}
    assert int(re.search(r"#define MIMRL_MAX_CLASSES (\d+)", h).group(1)) == _lib.MAX_CLASSES == 8
    members = re.findall(r"^\s+(?:int32_t|uint64_t|float)\s+([a-z_0-9]+)", re.search(r"typedef struct mimrl_cfg \{(.*?)\} mimrl_cfg;", h, re.S).group(1), re.M)
    assert members[-2:] == ["seed", "num_class"]                          # appended at the tail, behind seed
    assert [f[0] for f in _lib.Cfg._fields_][-2:] == ["seed", "num_class"]
    assert _lib.Cfg().num_class == 0                                      # a zero-initialised cfg: the one-output head
    o = make_opt(CONFIGS["tiny_sep"])
    assert _lib.make_cfg(o, 768, 74, 35).num_class == 1
    o.num_class = 7
    assert _lib.make_cfg(o, 768, 74, 35).num_class == 7
    del o.num_class
    assert _lib.make_cfg(o, 768, 74, 35).num_class == 1


@pytest.mark.parametrize("tag,name", CASES)
def test_restated_losses_equal_the_reference(tag, name):
    """tests/class_loss_ref.py (what the GPU tests hand the oracle) and Utils.TASK_LOSS_FUNCTIONS (Solver.compute_loss) against the value
    and autograd gradient of the reference's own loss object; float64 of the same formula too, which is what bounds the fp32 kernels.
    Bands: those of tests/test_gpu_task_loss.py's op test; sure128c7 / CE adds 4 x the measured fp32-vs-float64 spread of the reference's
    own gradient, 8.83e-11 (class_loss_ref.GRAD_SPREAD)."""
    g = load_golden("units_cls")
    B, C, _ = CL.UNIT_CASES[tag]
    x, y = g[f"{tag}_logits"], g[f"{tag}_y"]
    assert x.shape == (B, C) and y.shape == (B,)
    x2, y2 = CL.unit_vectors(tag)
    assert np.array_equal(x, x2) and np.array_equal(y, y2)
    want_v, want_g = float(g[f"{tag}_{name}_loss"]), g[f"{tag}_{name}_grad"]
    gs = float(np.abs(want_g).max())
    for dtype in (torch.float32, torch.float64):
        v, grad = CL.value_and_grad(name, x, y, dtype=dtype)
        np.testing.assert_allclose(v, want_v, rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(grad, want_g, rtol=1e-5, atol=CL.grad_atol(tag, name, want_g))
    v, grad = CL.value_and_grad(name, x, y, fn=Utils.TASK_LOSS_FUNCTIONS[name])
    np.testing.assert_allclose(v, want_v, rtol=1e-6, atol=1e-7)
    np.testing.assert_allclose(grad, want_g, rtol=1e-6, atol=1e-6 * gs + 1e-12)


def test_fixtures_cover_the_edge_cases():
    g = load_golden("units_cls")
    for k in g.files:
        assert np.isfinite(g[k]).all(), k
    x = g["eq128c7_logits"]
    assert np.all(x == x[0, 0])
    np.testing.assert_allclose(float(g["eq128c7_CE_loss"]), np.log(7.0), rtol=1e-6)
    for tag in ("big128c7", "big128c2", "big128c1"):
        assert np.abs(g[tag + "_logits"]).max() == 80.0
    assert float(g["big128c7_CE_loss"]) > 10.0
    # the true class ahead by 20: CE ~ 6 exp(-20) is below fp32's resolution next to 1, Focal's (1 - p)^2 smaller still
    x, y = g["sure128c7_logits"], g["sure128c7_y"].astype(np.int64)
    other = np.where(np.arange(7)[None] == y[:, None], -np.inf, x).max(1)
    assert np.all(x[np.arange(128), y] - other >= 20.0 - 1e-5)
    assert 0.0 <= float(g["sure128c7_CE_loss"]) < 1e-7 and 0.0 <= float(g["sure128c7_Focal_loss"]) < 1e-14
    assert np.abs(g["sure128c7_CE_grad"]).max() < 1e-9 and np.abs(g["sure128c7_Focal_grad"]).max() < 1e-14
    # Focal is the focal factor on the batch-mean CE, not a mean of per-row focal terms
    ce = float(g["b128c7_CE_loss"])
    np.testing.assert_allclose(float(g["b128c7_Focal_loss"]), (1 - np.exp(-ce)) ** 2 * ce, rtol=1e-5)
    for tag, (B, C, _) in CL.UNIT_CASES.items():
        yy = g[tag + "_y"]
        assert np.all(yy == np.round(yy)) and yy.min() >= 0 and yy.max() < max(C, 2)


@pytest.mark.parametrize("C", [2, 7])
def test_numpy_scores_equal_scikit_learn(C):
    from sklearn.metrics import accuracy_score, f1_score
    from mimrl_amd.Solver import Solver
    g = np.random.Generator(np.random.PCG64(30 + C))
    for trial in range(4):
        n = 57 + trial
        t = g.integers(0, C, size=n)
        logits = g.standard_normal((n, C)).astype(np.float32)
        logits[np.arange(n), t] += 0.8                                    # better than chance, far from perfect
        if trial >= 2:
            logits[:, C - 1] = -50.0                                      # a class absent from the predictions
        sol = Solver.__new__(Solver)
        sol.opt = types.SimpleNamespace(task="classification", num_class=C)
        s = sol.get_score_from_result(logits, t.astype(np.float32).reshape(-1, 1))
        pred = logits.argmax(1)
        if trial >= 2:
            assert (pred == C - 1).sum() == 0 and (t == C - 1).sum() > 0
        np.testing.assert_allclose(s[f"{C}-class_acc"], accuracy_score(t, pred), rtol=0, atol=1e-12)
        np.testing.assert_allclose(s[f"{C}-f1"], f1_score(t, pred, average="weighted"), rtol=0, atol=1e-12)
        np.testing.assert_allclose(Utils.weighted_f1(t, pred), f1_score(t, pred, average="weighted"), rtol=0, atol=1e-12)
    # one class: the sign of the logit
    t = g.integers(0, 2, size=64)
    x = (g.standard_normal(64) + (t - 0.5)).astype(np.float32)
    sol.opt = types.SimpleNamespace(task="classification", num_class=1)
    s = sol.get_score_from_result(x.reshape(-1, 1), t.astype(np.float32).reshape(-1, 1))
    np.testing.assert_allclose(s["1-class_acc"], accuracy_score(t, x > 0), atol=1e-12)
    np.testing.assert_allclose(s["1-f1"], f1_score(t, (x > 0).astype(np.int64), average="weighted"), atol=1e-12)
    # accuracy compares upwards (Solver.py:428-429); regression keeps mae downwards
    sol.opt = types.SimpleNamespace(task="classification", num_class=C)
    k = f"{C}-class_acc"
    assert sol.current_result_better(None, {k: 0.1}) and sol.current_result_better({k: 0.5}, {k: 0.6})
    assert not sol.current_result_better({k: 0.5}, {k: 0.5}) and not sol.current_result_better({k: 0.5}, {k: 0.4})
    sol.opt = types.SimpleNamespace(task="regression", num_class=1)
    assert sol.current_result_better({"mae": 0.5}, {"mae": 0.4}) and not sol.current_result_better({"mae": 0.5}, {"mae": 0.6})


def test_product_code_does_not_import_scikit_learn_for_the_scores():
    for f in ("Solver.py", "Utils.py"):
        assert not re.search(r"^\s*(?:import|from)\s+sklearn", open(os.path.join(ROOT, "mimrl_amd", f)).read(), re.M)


@pytest.mark.parametrize("C", [2, 7])
@pytest.mark.parametrize("name", ["tiny_sep", "tiny_cat", "tiny_conv"])
def test_native_layout_matches_python_with_classes(name, C):
    o = make_opt(CONFIGS[name])
    base, base_sizes = _lib.layout_entries(_lib.make_cfg(o, 768, 74, 35, bank_capacity=CONFIGS[name]["N"]))
    o.num_class = C
    entries, sizes = _lib.layout_entries(_lib.make_cfg(o, 768, 74, 35, bank_capacity=CONFIGS[name]["N"]))
    py_entries, py_sizes = layout.build_layout(o, 768, 74, 35)
    assert len(entries) == len(py_entries) == len(base)
    for (n, g, off, shape), e in zip(entries, py_entries):
        assert (n, off, tuple(shape)) == (e.name, e.offset, e.shape)
        assert g == (1 if e.group == "critic" else 0)
    assert sizes == (py_sizes["main"], py_sizes["critic"])
    shapes = {n: tuple(s) for n, _, _, s in entries}
    assert shapes["classifier.0.weight"] == (C, 128) and shapes["classifier.0.bias"] == (C,)
    assert sizes[1] == base_sizes[1] and sizes[0] == base_sizes[0] + (C - 1) * 128


def test_too_many_classes_are_refused_by_name():
    o = make_opt(CONFIGS["tiny_sep"])
    o.num_class = 9
    with pytest.raises(_lib.MimrlError, match="num_class"):
        _lib.layout_entries(_lib.make_cfg(o, 768, 74, 35))
    o.num_class = 8
    assert dict((n, s) for n, _, _, s in _lib.layout_entries(_lib.make_cfg(o, 768, 74, 35))[0])["classifier.0.bias"] == (8,)


@pytest.mark.parametrize("C", [1, 2, 3, 5, 7, 8])
def test_synthetic_class_labels(C):
    _, _, _, y = synth.synthetic_batch(400, 2, seed=3)
    lab = synth.class_labels(y, C)
    assert lab.dtype == np.float32 and lab.shape == y.shape and np.all(lab == np.round(lab))
    assert sorted(set(lab.tolist())) == list(range(max(C, 2)))           # in range, and every class occurs
    assert np.array_equal(lab, synth.class_labels(y, C))                  # a pure function of the label
    if C <= 2:
        assert np.array_equal(lab, (y >= 0).astype(np.float32))
    if C == 7:
        assert np.array_equal(lab, np.clip(np.round(y), -3, 3) + 3)
    assert np.all(np.diff(lab[np.argsort(y, kind="stable")]) >= 0)        # monotone in the regression label


def test_synthetic_loader_serves_class_labels():
    from mimrl_amd import data
    o = Parameters.parse_args(["--dataset", "synthetic", "--synthetic_n", "64", "--batch_size", "16", "--time_len", "4", "--task",
                               "classification", "--num_class", "7", "--loss", "CE"])
    assert _lib.task_loss_code(o) == 5
    tr, va, te = data.get_data_loader(o)[:3]
    y = torch.cat([d[5].cpu() for d in tr]).reshape(-1).numpy()
    _, _, _, y0 = synth.synthetic_batch(64, 4, seed=o.seed)
    assert np.array_equal(y, synth.class_labels(y0, 7))
    o = Parameters.parse_args(["--dataset", "synthetic", "--synthetic_n", "64", "--batch_size", "16", "--time_len", "4"])
    y = torch.cat([d[5].cpu() for d in data.get_data_loader(o)[0]]).reshape(-1).numpy()
    assert np.array_equal(y, y0)                                          # regression: the labels of before


def test_layout_entry_points_under_sanitizers(tmp_path):
    """tests/layout_cls_main.cpp + the host-only sources of the library, -fsanitize=address,undefined: mimrl_layout_count /
    mimrl_layout_entry at num_class 0, 1, 7 (shapes, offsets, a short name buffer) and 9 / -1 (refused by name)."""
    hipcc = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    assert os.path.exists(hipcc), "hipcc not found"
    csrc = os.path.join(ROOT, "mimrl_amd", "csrc")
    exe = str(tmp_path / "layout_cls")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer"]
    cmd = [hipcc, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "--offload-arch=gfx950"] + [a for f in san for a in ("-Xarch_host", f)] + \
          [os.path.join(ROOT, "tests", "layout_cls_main.cpp")] + [os.path.join(csrc, f) for f in ("layout.cpp", "errors.cpp", "host_abi.cpp")] + ["-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "layout cls ok" in r.stdout and "FAILED" not in r.stdout
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr
