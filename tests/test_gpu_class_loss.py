"""-m gpu: --task classification (CE, Focal, BCE at 1 / 2 / 7 classes; Solver.py:172-178,324-333) at every place the step computes a task
loss and through the [num_class, 128] head -- the stand-alone op against the reference's own loss objects (tests/golden/units_cls.npz), the
head forward / backward against float64 torch, the fused HEAD mode against the separate launch bit for bit, reference trajectories
(tiny_cls*.npz) and the oracle with its task loss swapped on the separate stages, the combined step with the stage boundary inside the
critic clip + Adam and as its own launch, bf16 mode, a change of kind behind a captured graph, the deterministic build, the reference's own
Solver (epoch_tail_cls2.npz); and the one-output MAE handle, unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mimrl_amd import _lib, synth
from mimrl_amd.engine import HipEngine
from mimrl_amd.Solver import Solver
from oracle import mimrl_ref as R
from tests import class_loss_ref as CL
from tests.epoch_helpers import DrawReplay, bands, epoch_case
from tests.gpu_helpers import assert_close, grad_close, oracle_raw_grads
from tests.helpers import case, load_golden, oracle_params
from tests.test_gpu_boundary import as_datas, solver_opt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = _lib.CLASS_LOSSES
UNIT = [(tag, name) for tag, (B, C, _) in CL.UNIT_CASES.items() for name in CL.losses_for(C)]


def op_class_loss(kind, logits, y, grad=True):
    lib = _lib.load()
    x, t = logits.contiguous(), y.contiguous()
    B, C = x.shape
    dx = torch.full((B, C), 7.0, device=x.device) if grad else None
    loss = torch.full((1,), 7.0, device=x.device)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.mimrl_op_class_loss(s, int(kind), x.data_ptr(), t.data_ptr(), dx.data_ptr() if grad else None, loss.data_ptr(), B, C))
    torch.cuda.synchronize()
    return loss.item(), (dx.cpu().numpy() if grad else None)


@pytest.mark.parametrize("tag,name", UNIT)
def test_op_class_loss_vs_reference(tag, name):
    """mimrl_op_class_loss against value and autograd gradient of the reference's loss object, at the bands of
    test_gpu_task_loss.py::test_op_task_loss_vs_reference (rtol 1e-5; gradient atol 1e-5 x the largest gradient entry).  sure128c7 / CE
    adds 4 x 8.83e-11 to the gradient atol: the measured distance between the reference's own fp32 gradient (exactly 0 at the true class)
    and float64 of the same formula (class_loss_ref.GRAD_SPREAD; the case's largest gradient entry is 1.6e-11)."""
    g = load_golden("units_cls")
    x, y = (torch.from_numpy(g[f"{tag}_{k}"]).cuda() for k in ("logits", "y"))
    want_v, want_g = float(g[f"{tag}_{name}_loss"]), g[f"{tag}_{name}_grad"]
    v, dx = op_class_loss(K[name], x, y)
    print(tag, name, "value", v, want_v, "max |dgrad|", float(np.abs(dx - want_g).max()), "grad scale", float(np.abs(want_g).max()))
    assert np.isfinite(v) and np.isfinite(dx).all()
    np.testing.assert_allclose(v, want_v, rtol=1e-5, atol=1e-7)
    np.testing.assert_allclose(dx, want_g, rtol=1e-5, atol=CL.grad_atol(tag, name, want_g))
    v2, _ = op_class_loss(K[name], x, y, grad=False)                     # dlogits = NULL: the value alone, the same
    assert v2 == v


def test_op_class_loss_rejects_bad_arguments_and_bad_labels():
    lib = _lib.load()
    x = torch.zeros(1025 * 8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    p = x.data_ptr()
    for kind, B, C in ((4, 8, 2), (8, 8, 2), (5, 0, 2), (5, 1025, 2), (5, 8, 0), (5, 8, 9), (5, 8, 1), (6, 8, 1), (7, 8, 3), (7, 8, 7)):
        assert lib.mimrl_op_class_loss(s, kind, p, p, None, p, B, C) == -1, (kind, B, C)
    assert lib.mimrl_op_class_loss(s, 5, None, p, None, p, 8, 2) == -1
    assert lib.mimrl_op_task_loss(s, 5, p, p, None, p, 8) == -1                       # the regression op keeps refusing the new kinds
    # a label that is no class index: never an index, a NaN loss and NaN gradients in that row only (CE) / everywhere (Focal couples)
    logits = torch.randn(6, 3, device="cuda")
    for bad in (3.0, -1.0, 1.5, float("nan"), 1e9):
        y = torch.tensor([0.0, 1.0, 2.0, bad, 1.0, 0.0], device="cuda")
        for name in ("CE", "Focal"):
            v, dx = op_class_loss(K[name], logits, y)
            assert np.isnan(v), (name, bad, v)
            assert np.isnan(dx[3]).all()
            assert np.isfinite(np.delete(dx, 3, 0)).all() == (name == "CE")
    for C, bad in ((1, 2.0), (1, 0.5), (2, 2.0), (2, -1.0)):
        y = torch.tensor([0.0, 1.0, bad, 1.0], device="cuda")
        v, dx = op_class_loss(K["BCE"], torch.randn(4, C, device="cuda"), y)
        assert np.isnan(v) and np.isnan(dx[2]).all() and np.isfinite(np.delete(dx, 2, 0)).all()


def make(name, precision="fp32", use_graph=False, banks_on=True):
    c, opt, batch, banks = CL.cls_case(name)
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision=precision, use_graph=use_graph)
    p = oracle_params(opt, c["seed"])
    eng.load_params(p)
    eng.set_batch(*batch)
    if banks_on:
        eng.set_banks(*(banks[k] for k in "CFTAV"))
    return c, opt, batch, banks, p, eng


@pytest.mark.parametrize("name", ["tiny_cls2_ce", "tiny_cls7_ce"])
def test_head_forward_backward_vs_float64(name):
    """The [C, 128] head at C = 2 and 7.  (a) pred of mimrl_forward against float64 F_F W^T + b on the F_F the device wrote: a 128-term fp32
    dot product of |F_F| <= ~1 with |w| <= 1/sqrt(128) -- worst case 128 x 2^-24 x 11 = 8e-5, observed far lower: rtol 1e-5, atol 2e-5.
    (b) epoch-0 rule (no banks: the loss is the task loss, the F_F gradient comes from dpred alone), mimrl_stage_grads(2): the classifier
    gradients against float64 dlogits^T F_F and column sums of dlogits -- 8-term sums of fp32 products: 2e-5 of the tensor's scale.
    (c) with banks, every main-bucket gradient -- all that sits in front of the CubeMLP is a function of the CubeMLP input gradient the head
    backward starts -- against float64 autograd of the oracle at the band of test_gpu_step's gradient test (3e-3 of the tensor's scale),
    and mimrl_stage2_step's losses against it."""
    c, opt, batch, banks, p, eng = make(name, banks_on=False)
    C = opt.num_class
    assert eng.pred.shape == (c["B"], C) and eng.params["classifier.0.weight"].shape == (C, 128)
    eng.forward(train=False, with_losses=True)
    torch.cuda.synchronize()
    W, b = p["classifier.0.weight"].double(), p["classifier.0.bias"].double()
    ff = eng.feats[0].double().cpu()
    want = ff @ W.t() + b
    print(name, "max |pred - float64|", (eng.pred.double().cpu() - want).abs().max().item())
    assert_close(eng.pred.cpu().numpy(), want.numpy(), 1e-5, 2e-5, "pred vs float64 on the device's F_F")
    want_task, want_dl = CL.value_and_grad(opt.loss, eng.pred.cpu().numpy(), batch[3].numpy(), dtype=torch.float64)
    assert_close(eng.read_scalars()[_lib.S2_TASK], want_task, 1e-5, 1e-7, "task loss of the forward")
    eng.stage_grads(2)
    torch.cuda.synchronize()
    ff = eng.feats[0].double().cpu().numpy()
    grad_close(eng.grads["classifier.0.weight"].cpu().numpy(), want_dl.T @ ff, 2e-5, "classifier weight gradient", atol=1e-9)
    grad_close(eng.grads["classifier.0.bias"].cpu().numpy(), want_dl.sum(0), 2e-5, "classifier bias gradient", atol=1e-9)
    eng.close()
    # (c) with banks, against the oracle in float64
    CL_patch = pytest.MonkeyPatch()
    try:
        CL.patch_oracle(CL_patch, opt.loss, C)
        c, opt, batch, banks, p, eng = make(name)
        anchors = load_golden(name)["anchors"][0]
        main = [n for n in p if not R.is_critic_param(n)]
        eng.set_anchors(2, anchors[1], exact_ties=True)
        eng.stage_grads(2)
        torch.cuda.synchronize()
        s = eng.read_scalars().copy()
        p64 = {n: v.double() for n, v in p.items()}
        b64 = tuple(x.double() for x in batch)
        k64 = {k: v.double() for k, v in banks.items()}
        loss, mis, pred, feats, task, grads = oracle_raw_grads(p64, opt, 2, b64, k64, anchors[1], main)
        assert_close(s[_lib.S2_TASK], task.item(), 1e-3, 1e-6, "task loss vs oracle")
        assert_close(s[_lib.S2_LOSS], loss.item(), 1e-3, 1e-5, "stage-2 loss vs oracle")
        assert_close(eng.pred.cpu().numpy(), pred.numpy().reshape(-1, C), 1e-3, 2e-5, "pred vs oracle")
        bad = []
        for n in main:
            try:
                grad_close(eng.grads[n].cpu().numpy(), grads[n].numpy(), 3e-3, n)
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, f"{len(bad)}/{len(main)} gradient tensors off:\n" + "\n".join(bad[:12])
        eng.stage2_step()
        torch.cuda.synchronize()
        assert_close(eng.read_scalars()[_lib.S2_LOSS], s[_lib.S2_LOSS], 1e-6, 1e-7, "mimrl_stage2_step == mimrl_stage_grads(2)'s loss")
        eng.close()
    finally:
        CL_patch.undo()


def _worker(tmp_path, mode, knob=None):
    out = tmp_path / f"{mode}_{knob}.npz"
    env = dict(os.environ, PYTHONPATH=ROOT, MIMRL_DETERMINISTIC="1")
    for n in [n for n in env if n.startswith("MIMRL_") and n != "MIMRL_DETERMINISTIC"]:
        env.pop(n)
    if knob is not None:
        env["MIMRL_NO_FUSED_TAIL_PRE"] = knob
    r = subprocess.run([sys.executable, os.path.join(HERE, "class_loss_worker.py"), str(out), mode], env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return np.load(out)


def test_fused_head_equals_separate_launch_bit_for_bit(tmp_path):
    """C = 7, bf16 mode: the head as the last fused CubeMLP block's epilogue against head_fwd_kernel as a launch of its own
    (MIMRL_NO_FUSED_TAIL_PRE=2), a fresh child process per setting: both call head_finish (csrc/cube_bookends.h)."""
    a, b = _worker(tmp_path, "head"), _worker(tmp_path, "head", "2")
    assert sorted(a.files) == sorted(b.files) and len(a.files) == 7
    for k in a.files:
        assert np.isfinite(a[k]).all() and np.abs(a[k]).max() > 0, k
        assert np.array_equal(a[k], b[k]), f"{k}: fused vs separate head differ by {np.abs(a[k].astype(np.float64) - b[k]).max():.3e}"
    assert a["eval_pred"].shape == (8, 7)


def test_class_loss_reproducible_in_the_deterministic_build(tmp_path):
    """Two runs of three captured steps at tiny_cls7_ce leave bit-identical scalars and parameter buckets (head_bwd_cls_kernel accumulates
    through acc_add)."""
    d = _worker(tmp_path, "det")
    for k in ("scalars", "main", "crit"):
        assert np.array_equal(d["a_" + k], d["b_" + k]), k
    assert np.isfinite(d["a_scalars"]).all() and d["a_scalars"].shape[0] == 3
    g = load_golden("tiny_cls7_ce")
    assert_close(d["a_scalars"][0, _lib.S2_TASK], g["traj_s2_task"][0], 1e-3, 2e-5, "first step's task loss vs reference")


def run_steps(eng, anchors, path, steps):
    out = []
    for it in range(steps):
        eng.set_anchors(1, anchors[it, 0], exact_ties=True)              # class labels are all ties
        eng.set_anchors(2, anchors[it, 1], exact_ties=True)
        if path == "stage2":
            eng.stage1_step()
            eng.stage2_step()
        else:
            eng.step()
        torch.cuda.synchronize()
        out.append(eng.read_scalars().copy())
    return out


@pytest.mark.parametrize("path", ["stage2", "combined", "combined_frag0"])
@pytest.mark.parametrize("name", list(CL.CLS_CONFIGS))
def test_class_loss_trajectory_vs_reference_and_oracle(name, path, monkeypatch):
    """Three alternating stage-1 / stage-2 updates per step fixture vs the reference and the oracle with its task loss swapped, through
    each path that computes the task loss (see test_gpu_task_loss.py::test_task_loss_trajectory_vs_reference_and_oracle; its bands)."""
    if path == "combined_frag0":
        monkeypatch.setenv("MIMRL_ADAM_FRAG", "0")
    else:
        monkeypatch.delenv("MIMRL_ADAM_FRAG", raising=False)
    base, C, loss = CL.CLS_CONFIGS[name]
    CL.patch_oracle(monkeypatch, loss, C)
    c, opt, batch, banks, p, eng = make(name, use_graph=path != "stage2")
    assert eng.task_loss == K[loss] and eng.num_class == max(C, 1)
    if path != "stage2":
        eng.set_stage2_prefetch(1)
    g = load_golden(name)
    anchors = g["anchors"]
    crit = [n for n in p if R.is_critic_param(n)]
    main = [n for n in p if not R.is_critic_param(n)]
    adam_v, adam_m = R.AdamState(p, crit), R.AdamState(p, main)
    for it in range(3):
        s = run_steps(eng, anchors[it:], path, 1)[0]
        r1, r2 = R.two_stage_step(p, opt, adam_v, adam_m, batch, banks, anchors[it, 0], anchors[it, 1])
        rt, at = (1e-3, 2e-5) if it == 0 else (3e-2, 5e-3)
        print(name, path, it, "task", s[_lib.S2_TASK], g["traj_s2_task"][it], "s2", s[_lib.S2_LOSS], g["traj_s2_loss"][it], r2["loss"].item(),
              "s1", s[_lib.S1_LOSS], g["traj_s1_loss"][it])
        assert_close(s[_lib.S2_TASK], g["traj_s2_task"][it], rt, at, f"{name} {path} it{it} task vs reference")
        assert_close(s[_lib.S2_LOSS], g["traj_s2_loss"][it], rt, at, f"{name} {path} it{it} s2 loss vs reference")
        assert_close(s[_lib.S1_LOSS], g["traj_s1_loss"][it], rt, at, f"{name} {path} it{it} s1 loss vs reference")
        assert_close(s[_lib.S2_LOSS], r2["loss"].item(), rt, at, f"{name} {path} it{it} s2 loss vs oracle")
        if it == 0:
            names2 = [str(x) for x in g["s2_gnorm_names"]]
            ps = np.array([eng.params[n].double().sum().item() for n in names2])
            np.testing.assert_allclose(ps, g["s2_psum_after"], rtol=1e-4, atol=0.05)
    if path == "stage2":
        # forward (eval, with losses) and estimate(2): S2_TASK == the op's value on the predictions of that forward
        eng.forward(train=False, with_losses=True)
        torch.cuda.synchronize()
        s = eng.read_scalars()
        want, _ = op_class_loss(K[loss], eng.pred.reshape(c["B"], -1), eng.labels, grad=False)
        np.testing.assert_allclose(s[_lib.S2_TASK], want, rtol=1e-6, atol=1e-7)
        eng.scalars.zero_()
        eng.estimate(2)
        torch.cuda.synchronize()
        np.testing.assert_allclose(eng.read_scalars()[_lib.S2_TASK], want, rtol=1e-6, atol=1e-7)
    eng.close()


@pytest.mark.parametrize("name", list(CL.CLS_CONFIGS))
def test_class_loss_bf16_mode_vs_reference(name):
    """bf16 mode, one combined step per step fixture at the bf16 bands of test_gpu_task_loss.py."""
    c, opt, batch, banks, p, eng = make(name, precision="bf16", use_graph=True)
    eng.set_stage2_prefetch(1)
    g = load_golden(name)
    s = run_steps(eng, g["anchors"], "combined", 1)[0]
    print(name, "bf16 task", s[_lib.S2_TASK], g["traj_s2_task"][0], "s2", s[_lib.S2_LOSS], g["traj_s2_loss"][0])
    assert_close(s[_lib.S2_TASK], g["traj_s2_task"][0], 2e-2, 1e-3, f"bf16 {name} task")
    assert_close(s[_lib.S2_LOSS], g["traj_s2_loss"][0], 2e-2, 1e-3, f"bf16 {name} s2 loss")
    eng.close()


def test_kind_change_after_capture_takes_effect():
    """C = 7: a captured combined step (CE), then set_task_loss(Focal): the next step runs Focal -- the same as the uncaptured separate
    stages that switch at the same point.  Kinds the handle cannot run are refused and leave it as it was."""
    res = {}
    for path in ("combined", "stage2"):
        c, opt, batch, banks, p, eng = make("tiny_cls7_ce", use_graph=path == "combined")
        if path == "combined":
            eng.set_stage2_prefetch(1)
        anchors = load_golden("tiny_cls7_ce")["anchors"]
        s0 = run_steps(eng, anchors, path, 1)[0]
        lib = _lib.load()
        assert lib.mimrl_set_class_loss(eng.handle, 7) == -1 and lib.mimrl_set_class_loss(eng.handle, 4) == -1     # BCE at 7 classes; a regression kind
        assert lib.mimrl_set_class_loss(eng.handle, 8) == -1 and lib.mimrl_set_task_loss(eng.handle, 0) == -1     # unknown; MAE on [B, 7] logits
        eng.set_task_loss(K["Focal"])
        assert eng.task_loss == K["Focal"]
        s1 = run_steps(eng, anchors[1:], path, 1)[0]
        res[path] = (s0, s1)
        eng.close()
    g = load_golden("tiny_cls7_ce")
    assert_close(res["combined"][0][_lib.S2_TASK], g["traj_s2_task"][0], 1e-3, 2e-5, "CE step before the switch")
    a, b = res["combined"][1], res["stage2"][1]
    assert_close(a[_lib.S2_TASK], b[_lib.S2_TASK], 1e-3, 2e-5, "Focal step after the switch")
    assert_close(a[_lib.S2_LOSS], b[_lib.S2_LOSS], 1e-3, 2e-5, "stage-2 loss after the switch")
    ce = g["traj_s2_task"][1]                                            # Focal of a batch-mean CE near the reference's second step
    assert abs(a[_lib.S2_TASK] - res["combined"][0][_lib.S2_TASK]) > 1e-2
    assert_close(a[_lib.S2_TASK], (1 - np.exp(-ce)) ** 2 * ce, 5e-2, 5e-3, "Focal = (1 - exp(-ce))^2 ce")


def test_solver_epochs_with_ce_match_reference_solver(monkeypatch):
    """mimrl_amd.Solver.train / evaluate with --task classification --num_class 2 --loss CE over the epochs of epoch_tail (a partial last
    batch of 4 on the shared handle) == the reference's own Solver (epoch_tail_cls2.npz): losses, predictions, banks, accuracy and F1."""
    c, opt, sets, _ = epoch_case("epoch_tail")
    g = load_golden("epoch_tail_cls2")
    cls = lambda b: (b[0], b[1], b[2], torch.from_numpy(synth.class_labels(b[3].numpy(), 2)))
    loaders = tuple([as_datas(cls(b)) for b in sets[k]] for k in ("train", "valid", "test")) + (768, 74, 35)
    sol = Solver(solver_opt(opt, loss="CE", task="classification", num_class=2), loaders)
    so = sol.opt
    sol.model.load_state_dict(oracle_params(so, c["seed"]))
    draw = DrawReplay(g)
    monkeypatch.setattr(synth, "draw_anchors", lambda N, m, calls=6: draw(N, m))
    banks = ([], [], [], [], [])
    for ep in range(c["epochs"]):
        rt, at, aat = bands(ep)
        r = sol.train(ep, sol.train_loader, *banks)
        banks = r[4:]
        assert_close(r[0], g[f"ep{ep}_train_loss"], rt, at, f"ep{ep} train loss")
        assert_close(r[1], g[f"ep{ep}_train_loss_mi"], rt, at, f"ep{ep} stage-1 loss")
        assert_close(r[2], g[f"ep{ep}_train_mis"], rt, at, f"ep{ep} MI means")
        assert sorted(r[3]) == ["2-class_acc", "2-f1"]
        assert_close(r[3]["2-class_acc"], g[f"ep{ep}_train_acc"], rt, at, f"ep{ep} train accuracy")
        assert_close(r[3]["2-f1"], g[f"ep{ep}_train_f1"], rt, at, f"ep{ep} train F1")
        for k, bk in zip("CFTAV", banks):
            assert_close(bk.cpu().numpy(), g[f"ep{ep}_bank_{k}"], rt, aat, f"ep{ep} bank {k}")
        for tag, ld in (("valid", sol.valid_loader), ("test", sol.test_loader)):
            e = sol.evaluate(ld, *banks)
            assert_close(e[0], g[f"ep{ep}_{tag}_loss"], rt, at, f"ep{ep} {tag} loss")
            assert e[3].shape[1] == 2
            assert_close(e[3].reshape(-1), g[f"ep{ep}_{tag}_pred"], rt, aat, f"ep{ep} {tag} predictions")
            assert_close(e[2]["2-class_acc"], g[f"ep{ep}_{tag}_acc"], rt, at, f"ep{ep} {tag} accuracy")
            assert_close(e[2]["2-f1"], g[f"ep{ep}_{tag}_f1"], rt, at, f"ep{ep} {tag} F1")
    assert draw.done()
    assert list(sol._tails) == [4] and all(e.task_loss == K["CE"] and e.num_class == 2 for e in sol._tails.values())
    names = [str(n) for n in g["final_names"]]
    ps = np.array([sol.model.state_dict()[n].double().sum().item() for n in names])
    np.testing.assert_allclose(ps, g["final_psum"], rtol=1e-3, atol=0.05)


def test_one_class_mae_handle_is_unchanged():
    """A num_class = 1 MAE handle created after this change reproduces tiny_sep's reference fixture (three steps at the bands of
    test_gpu_task_loss.py), and refuses every classification kind except BCE's setter argument check order: CE -> -1."""
    c, opt, batch, banks = case("tiny_sep")
    assert opt.num_class == 1
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], use_graph=True)
    assert eng.task_loss == _lib.TASK_LOSSES["MAE"] and eng.pred.shape == (c["B"],) and eng.cfg.num_class == 1
    lib = _lib.load()
    assert lib.mimrl_set_class_loss(eng.handle, 5) == -1 and lib.mimrl_set_class_loss(eng.handle, 6) == -1
    assert lib.mimrl_set_task_loss(eng.handle, 5) == -1
    eng.load_params(oracle_params(opt, c["seed"]))
    eng.set_batch(*batch)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    eng.set_stage2_prefetch(1)
    g = load_golden("tiny_sep")
    for it in range(3):
        eng.set_anchors(1, g["anchors"][it, 0])
        eng.set_anchors(2, g["anchors"][it, 1])
        eng.step()
        torch.cuda.synchronize()
        s = eng.read_scalars()
        rt, at = (1e-3, 2e-5) if it == 0 else (3e-2, 5e-3)
        assert_close(s[_lib.S2_TASK], g["traj_s2_task"][it], rt, at, f"it{it} MAE vs reference")
        assert_close(s[_lib.S2_LOSS], g["traj_s2_loss"][it], rt, at, f"it{it} s2 loss vs reference")
        assert_close(s[_lib.S1_LOSS], g["traj_s1_loss"][it], rt, at, f"it{it} s1 loss vs reference")
    eng.close()
    # a zero-initialised tail (num_class = 0, what a caller built against the shorter struct's initialiser passes) is the same handle
    opt.num_class = 0
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"])
    assert eng.cfg.num_class == 0 and eng.num_class == 1 and eng.task_loss == 0 and eng.pred.shape == (c["B"],)
    eng.close()


@pytest.mark.parametrize("num_class,loss", [(7, "CE"), (2, "BCE")])
def test_main_cli_trains_a_classifier(num_class, loss, tmp_path):
    """`python Main.py --dataset synthetic --task classification --num_class C --loss L`: two epochs end to end, finite losses, accuracy
    and F1 in the epoch log lines and in the final scores."""
    cmd = [sys.executable, os.path.join(ROOT, "Main.py"), "--dataset", "synthetic", "--synthetic_n", "100", "--batch_size", "16",
           "--time_len", "12", "--d_hiddens", "12-3-128=4-3-128", "--d_outs", "12-3-128=4-3-128", "--bias", "--res_project", "1-1",
           "--dropout", "0.0-0.0-0.0-0.0", "--dropout_mlp", "0.0-0.0-0.0", "--epochs_num", "2", "--stage1_n", "1", "--task", "classification",
           "--num_class", str(num_class), "--loss", loss, "--task_name", "cli_cls", "--gradient_clip", "1.5", "--learning_rate", "1e-3"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = (tmp_path / "TaskRuning" / "cli_cls" / "Running.log").read_text()
    assert "Training complete." in log and "nan" not in log.lower()
    for key in (f"Val_{num_class}-class_acc:[", f"Val_{num_class}-f1:[", f"Test_{num_class}-class_acc:[", f"Train_{num_class}-class_acc:["):
        assert log.count(key) == 2, key
    assert f"Best Valid Score {num_class}-class_acc:[" in log
