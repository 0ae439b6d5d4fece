"""-m gpu: the regression task losses of --loss (MSE, RMSE, SIMSE, CCC; Solver.py:172-192) at every place the step computes a task loss --
the stand-alone op, the separate stage-2 step, the combined step with the stage boundary inside the critic clip + Adam (and as its own
launch, MIMRL_ADAM_FRAG=0), forward / estimate -- against the reference's own loss objects (tests/golden/units_losses.npz), reference
trajectories (tiny_sep_<loss>.npz), the oracle with its task loss swapped, and the reference's Solver (epoch_tail_ccc.npz); and MAE,
which bench.py times, unchanged."""
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
from tests import task_loss_ref as TL
from tests.epoch_helpers import DrawReplay, bands, epoch_case
from tests.gpu_helpers import assert_close
from tests.helpers import case, load_golden, oracle_params
from tests.test_gpu_boundary import as_datas, solver_opt

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
K = _lib.TASK_LOSSES
NEW = ["MSE", "RMSE", "SIMSE", "CCC"]
UNIT_CASES = (("b2", 2), ("b7", 7), ("b128", 128), ("b1024", 1024), ("const128", 128), ("zero7", 7))   # make_golden_losses.py


def op_task_loss(kind, pred, y, grad=True):
    lib = _lib.load()
    p, t = pred.contiguous(), y.contiguous()
    B = p.numel()
    dp = torch.full((B,), 7.0, device=p.device) if grad else None
    loss = torch.full((1,), 7.0, device=p.device)
    s = torch.cuda.current_stream().cuda_stream
    _lib.check(lib.mimrl_op_task_loss(s, int(kind), p.data_ptr(), t.data_ptr(), dp.data_ptr() if grad else None, loss.data_ptr(), B))
    torch.cuda.synchronize()
    return loss.item(), (dp.cpu().numpy() if grad else None)


@pytest.mark.parametrize("tag,B", UNIT_CASES)
@pytest.mark.parametrize("name", list(K))
def test_op_task_loss_vs_reference(tag, B, name):
    g = load_golden("units_losses")
    pred, y = (torch.from_numpy(g[f"{tag}_{k}"]).cuda() for k in ("pred", "y"))
    want_v, want_g = float(g[f"{tag}_{name}_loss"]), g[f"{tag}_{name}_grad"]
    v, dp = op_task_loss(K[name], pred, y)
    np.testing.assert_allclose(v, want_v, rtol=1e-5, atol=1e-7)
    gscale = float(np.nanmax(np.abs(want_g))) if np.isfinite(want_g).any() else 0.0
    np.testing.assert_allclose(dp, want_g, rtol=1e-5, atol=1e-5 * gscale + 1e-12, equal_nan=True)
    if tag == "zero7" and name == "RMSE":
        assert np.isnan(dp).all(), dp                                     # torch: NaN where the residual is zero
    v2, _ = op_task_loss(K[name], pred, y, grad=False)                   # dpred = NULL: the value alone, the same
    assert v2 == v


def test_op_task_loss_rejects_bad_arguments():
    lib = _lib.load()
    x = torch.zeros(8, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    assert lib.mimrl_op_task_loss(s, 5, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 8) == -1
    assert lib.mimrl_op_task_loss(s, 0, x.data_ptr(), x.data_ptr(), None, x.data_ptr(), 1025) == -1
    eng = make("tiny_sep", "MAE")[-1]
    assert lib.mimrl_set_task_loss(eng.handle, -1) == -1 and lib.mimrl_set_task_loss(eng.handle, 5) == -1
    eng.close()


def make(name, loss, precision="fp32", use_graph=False):
    c, opt, batch, banks = case(name)
    opt.loss = loss
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision=precision, use_graph=use_graph)
    p = oracle_params(opt, c["seed"])
    eng.load_params(p)
    eng.set_batch(*batch)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    return c, opt, batch, banks, p, eng


def run_steps(eng, anchors, path, steps):
    """`path`: 'stage2' = mimrl_stage1_step + mimrl_stage2_step (what Solver.train runs); 'combined' = mimrl_two_stage_step (captured graph,
    stage-2 prefetch on: the combined step with the stage boundary fused)."""
    out = []
    for it in range(steps):
        eng.set_anchors(1, anchors[it, 0])
        eng.set_anchors(2, anchors[it, 1])
        if path == "stage2":
            eng.stage1_step()
            eng.stage2_step()
        else:
            eng.step()
        torch.cuda.synchronize()
        out.append(eng.read_scalars().copy())
    return out


@pytest.mark.parametrize("path", ["stage2", "combined", "combined_frag0"])
@pytest.mark.parametrize("loss", NEW)
def test_task_loss_trajectory_vs_reference_and_oracle(loss, path, monkeypatch):
    """Three alternating stage-1 / stage-2 updates with --loss <loss> vs the reference (tiny_sep_<loss>.npz) and the oracle with the task
    loss swapped, through each path that computes the task loss: the separate stages (task_loss_kernel), the combined captured step with
    the stage boundary in workgroup 0 of the critic clip + Adam (adam8_kernel), and the same with the boundary as its own launch
    (MIMRL_ADAM_FRAG=0: stage_boundary_kernel)."""
    if path == "combined_frag0":
        monkeypatch.setenv("MIMRL_ADAM_FRAG", "0")
    else:
        monkeypatch.delenv("MIMRL_ADAM_FRAG", raising=False)
    TL.patch_oracle(monkeypatch, loss)
    c, opt, batch, banks, p, eng = make("tiny_sep", loss, use_graph=path != "stage2")
    assert eng.task_loss == K[loss]
    if path != "stage2":
        eng.set_stage2_prefetch(1)
    g = load_golden("tiny_sep_" + loss.lower())
    anchors = g["anchors"]
    crit = [n for n in p if R.is_critic_param(n)]
    main = [n for n in p if not R.is_critic_param(n)]
    adam_v, adam_m = R.AdamState(p, crit), R.AdamState(p, main)
    for it in range(3):
        s = run_steps(eng, anchors[it:], path, 1)[0]
        r1, r2 = R.two_stage_step(p, opt, adam_v, adam_m, batch, banks, anchors[it, 0], anchors[it, 1])
        rt, at = (1e-3, 2e-5) if it == 0 else (3e-2, 5e-3)
        assert_close(s[_lib.S2_TASK], g["traj_s2_task"][it], rt, at, f"{loss} {path} it{it} task vs reference")
        assert_close(s[_lib.S2_LOSS], g["traj_s2_loss"][it], rt, at, f"{loss} {path} it{it} s2 loss vs reference")
        assert_close(s[_lib.S1_LOSS], g["traj_s1_loss"][it], rt, at, f"{loss} {path} it{it} s1 loss vs reference")
        assert_close(s[_lib.S2_LOSS], r2["loss"].item(), rt, at, f"{loss} {path} it{it} s2 loss vs oracle")
        if it == 0:
            names2 = [str(x) for x in g["s2_gnorm_names"]]
            ps = np.array([eng.params[n].double().sum().item() for n in names2])
            np.testing.assert_allclose(ps, g["s2_psum_after"], rtol=1e-4, atol=0.05)
    if path == "stage2":
        # forward (eval, with losses) and estimate(2): S2_TASK == the op's value on the predictions of that forward
        eng.forward(train=False, with_losses=True)
        torch.cuda.synchronize()
        s = eng.read_scalars()
        want, _ = op_task_loss(K[loss], eng.pred, eng.labels, grad=False)
        np.testing.assert_allclose(s[_lib.S2_TASK], want, rtol=1e-6, atol=1e-7)
        eng.scalars.zero_()
        eng.estimate(2)
        torch.cuda.synchronize()
        np.testing.assert_allclose(eng.read_scalars()[_lib.S2_TASK], want, rtol=1e-6, atol=1e-7)
    eng.close()


@pytest.mark.parametrize("loss", NEW)
def test_task_loss_bf16_mode_vs_reference(loss):
    """bf16 mode, combined step: the first step's losses at the bf16 bands of test_gpu_step.test_bf16_mode_tracks_fp32."""
    c, opt, batch, banks, p, eng = make("tiny_sep", loss, precision="bf16", use_graph=True)
    eng.set_stage2_prefetch(1)
    g = load_golden("tiny_sep_" + loss.lower())
    s = run_steps(eng, g["anchors"], "combined", 1)[0]
    assert_close(s[_lib.S2_TASK], g["traj_s2_task"][0], 2e-2, 1e-3, f"bf16 {loss} task")
    assert_close(s[_lib.S2_LOSS], g["traj_s2_loss"][0], 2e-2, 1e-3, f"bf16 {loss} s2 loss")
    eng.close()


def test_kind_change_after_capture_takes_effect():
    """A captured combined step (MAE), then set_task_loss(CCC): the next step runs CCC -- the same as the uncaptured separate stages
    that switch at the same point."""
    res = {}
    for path in ("combined", "stage2"):
        c, opt, batch, banks, p, eng = make("tiny_sep", "MAE", use_graph=path == "combined")
        if path == "combined":
            eng.set_stage2_prefetch(1)
        anchors = load_golden("tiny_sep")["anchors"]
        s0 = run_steps(eng, anchors, path, 1)[0]
        eng.set_task_loss(K["CCC"])
        s1 = run_steps(eng, anchors[1:], path, 1)[0]
        res[path] = (s0, s1)
        eng.close()
    g = load_golden("tiny_sep")
    assert_close(res["combined"][0][_lib.S2_TASK], g["traj_s2_task"][0], 1e-3, 2e-5, "MAE step before the switch")
    a, b = res["combined"][1], res["stage2"][1]
    assert_close(a[_lib.S2_TASK], b[_lib.S2_TASK], 1e-3, 2e-5, "CCC step after the switch")
    assert_close(a[_lib.S2_LOSS], b[_lib.S2_LOSS], 1e-3, 2e-5, "stage-2 loss after the switch")
    assert abs(a[_lib.S2_TASK] - res["combined"][0][_lib.S2_TASK]) > 1e-3


def test_solver_epochs_with_ccc_match_reference_solver(monkeypatch):
    """mimrl_amd.Solver.train / evaluate with --loss CCC over the epochs of epoch_tail (a partial last batch of 4 on the shared handle)
    == the reference's own Solver with --loss CCC (epoch_tail_ccc.npz)."""
    c, opt, sets, _ = epoch_case("epoch_tail")
    g = load_golden("epoch_tail_ccc")
    loaders = tuple([as_datas(b) for b in sets[k]] for k in ("train", "valid", "test")) + (768, 74, 35)
    sol = Solver(solver_opt(opt, loss="CCC"), loaders)
    sol.model.load_state_dict(oracle_params(opt, c["seed"]))
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
        assert_close(r[3]["mae"], g[f"ep{ep}_train_mae"], rt, at, f"ep{ep} train mae")
        for k, bk in zip("CFTAV", banks):
            assert_close(bk.cpu().numpy(), g[f"ep{ep}_bank_{k}"], rt, aat, f"ep{ep} bank {k}")
        for tag, ld in (("valid", sol.valid_loader), ("test", sol.test_loader)):
            e = sol.evaluate(ld, *banks)
            assert_close(e[0], g[f"ep{ep}_{tag}_loss"], rt, at, f"ep{ep} {tag} loss")
            assert_close(e[3].reshape(-1), g[f"ep{ep}_{tag}_pred"], rt, aat, f"ep{ep} {tag} predictions")
    assert draw.done()
    assert list(sol._tails) == [4] and all(e.task_loss == K["CCC"] for e in sol._tails.values())
    names = [str(n) for n in g["final_names"]]
    ps = np.array([sol.model.state_dict()[n].double().sum().item() for n in names])
    np.testing.assert_allclose(ps, g["final_psum"], rtol=1e-3, atol=0.05)


def test_main_cli_with_rmse(tmp_path):
    """`python Main.py --loss RMSE`: one epoch end to end, finite losses."""
    cmd = [sys.executable, os.path.join(ROOT, "Main.py"), "--dataset", "synthetic", "--synthetic_n", "100", "--batch_size", "16",
           "--time_len", "12", "--d_hiddens", "12-3-128=4-3-128", "--d_outs", "12-3-128=4-3-128", "--bias", "--res_project", "1-1",
           "--dropout", "0.0-0.0-0.0-0.0", "--dropout_mlp", "0.0-0.0-0.0", "--epochs_num", "1", "--stage1_n", "1", "--loss", "RMSE",
           "--task_name", "cli_rmse", "--gradient_clip", "1.5", "--learning_rate", "1e-3"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = (tmp_path / "TaskRuning" / "cli_rmse" / "Running.log").read_text()
    assert "Training complete." in log and "nan" not in log.lower()


def test_mae_unchanged_and_ccc_reproducible_in_the_deterministic_build(tmp_path):
    """Deterministic build (bit-reproducible runs): three steps at cfg1_sep with no setter call, with set_task_loss(MAE), and on a handle
    switched MAE -> MSE -> MAE before its first step leave bit-identical scalars and parameter buckets; two CCC runs are bit-identical."""
    out = tmp_path / "det.npz"
    env = dict(os.environ, PYTHONPATH=ROOT, MIMRL_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "task_loss_det_worker.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    for run in ("mae_explicit", "mae_switched"):
        for k in ("scalars", "main", "crit"):
            assert np.array_equal(d[f"{run}_{k}"], d[f"mae_default_{k}"]), (run, k)
    for k in ("scalars", "main", "crit"):
        assert np.array_equal(d[f"ccc_a_{k}"], d[f"ccc_b_{k}"]), k
    assert np.isfinite(d["ccc_a_scalars"]).all()
    assert not np.array_equal(d["ccc_a_scalars"][:, _lib.S2_TASK], d["mae_default_scalars"][:, _lib.S2_TASK])
    assert np.all(np.abs(d["ccc_a_scalars"][:, _lib.S2_TASK] - 1.0) < 1.0)          # 1 - ccc with |ccc| <= 1
