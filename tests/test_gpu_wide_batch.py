"""-m gpu: per-rank batches above 1024 rows (up to MIMRL_MAX_BATCH = 2048) -- the wide InfoNCE row kernel and the dynamic-LDS bound
kernel at op level against float64 autograd of the oracle's bounds, a full fp32 two-stage step at B = 2048 against the oracle, bf16 and
graph modes, the deterministic build and Main.py with a ragged last batch above 1024."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mimrl_amd import _lib, synth
from mimrl_amd.engine import HipEngine
from oracle import mimrl_ref as R
from tests.golden.configs import make_opt
from tests.gpu_helpers import P, assert_close, dev, grad_close, oracle_raw_grads, stream
from tests.helpers import oracle_params

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

pytestmark = pytest.mark.gpu

WIDE = [1025, 1536, 2048]


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


def _scores(seed, E, B, scale=1.5):
    return (np.random.default_rng(seed).standard_normal((E, B, B)) * scale).astype(np.float32)


@pytest.mark.parametrize("bound", [b for b in _lib.BOUNDS if b != "mine"])
@pytest.mark.parametrize("B", WIDE)
def test_wide_bounds_value_and_gradient(lib, bound, B):
    E = 2
    s = _scores(40 + B, E, B)
    gs = np.array([-1.0, 0.5], np.float32)
    S, dS, mi, GS = dev(s), torch.zeros(E, B, B, device="cuda"), torch.zeros(E, device="cuda"), dev(gs)
    _lib.check(lib.mimrl_op_mi_bound(stream(), P(S), P(dS), P(mi), P(GS), E, B, _lib.BOUNDS[bound]))
    torch.cuda.synchronize()
    for e in range(E):
        st = torch.from_numpy(s[e]).double().requires_grad_(True)
        val = R.BOUNDS[bound](st)
        (val * float(gs[e])).backward()
        assert_close(mi[e].item(), val.item(), 1e-4, 2e-5, f"{bound} value B={B}")
        grad_close(dS[e].cpu().numpy(), st.grad.numpy(), 1e-3, f"{bound} gradient B={B}")


@pytest.mark.parametrize("B", WIDE)
def test_wide_mine_bound_both_gradient_forms(lib, B):
    E = 2
    s = _scores(60 + B, E, B, 1.2)
    coef = np.array([1.0, 0.5], np.float32)
    S, dS, GS = dev(s), torch.zeros(E, B, B, device="cuda"), dev(-coef)
    mi, ml = torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")
    _lib.check(lib.mimrl_op_mi_bound_ex(stream(), P(S), P(dS), P(mi), P(ml), P(GS), E, B, _lib.BOUNDS["mine"], 0b01))
    torch.cuda.synchronize()
    for e in range(E):
        st = torch.from_numpy(s[e]).double().requires_grad_(True)
        t = st.diag()
        et = torch.exp(st) * (1.0 - torch.eye(B, dtype=st.dtype))
        val = t.mean() - R._logmeanexp_nodiag(st)
        loss = t.mean() - (1 / (0.99 + 0.01 * et.mean())).detach() * et.mean()
        lossform = bool((0b01 >> e) & 1)
        (float(coef[e]) * (loss if lossform else -val)).backward()
        assert_close(mi[e].item(), val.item(), 1e-4, 2e-5, "mine value")
        assert_close(ml[e].item(), (loss if lossform else -val).item(), 1e-4, 2e-5, "mine loss term")
        grad_close(dS[e].cpu().numpy(), st.grad.numpy(), 1e-3, f"mine gradient (lossform={lossform})")


@pytest.mark.parametrize("bound", ["tuba", "interpolate"])
@pytest.mark.parametrize("B", WIDE)
def test_wide_bounds_with_log_baseline(lib, bound, B):
    """The Gaussian and unnormalized baselines reach the bound as a per-row log a(y_i): value, d/dscores and d/dbaseline."""
    g = np.random.default_rng(80 + B)
    E = 2
    s = (g.standard_normal((E, B, B)) * 1.2).astype(np.float32)
    lbv = (g.standard_normal((E, B)) * 0.7 - 0.3).astype(np.float32)
    gs = np.array([-1.0, 0.5], np.float32)
    S, dS, GS = dev(s), torch.zeros(E, B, B, device="cuda"), dev(gs)
    LB, dLB, mi = dev(lbv), torch.zeros(E, B, device="cuda"), torch.zeros(E, device="cuda")
    _lib.check(lib.mimrl_op_mi_bound_baseline(stream(), P(S), P(dS), P(mi), P(GS), P(LB), P(dLB), E, B, _lib.BOUNDS[bound]))
    torch.cuda.synchronize()
    for e in range(E):
        st = torch.from_numpy(s[e]).double().requires_grad_(True)
        lt = torch.from_numpy(lbv[e]).double().reshape(B, 1).requires_grad_(True)
        val = R.BOUNDS[bound](st, lt)
        (val * float(gs[e])).backward()
        assert_close(mi[e].item(), val.item(), 1e-4, 2e-5, f"{bound} value B={B}")
        grad_close(dS[e].cpu().numpy(), st.grad.numpy(), 1e-3, f"{bound} d/dscores B={B}")
        grad_close(dLB[e].cpu().numpy(), lt.grad.numpy().reshape(-1), 1e-3, f"{bound} d/dbaseline B={B}")


@pytest.mark.parametrize("B", [1000] + WIDE)
def test_infonce_rows_kernel(lib, B):
    """The engine's row-tiled InfoNCE kernel (16 values per lane up to 1024, 32 above) through mimrl_op_mi_infonce_rows: value, loss term
    and gradient vs float64 autograd; a second call on the same workspace (the tickets reset themselves) gives bit-identical results."""
    E = 5
    s = _scores(100 + B, E, B, 2.0)
    gs = np.array([-1.0, 0.5, -0.01, 2.0, -0.3], np.float32)
    S, GS = dev(s), dev(gs)
    ws = torch.zeros(_lib.NCE_WS_FLOATS, device="cuda")
    outs = []
    for _ in range(2):
        dS, mi, ml = torch.full((E, B, B), float("nan"), device="cuda"), torch.zeros(E, device="cuda"), torch.zeros(E, device="cuda")
        _lib.check(lib.mimrl_op_mi_infonce_rows(stream(), P(S), P(dS), P(mi), P(ml), P(GS), E, B, P(ws)))
        torch.cuda.synchronize()
        outs.append((mi.cpu().numpy(), ml.cpu().numpy(), dS.cpu().numpy()))
    assert not ws[:16].view(torch.int32).any().item(), "ticket counters not reset"
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    mi, ml, dS = outs[0]
    for e in range(E):
        st = torch.from_numpy(s[e]).double().requires_grad_(True)
        val = R.infonce_lower_bound(st)
        (val * float(gs[e])).backward()
        assert_close(mi[e], val.item(), 1e-4, 2e-5, f"infonce value B={B}")
        assert ml[e] == -mi[e]
        grad_close(dS[e], st.grad.numpy(), 1e-3, f"infonce gradient B={B}")


# B = 2048 with small T and feature dims, so the CPU oracle stays in seconds
WIDE_CASE = dict(B=2048, T=6, N=1400, seed=31, critic="separate", cube="6-3-128=4-3-128")


def _wide_case(dtype=torch.float32, **kw):
    c = dict(WIDE_CASE, **kw)
    opt = make_opt(c)
    t, a, v, y = synth.synthetic_batch(c["B"], c["T"], seed=c["seed"], ragged=True)
    banks = synth.synthetic_banks(c["N"], seed=c["seed"])
    batch = tuple(torch.from_numpy(x).to(dtype) for x in (t, a, v, y))
    banks = {k: torch.from_numpy(val).to(dtype) for k, val in banks.items()}
    rng = np.random.default_rng(c["seed"])
    m = c["B"] // opt.k_neighbor
    anchors = [np.stack([rng.choice(c["N"], size=m, replace=False) for _ in range(6)]) for _ in range(2)]
    return c, opt, batch, banks, anchors


def _engine(c, opt, batch, banks, precision="fp32", use_graph=False):
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision=precision, use_graph=use_graph)
    p = oracle_params(opt, c["seed"])
    eng.load_params(p)
    eng.set_batch(*batch)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    return eng, p


def test_two_stage_step_at_2048_vs_oracle():
    """fp32, separable critic, B = 2048, host-provided kNN anchors: the 11 stage-1 and 8 stage-2 MI/CMI values, both stage losses, the
    task loss and every critic and main gradient tensor against the oracle's autograd."""
    c, opt, batch, banks, anchors = _wide_case()
    eng, p = _engine(c, opt, batch, banks)
    crit = [n for n in p if R.is_critic_param(n)]
    main = [n for n in p if not R.is_critic_param(n)]
    adam_v = R.AdamState(p, crit)
    for stage, names in ((1, crit), (2, main)):
        eng.set_anchors(stage, anchors[stage - 1])
        eng.stage_grads(stage)
        torch.cuda.synchronize()
        s = eng.read_scalars()
        loss, mis, pred, feats, task, grads = oracle_raw_grads(p, opt, stage, batch, banks, anchors[stage - 1], names)
        if stage == 1:
            assert_close(s[_lib.S1_LOSS], loss.item(), 1e-3, 1e-5, "stage-1 loss")
            assert_close(s[_lib.S1_MIS:_lib.S1_MIS + 11], [m.item() for m in mis], 1e-3, 2e-5, "stage-1 MI/CMI")
        else:
            assert_close(s[_lib.S2_LOSS], loss.item(), 1e-3, 1e-5, "stage-2 loss")
            assert_close(s[_lib.S2_TASK], task.item(), 1e-3, 1e-6, "task loss")
            assert_close(s[_lib.S2_MIS:_lib.S2_MIS + 8], [m.item() for m in mis], 1e-3, 5e-5, "stage-2 MI terms")
        bad = []
        for n in names:
            try:
                grad_close(eng.grads[n].cpu().numpy(), grads[n].numpy(), 3e-3, n)
            except AssertionError as e:
                bad.append(str(e))
        assert not bad, f"stage {stage}: {len(bad)}/{len(names)} gradient tensors off:\n" + "\n".join(bad[:12])
        if stage == 1:
            eng.stage_apply(1)
            clip = float(opt.gradient_clip)
            adam_v.step(p, {n: grads[n].clamp(-clip, clip) for n in crit}, float(opt.learning_rate) * float(opt.mi_lr_rate),
                        float(opt.weight_decay))
            dp = max((eng.params[n].cpu() - p[n]).abs().max().item() for n in crit)
            assert dp <= 2.5 * float(opt.learning_rate), f"critic update differs by {dp}"
            eng.load_params({n: p[n] for n in crit}, strict=False)
    eng.close()


@pytest.mark.parametrize("bound", ["nwj", "interpolate"])
def test_stage1_above_1024_other_bounds_vs_oracle(bound):
    """The dynamic-LDS bound kernel inside a step: stage-1 MI/CMI values and critic gradients at B = 1536."""
    c, opt, batch, banks, anchors = _wide_case(bound=bound, B=1536)
    eng, p = _engine(c, opt, batch, banks)
    crit = [n for n in p if R.is_critic_param(n)]
    eng.set_anchors(1, anchors[0])
    eng.stage_grads(1)
    torch.cuda.synchronize()
    s = eng.read_scalars()
    loss, mis, pred, feats, task, grads = oracle_raw_grads(p, opt, 1, batch, banks, anchors[0], crit)
    assert_close(s[_lib.S1_LOSS], loss.item(), 1e-3, 1e-5, "stage-1 loss")
    assert_close(s[_lib.S1_MIS:_lib.S1_MIS + 11], [m.item() for m in mis], 1e-3, 2e-5, "stage-1 MI/CMI")
    for n in crit:
        grad_close(eng.grads[n].cpu().numpy(), grads[n].numpy(), 3e-3, n)
    eng.close()


def _steps(eng, anchors, n=2):
    out = []
    for _ in range(n):
        eng.set_anchors(1, anchors[0])
        eng.set_anchors(2, anchors[1])
        eng.step()
        torch.cuda.synchronize()
        out.append(eng.read_scalars().copy())
    return np.stack(out)


def test_bf16_and_graph_modes_at_2048():
    """bf16 mode at B = 2048 tracks the fp32 engine (losses, MI values, cosine of both gradient buckets); the captured bf16 step agrees
    with the eager bf16 step (bit-equality is the deterministic build's test: float atomics reorder additions here)."""
    c, opt, batch, banks, anchors = _wide_case()
    res = {}
    for mode, prec, graph in (("fp32", "fp32", False), ("bf16", "bf16", False), ("bf16g", "bf16", True)):
        eng, p = _engine(c, opt, batch, banks, precision=prec, use_graph=graph)
        eng.set_anchors(1, anchors[0])
        eng.stage_grads(1)
        g1 = eng.bucket_grad(1).double().cpu().clone()
        eng.set_anchors(2, anchors[1])
        eng.stage_grads(2)
        g2 = eng.bucket_grad(2).double().cpu().clone()
        eng.close()
        eng, p = _engine(c, opt, batch, banks, precision=prec, use_graph=graph)
        res[mode] = (_steps(eng, anchors), g1, g2)
        eng.close()
    f, b, bg = res["fp32"], res["bf16"], res["bf16g"]
    for i in (_lib.S1_LOSS, _lib.S2_LOSS, _lib.S2_TASK):
        assert_close(b[0][:, i], f[0][:, i], 3e-2, 2e-3, f"bf16 scalar {i}")
    # (the first step only: after one Adam update the two modes differ by the sign-flip noise of near-zero gradients)
    assert_close(b[0][0, _lib.S2_MIS:_lib.S2_MIS + 8], f[0][0, _lib.S2_MIS:_lib.S2_MIS + 8], 3e-2, 3e-3, "bf16 stage-2 MI")
    # critic bucket: measured 0.99997 at B = 2048.  Main bucket: this small-T shape's task gradient cancels over large batches and bf16
    # forward rounding moves what is left -- measured 0.986 / 0.773 / 0.928 / 0.857 at B = 256 / 1024 / 1025 / 2048, the same order at
    # B <= 1024, where no kernel of the wide path runs
    for k, lim in ((1, 0.999), (2, 0.75)):
        cos = torch.nn.functional.cosine_similarity(b[k], f[k], dim=0).item()
        assert cos > lim, f"bucket {k} cosine {cos}"
    assert np.isfinite(bg[0]).all()
    # first step tight; the second follows an Adam update, where float atomics move near-zero gradients across their sign
    assert_close(bg[0][0], b[0][0], 1e-4, 1e-5, "captured vs eager bf16 scalars, step 1")
    assert_close(bg[0][1], b[0][1], 1e-2, 1e-3, "captured vs eager bf16 scalars, step 2")


def test_deterministic_build_at_2048_is_bit_exact(tmp_path):
    """Deterministic build at B = 2048: two captured runs and an eager run leave bit-identical scalars and parameter buckets."""
    out = tmp_path / "wide_det.npz"
    env = dict(os.environ, PYTHONPATH=ROOT, MIMRL_DETERMINISTIC="1")
    r = subprocess.run([sys.executable, os.path.join(HERE, "wide_batch_det_worker.py"), str(out)], env=env, capture_output=True, text=True,
                       timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = np.load(out)
    assert np.isfinite(d["graph_a_scalars"]).all()
    for run in ("graph_b", "eager"):
        for k in ("scalars", "main", "crit"):
            assert np.array_equal(d[f"{run}_{k}"], d[f"graph_a_{k}"]), (run, k)


def test_main_cli_batch_2048_with_ragged_tail(tmp_path):
    """`python Main.py --batch_size 2048` over 3100 rows: a full batch and a ragged last batch of 1052 rows (the sibling handle), end to
    end, finite losses."""
    cmd = [sys.executable, os.path.join(ROOT, "Main.py"), "--dataset", "synthetic", "--synthetic_n", "3100", "--batch_size", "2048",
           "--time_len", "6", "--d_hiddens", "6-3-128=4-3-128", "--d_outs", "6-3-128=4-3-128", "--bias", "--res_project", "1-1",
           "--dropout", "0.0-0.0-0.0-0.0", "--dropout_mlp", "0.0-0.0-0.0", "--epochs_num", "1", "--stage1_n", "1",
           "--task_name", "cli_wide", "--gradient_clip", "1.5", "--learning_rate", "1e-3"]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    log = (tmp_path / "TaskRuning" / "cli_wide" / "Running.log").read_text()
    assert "Training complete." in log and "nan" not in log.lower()
