"""-m gpu: --activate relu | tanh | elu | leakyrelu | hardtanh (gelu as the control) through every CubeMLP kernel family against the oracle.

No other test runs an activation but gelu, so the generic branch of act_dispatch (csrc/common.h: everything that is not gelu, relu and tanh
included) is held to the oracle here: the fused bf16 block kernels and the bf16 GEMM chain against the rounded-operand
float64 oracle (tests/rounded_ref.py), the fp32 engine against the un-rounded one, the long-sequence L-axis kernels, the ln_first chain, the
whole two-stage step (eager and captured), the forward tail's bookends and the deterministic build.

Test points.  A piecewise activation cannot be compared where a pre-activation sits on a kink: at tiny_odd with the portable initialisation
the nearest of the 152,064 CubeMLP pre-activations lies 1.4e-6 from one, inside fp32 forward noise, and a unit whose piece differs between
kernel and oracle would read as a gradient bug.  So:
  zones   : every mlp_encoder fc1.weight x 0.05, every fc1.bias = the repeating pattern (-3, -0.5, +0.5, +3): every hidden unit sits firmly
            inside one of the four pieces (below -1, (-1, 0), (0, 1), above 1) and all four are populated.  Asserted on the oracle before
            anything is compared: nearest kink >= 0.1, every piece >= 10 % of the units.  Every activation runs here.
            And every fc2.bias in front of a LayerNorm over at most 4 entries (the K axis, a 3- or 4-row L axis) is the ramp -2 .. 2: among
            thousands of such triples some have a variance near the LayerNorm's eps by chance (4.8e-7 measured in block 0's K axis), their
            rstd ~1000 amplifies fp32 noise, and at the point without the ramp torch's own float32 autograd is 1e-3 (gelu) to 4e-3
            (leakyrelu) of a tensor's scale away from float64 -- the gelu control failed there, fp32 and fused bf16.  With the ramp the
            smallest variance is 0.8 and float32 autograd agrees with float64 to 4e-6.
  natural : perturbed_params as they are -- the smooth activations only (tanh, elu with alpha = 1 is C1 at 0, and gelu).

Tolerances are the project's: bf16 output within 6e-3 (fused) / 1e-2 (chain) of the output scale; bf16 gradients tensor_ok with TOL = 1e-2,
3 x chaos_floor at JITTER = 1e-6 and the 2 %-of-group-scale rule (test_cube_stack_vs_rounded_oracle's constants); fp32: every tensor within
2e-3 of its scale (README: the engine's gradient probe against float64 autograd).  Measured errors are recorded under activate/ by
tests/test_gpu_step.py's recorder (a copy of them: profiles/activate_errors.json)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mimrl_amd import _lib
from mimrl_amd.engine import HipEngine
from oracle import mimrl_ref as R
from tests import rounded_ref as Q
from tests.golden.configs import CONFIGS, make_opt
from tests.gpu_helpers import assert_close
from tests.helpers import case, load_golden, oracle_params
# the scaling rule and bands of tests/test_gpu_fused_oracle.py::test_cube_stack_vs_rounded_oracle
from tests.test_gpu_fused_oracle import JITTER, TOL, chaos_floor, errs, perturbed_params, tensor_ok
from tests.test_gpu_step import _record_errors

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ACTS = ["relu", "tanh", "elu", "leakyrelu", "hardtanh", "gelu"]
SMOOTH = ["tanh", "elu", "gelu"]
POINTS = [(a, "zones") for a in ACTS] + [(a, "natural") for a in SMOOTH]
FP32_TOL = 2e-3
ZONE_BIAS = (-3.0, -0.5, 0.5, 3.0)
# the smallest L that selects laxis_fwd_long_kernel and laxis_bwd_kernel<true> (il > 64 && il % 4 == 0)
LONG = dict(B=4, T=68, N=40, seed=23, critic="separate", cube="8-3-128=4-3-128")


def _record(key, val):
    """the merging recorder of tests/test_gpu_step.py (the project's file of measured step errors), keys under activate/"""
    _record_errors("activate/" + key, val)


def zones_params(p):
    """The zones point: a copy of ``p`` with every mlp_encoder fc1 moved as the module docstring says."""
    out = dict(p)
    for n, v in p.items():
        if n.startswith("mlp_encoder.") and n.endswith(".fc1.weight"):
            out[n] = v * 0.05
        elif n.startswith("mlp_encoder.") and n.endswith(".fc1.bias"):
            out[n] = torch.tensor(ZONE_BIAS, dtype=v.dtype).repeat((v.numel() + 3) // 4)[:v.numel()].reshape(v.shape).clone()
        elif n.startswith("mlp_encoder.") and n.endswith(".fc2.bias") and v.numel() <= 4:
            out[n] = torch.linspace(-2.0, 2.0, v.numel(), dtype=v.dtype)
    return out


def cube_preactivations(p, opt, x):
    """Every pre-activation of the float64 oracle's CubeMLP (R.cube_block with a recording activation), flattened."""
    seen = []
    act = R._act(opt.activate)

    def rec(u):
        seen.append(u.detach().reshape(-1))
        return act(u)
    with torch.no_grad():
        for i in range(len(opt.d_hiddens)):
            x = R.cube_block(p, f"mlp_encoder.layers_stack.{i}", x, rec, opt.ln_first, opt.res_project[i])
    return torch.cat(seen)


def assert_zones(u, key):
    """The precondition of the zones point (not a skip: these inputs meet it)."""
    near = float(torch.stack([(u - s).abs().min() for s in (-1.0, 0.0, 1.0)]).min())
    shares = [float(m.double().mean()) for m in (u < -1, (u > -1) & (u < 0), (u > 0) & (u < 1), u > 1)]
    assert near >= 0.1 and min(shares) >= 0.10, (key, near, shares)
    return {"nearest_kink": near, "zone_shares": shares, "units": int(u.numel())}


_INPUTS = {}


def probe_inputs(B, L, ol, ok):
    """the cube's input as test_cube_stack_vs_rounded_oracle draws it (O(1) entries, a non-negative half) and the random upstream gradient"""
    key = (B, L, ol, ok)
    if key not in _INPUTS:
        g = torch.Generator().manual_seed(11)
        x = torch.randn(B, L, 3, 128, generator=g, dtype=torch.float64)
        x[:, :, 1:] = torch.relu(x[:, :, 1:])
        _INPUTS[key] = (x, torch.randn(B, ol, ok, 128, generator=g, dtype=torch.float64))
    return _INPUTS[key]


def cube_long_q(p, opt, x):
    """What the kernels compute at L = 68 with blocks 8-3-128=4-3-128 (csrc/engine_forward.hip cube_forward): block 0 is too long for the
    LDS-resident block kernel -- laxis_fwd_long_kernel (every operand fp16, cube_long.hip) + the fp32 K-axis mix + the bf16 D-axis GEMMs, no
    tile rounding --, block 1 (L = 8) the fused block kernel.  Backward products bf16 throughout.  Pieces of tests/rounded_ref.py."""
    act = R._act(opt.activate)
    pre = "mlp_encoder.layers_stack.0"
    xl = x.permute(0, 2, 3, 1)
    x = Q._ln(p, f"{pre}.ln_l", Q._mlp_res(p, pre, "l", xl, xl, act, Q.F16_FWD)).permute(0, 3, 1, 2)
    xk = x.permute(0, 1, 3, 2)
    x = Q._ln(p, f"{pre}.ln_k", Q._mlp_res(p, pre, "k", xk, xk, act, Q.EXACT)).permute(0, 1, 3, 2)
    x = Q._ln(p, f"{pre}.ln_d", Q._mlp_res(p, pre, "d", x, x, act, Q.BF16))
    return Q.cube_block_q(p, "mlp_encoder.layers_stack.1", x, act, Q.F16_FWD, True, False)


def run_probe(key, c, act, point, monkeypatch, precision="bf16", env=(), ln_first=False, ref="fused", want_raw=False):
    """probe_cube (output, dx, every mlp_encoder.* gradient) against the oracle.  ref: "fused" = Q.cube_mlp_q(F16_FWD, round_tile) at 6e-3,
    "chain" = Q.cube_mlp_q(BF16) at 1e-2, "long" = cube_long_q at 1e-2 (block 0 is a chain), "exact" = R.cube_mlp, every tensor at FP32_TOL."""
    for k, v in (env.items() if isinstance(env, dict) else [(k, "1") for k in env]):
        monkeypatch.setenv(k, v)
    opt = make_opt(c)
    opt.activate, opt.ln_first = act, bool(ln_first)
    p = perturbed_params(opt, c["seed"])
    if point == "zones":
        p = zones_params(p)
    B, L = c["B"], opt.time_len
    ol, ok = opt.d_outs[-1][0], opt.d_outs[-1][1]
    x, dout = probe_inputs(B, L, ol, ok)
    rec = {}
    if point == "zones":
        rec["zones"] = assert_zones(cube_preactivations(p, opt, x), key)
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision=precision)
    eng.load_params(p)
    out, dx = eng.probe_cube(x, dout)
    torch.cuda.synchronize()
    got = {"out": out.double().cpu(), "dx": dx.double().cpu(), **{n: v.double().cpu().clone() for n, v in eng.grads.items() if n.startswith("mlp_encoder.")}}
    eng.close()
    for k in env:
        monkeypatch.delenv(k, raising=False)
    names = [n for n in p if n.startswith("mlp_encoder.")]
    g = torch.Generator().manual_seed(12)

    def reference(jitter=0.0):
        leaves = {n: (p[n] + jitter * torch.randn(p[n].shape, generator=g, dtype=torch.float64) if n.endswith(".bias") else p[n].clone()).requires_grad_(True)
                  for n in names}
        xr = x.clone().requires_grad_(True)
        pp = {**p, **leaves}
        if ref == "exact":
            o = R.cube_mlp(pp, opt, xr)
        elif ref == "long":
            o = cube_long_q(pp, opt, xr)
        else:
            o = Q.cube_mlp_q(pp, opt, xr, Q.F16_FWD if ref == "fused" else Q.BF16, round_tile=ref == "fused")
        return o.detach(), torch.autograd.grad((o * dout).sum(), [xr] + [leaves[n] for n in names])

    want, gr = reference()
    if ref == "exact":
        chaos = {n: 0.0 for n in ["dx"] + names}            # the float64 oracle rounds nothing: no chaos band
    else:
        chaos = dict(zip(["dx"] + names, chaos_floor(gr, reference(JITTER)[1])))
    rec["out"] = errs(got["out"], want)
    worst = ("", 0.0)
    for n, gw in zip(["dx"] + names, gr):
        e = errs(got[n], gw)
        e["chaos"] = chaos[n]
        rec[n] = e
        if e["max_rel_scale"] > worst[1]:
            worst = (n, e["max_rel_scale"])
    rec["worst_grad"] = worst
    _record(key, {"out": rec["out"]["max_rel_scale"], "worst_grad": worst, **({"zones": rec["zones"]} if "zones" in rec else {}),
                  "max_rel_scale, chaos": {n: [float("%.3g" % rec[n]["max_rel_scale"]), float("%.3g" % rec[n]["chaos"])] for n in ["dx"] + names}})
    print(key, "out", rec["out"]["max_rel_scale"], "worst grad", worst)
    assert all(torch.isfinite(v).all() for v in got.values()), key
    out_tol = {"fused": 6e-3, "chain": 1e-2, "long": 1e-2, "exact": FP32_TOL}[ref]
    tol = FP32_TOL if ref == "exact" else TOL
    assert rec["out"]["max_rel_scale"] <= out_tol, (key, rec["out"])
    gs = max(rec[n]["scale"] for n in names)
    bad = {n: rec[n] for n in ["dx"] + names if not tensor_ok(rec[n], tol, gs if n != "dx" else rec[n]["scale"], rec[n]["chaos"])}
    assert not bad, (key, {n: (e["max_rel_scale"], e["l2_rel"], e["chaos"]) for n, e in bad.items()})
    return got if want_raw else None


@pytest.mark.parametrize("act,point", POINTS, ids=[f"{a}-{p}" for a, p in POINTS])
def test_bf16_fused_kernels(act, point, monkeypatch):
    """tiny_odd (B = 12, L = 8 zero-padded tile, blocks 8-3-128=3-3-128): cube_fwd_fused_kernel, laxis / daxis_bwd_kernel, kmix_bwd_kernel
    with a padded tile and a partial batch tile."""
    run_probe(f"fused/tiny_odd/{act}/{point}", CONFIGS["tiny_odd"], act, point, monkeypatch, ref="fused")


@pytest.mark.parametrize("act,point", POINTS, ids=[f"{a}-{p}" for a, p in POINTS])
def test_bf16_gemm_chain(act, point, monkeypatch):
    """The same fixture as the unfused bf16 chain: the GEMM epilogues' act_apply and their gradact_u / act_grad path (csrc/gemm.hip), the
    stand-alone K-axis kernels."""
    run_probe(f"chain/tiny_odd/{act}/{point}", CONFIGS["tiny_odd"], act, point, monkeypatch,
              env=("MIMRL_NO_FUSED_CUBE", "MIMRL_NO_FUSED_CUBE_BWD"), ref="chain")


@pytest.mark.parametrize("act", ["elu", "hardtanh", "gelu"])
def test_ln_first_chain(act, monkeypatch):
    """forward_ln_first (MLPProcess.py:64-92) only exists as the bf16 chain; at cfg1_sep's shape (at L = 6 / 4 its bf16 gradients are noise:
    tests/test_gpu_fused_oracle.py)."""
    run_probe(f"chain-ln_first/cfg1_sep/{act}/zones", CONFIGS["cfg1_sep"], act, "zones", monkeypatch, ln_first=True, ref="chain")


@pytest.mark.parametrize("act", ["elu", "hardtanh", "gelu"])
def test_long_l_axis_kernels(act, monkeypatch):
    """time_len = 68, B = 4: laxis_fwd_long_kernel and laxis_bwd_kernel<true>.  They ran: with MIMRL_LAXIS_LONG=0 the output, with
    MIMRL_LAXIS_BWD_LONG=0 the backward's results are other numbers (as the long-sequence tests of tests/test_gpu_fused_oracle.py prove it.
    Those compare dx alone, at 50 hidden rows; with this shape's 8 rows both paths sum dx's eight products in one MFMA step and can agree bit
    for bit -- hardtanh and gelu did --, so here: dx or any parameter gradient, e.g. the bias gradients the long kernel sums itself)."""
    long_ = run_probe(f"long/L68/{act}/zones", LONG, act, "zones", monkeypatch, ref="long", want_raw=True)
    for knob in ("MIMRL_LAXIS_LONG", "MIMRL_LAXIS_BWD_LONG"):
        monkeypatch.setenv(knob, "0")
        opt = make_opt(LONG)
        opt.activate = act
        eng = HipEngine(opt, 768, 74, 35, seq_len=LONG["T"], bank_capacity=LONG["N"], precision="bf16")
        eng.load_params(zones_params(perturbed_params(opt, LONG["seed"])))
        out, dx = eng.probe_cube(*probe_inputs(LONG["B"], 68, 4, 3))
        torch.cuda.synchronize()
        chain = {"out": out.double().cpu(), "dx": dx.double().cpu(), **{n: v.double().cpu().clone() for n, v in eng.grads.items() if n.startswith("mlp_encoder.")}}
        eng.close()
        monkeypatch.delenv(knob)
        if knob == "MIMRL_LAXIS_LONG":
            assert not torch.equal(long_["out"], chain["out"]), f"{knob}=0 changed nothing: the long kernel did not run"
        else:
            assert torch.equal(long_["out"], chain["out"])      # (the forward is untouched by the backward's knob)
            moved = [n for n in chain if n != "out" and not torch.equal(long_[n], chain[n])]
            print(knob, "=0 moved", len(moved), "of", len(chain) - 1, "tensors")
            assert moved, f"{knob}=0 changed nothing: the long kernel did not run"


@pytest.mark.parametrize("act,point", POINTS, ids=[f"{a}-{p}" for a, p in POINTS])
def test_fp32_engine(act, point, monkeypatch):
    """precision = fp32 (the fp32 GEMM chain) against the un-rounded float64 oracle's autograd: every tensor within 2e-3 of its scale."""
    run_probe(f"fp32/tiny_odd/{act}/{point}", CONFIGS["tiny_odd"], act, point, monkeypatch, precision="fp32", ref="exact")


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("act,point", [("elu", "natural"), ("hardtanh", "zones")])
def test_two_stage_step_fp32(act, point, use_graph, monkeypatch):
    """The flag through mimrl_create, the step and the graphs: one two-stage step at tiny_sep against the oracle's, compared the way
    tests/test_gpu_step.py::test_two_stage_trajectory compares the gelu step at it = 0 (its tolerances), plus the MI / CMI values of both
    stages (test_stage_losses_and_all_gradients_vs_oracle's)."""
    c, opt, batch, banks = case("tiny_sep")
    opt.activate = act
    p = oracle_params(opt, c["seed"])
    if point == "zones":
        p = zones_params(p)
        seen = []
        real = R._act

        def recording(name):
            f = real(name)
            return lambda u: (seen.append(u.detach().reshape(-1)), f(u))[1]
        monkeypatch.setattr(R, "_act", recording)
        with torch.no_grad():
            R.model_forward({k: v.double() for k, v in p.items()}, opt, *[b.double() for b in batch[:3]])
        monkeypatch.setattr(R, "_act", real)
        _record(f"step/tiny_sep/{act}/{point}/zones", assert_zones(torch.cat(seen), "step"))
    anchors = load_golden("tiny_sep")["anchors"][0]
    eng = HipEngine(opt, 768, 74, 35, seq_len=c["T"], bank_capacity=c["N"], precision="fp32", use_graph=use_graph)
    eng.load_params(p)
    eng.set_batch(*batch)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
    eng.set_anchors(1, anchors[0])
    eng.set_anchors(2, anchors[1])
    eng.stage1_step()
    eng.stage2_step()
    torch.cuda.synchronize()
    s = eng.read_scalars().copy()
    after = {n: v.detach().double().cpu().clone() for n, v in eng.params.items()}
    eng.close()
    crit = [n for n in p if R.is_critic_param(n)]
    main = [n for n in p if not R.is_critic_param(n)]
    q = {n: v.clone() for n, v in p.items()}
    r1, r2 = R.two_stage_step(q, opt, R.AdamState(q, crit), R.AdamState(q, main), batch, banks, anchors[0], anchors[1])
    rel = lambda a, b: float(abs(a - b) / max(abs(b), 1e-30))
    rec = {"s1_loss": rel(s[_lib.S1_LOSS], r1["loss"].item()), "s2_loss": rel(s[_lib.S2_LOSS], r2["loss"].item()),
           "task": rel(s[_lib.S2_TASK], r2["task"].item()),
           "mi1": float(np.abs(s[_lib.S1_MIS:_lib.S1_MIS + 11] - np.array([m.item() for m in r1["mis"]])).max()),
           "mi2": float(np.abs(s[_lib.S2_MIS:_lib.S2_MIS + 8] - np.array([m.item() for m in r2["mis"]])).max()),
           "param_max_diff": max(float((after[n] - q[n].double()).abs().max()) for n in q),
           "param_sum_max_diff": max(abs(float(after[n].sum() - q[n].double().sum())) for n in q)}
    _record(f"step/tiny_sep/{act}/{point}/{'graph' if use_graph else 'eager'}", rec)
    print(rec)
    assert np.isfinite(s[:64]).all()
    assert_close(s[_lib.S1_LOSS], r1["loss"].item(), 1e-3, 2e-5, "stage-1 loss vs oracle")
    assert_close(s[_lib.S2_LOSS], r2["loss"].item(), 1e-3, 2e-5, "stage-2 loss vs oracle")
    assert_close(s[_lib.S2_TASK], r2["task"].item(), 1e-3, 2e-5, "task loss vs oracle")
    assert_close(s[_lib.S1_MIS:_lib.S1_MIS + 11], [m.item() for m in r1["mis"]], 1e-3, 2e-5, "stage-1 MI/CMI vs oracle")
    assert_close(s[_lib.S2_MIS:_lib.S2_MIS + 8], [m.item() for m in r2["mis"]], 1e-3, 5e-5, "stage-2 MI terms vs oracle")
    # parameters after one clip+Adam update of each bucket: per-tensor sums as test_two_stage_trajectory (a few sign flips of ~0 gradients),
    # and no entry further than 2.5 lr from the oracle's (Adam t = 1 moves every entry by at most lr: test_gpu_step.py's critic-update bound)
    names = sorted(q)
    np.testing.assert_allclose([after[n].sum().item() for n in names], [q[n].double().sum().item() for n in names], rtol=1e-4, atol=0.05)
    assert rec["param_max_diff"] <= 2.5 * float(opt.learning_rate), rec
    assert max(float((after[n] - p[n].double()).abs().max()) for n in main if n.startswith("mlp_encoder.")) > 0, "CubeMLP was not updated"


_WORKER = {}


def _worker(tmp_path_factory):
    """tests/activate_det_worker.py once, in a fresh process under MIMRL_DETERMINISTIC=1 (the library is chosen at import)."""
    if not _WORKER:
        d = tmp_path_factory.mktemp("activate")
        env = dict(os.environ, PYTHONPATH=ROOT, MIMRL_DETERMINISTIC="1")
        for name in [n for n in env if n.startswith("MIMRL_") and n != "MIMRL_DETERMINISTIC"]:
            env.pop(name)
        r = subprocess.run([sys.executable, os.path.join(HERE, "activate_det_worker.py"), str(d / "r.json")], env=env, cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        _WORKER["r"] = r
        _WORKER["res"] = json.load(open(d / "r.json")) if r.returncode == 0 and "ACTIVATE_DONE" in r.stdout else None
    r = _WORKER["r"]
    assert _WORKER["res"] is not None, r.stdout[-2000:] + r.stderr[-3000:]
    return _WORKER["res"]


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("shape", ["T5_L8_ragged", "T50_two_blocks"])
def test_bookends_bit_identical_with_elu(shape, use_graph, tmp_path_factory):
    """tests/test_gpu_cube_bookends.py's on / off comparison (block 0 builds its tile from the encoder outputs, the last block ends in the
    head, against tail_pre / head_fwd as launches of their own) with --activate elu: bit identity of every compared item."""
    case_ = _worker(tmp_path_factory)["bookends"][f"{shape}|{int(use_graph)}"]
    assert len(case_) == 8
    for k, v in case_.items():
        assert v["finite"] and v["n"] > 0 and v["absmax"] > 0, (k, v)
        assert v["equal"], f"{k}: folded vs separate launches differ by {v['maxdiff']:.3e} (scale {v['absmax']:.3e})"


def test_deterministic_build_runs_elu_bit_identically(tmp_path_factory):
    """libmimrl_hip_det.so builds the same sources: one elu probe_cube case (tiny_odd, bf16 fused kernels, zones point) twice on fresh
    engines -- output, dx and every gradient bit-identical run to run, and not the identity's numbers."""
    det = _worker(tmp_path_factory)["det"]
    assert det["deterministic"] == 1 and det["tensors"] >= 40
    assert det["finite"] and det["grad_absmax"] > 0
    assert det["differs_from_gelu"], "elu and gelu gave the same numbers: the activation code did not reach the kernels"
    assert det["equal"], det["unequal"]
