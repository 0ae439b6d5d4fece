"""-m gpu: the GRU and LSTM recurrence kernels with 2, 3 and 4 batch rows per workgroup and PARTIAL last tiles, against float64.

The persistent recurrence kernels (gru.hip, lstm.hip) give each workgroup btv batch rows (mimrl_op_recur_btv: ceil(2 B nmod / 128), 1..4).
When B % btv != 0 the padding lanes of the last tile mirror its last real row and store nothing, and rows of different lengths that share a
tile go idle at different steps.  The fixtures of the rest of the suite run btv = 1 (B = 8 / 32) or full tiles of 4 (B = 128): this file
covers the rest, each case asserting the tiling it is named for.

Operator level (one modality, both directions, mimrl_op_{gru,lstm}_{forward,backward}): lengths built per tile -- 1, T and values between
in one tile, a tile whose rows are all shorter than T (the reverse direction starts late for the whole tile), the mirrored last row of
length 1 or T -- every output NaN-filled before the launch, out / dg / h_prev and the weight, bias and input gradients built from them
against float64: the fp32 kernels against autograd of oracle.gru_direction / lstm_direction, the bf16 kernels against the rounded-operand
restatements (tests/rounded_ref.py: _GruDirQ, _LstmDirQ; the oracle itself under the identity hook, tests/test_rounded_ref.py).

Engine level (two modalities, mimrl_probe_encoders: the step's own code path with the input projections, LayerNorm / ReLU and the
weight-gradient GEMMs): every W_t / rnn_* / ln_* gradient against the rounded float64 oracle, as tests/test_gpu_fused_oracle.py does at
the fixture shapes.  Bands are 3x the measured worst error (recorded with the fused-oracle errors, tests/test_gpu_fused_oracle.py::_record,
under recurrence_tiling/ keys)."""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from mimrl_amd import _lib, synth
from mimrl_amd.engine import HipEngine
from oracle import mimrl_ref as R
from tests import rounded_ref as Q
from tests.golden.configs import make_opt
from tests.gpu_helpers import P, stream
from tests.test_gpu_fused_oracle import _record as fused_oracle_record, errs, perturbed_params

pytestmark = pytest.mark.gpu
H = 128


def _record(key, val):
    """measured errors go to the error log of tests/test_gpu_fused_oracle.py, under recurrence_tiling/ keys"""
    fused_oracle_record("recurrence_tiling/" + key, val)


@pytest.fixture(scope="module")
def lib():
    lib = _lib.load()
    _lib.check(lib.mimrl_device_check())
    return lib


def _tiling(lib, B, nmod, btv):
    """the case runs the tiling it is named for: btv rows per workgroup, a last tile with B % btv real rows"""
    got = _lib.check(lib.mimrl_op_recur_btv(B, nmod))
    assert got == btv, f"B = {B}, nmod = {nmod}: {got} rows per workgroup, the case is for {btv} (was the pick retuned?)"
    assert B % btv != 0, f"B = {B} fills every tile of {btv} rows: no partial last tile"


# ----------------------------------------------------------------------------------------------------------------------------------
# operator level
# ----------------------------------------------------------------------------------------------------------------------------------
def _lengths(B, T, btv, last, seed):
    """Per-tile lengths: tile 0 holds 1, T and values between; tile 1 only lengths < T (its reverse direction starts late for every row); the
    rest drawn; the last row -- the one the padding lanes of the partial last tile mirror -- has length ``last``."""
    g = np.random.default_rng(seed)
    lens = g.integers(1, T + 1, size=B).astype(np.int32)
    if T > 1:
        lens[:btv] = np.linspace(1, T, btv).round().astype(np.int32)
        lens[btv:2 * btv] = np.linspace(max(T - 1, 1), 1, btv).round().astype(np.int32) if btv > 1 else T - 1
        assert lens[0] == 1 and lens[btv - 1] == T and (lens[btv:2 * btv] < T).all()
    lens[B - 1] = last
    return lens


def _op_inputs(enc, B, T, lens, seed, d=20):
    G = (3 if enc == "gru" else 4) * H
    g = np.random.default_rng(seed)
    x = g.standard_normal((B, T, d))
    for b in range(B):
        x[b, lens[b]:] = 0.0
    k = 1 / math.sqrt(H)                              # nn.GRU / nn.LSTM initialisation
    W = {f"{n}_{s}": g.uniform(-k, k, size=sh) for s in "fr" for n, sh in (("wih", (G, d)), ("whh", (G, H)), ("bih", (G,)), ("bhh", (G,)))}
    dout = g.standard_normal((B, T, 2 * H))           # a different upstream gradient per direction
    return x, W, dout


def _run_op(lib, enc, kernel, x, lens, W, dout):
    """forward + BPTT of one bidirectional layer on the device; gx hoisted on the host in float64 -> (out, {dir: (dg, hp)}) float64"""
    B, T, _ = x.shape
    G = (3 if enc == "gru" else 4) * H
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()
    gx = {s: f32((x @ W["wih_" + s].T + W["bih_" + s]).reshape(B, T, G)) for s in "fr"}
    Wd = {k: f32(v) for k, v in W.items()}
    lens_d = torch.from_numpy(lens).cuda()
    nan = lambda *sh: torch.full(sh, float("nan"), device="cuda")
    out = nan(B, T, 2 * H)
    if enc == "gru":
        nsv = lib.mimrl_op_gru_saved_floats(B, T)
        fwd, bwd = lib.mimrl_op_gru_forward, lib.mimrl_op_gru_backward
    else:
        nsv = B * T * 6 * H
        fwd, bwd = lib.mimrl_op_lstm_forward, lib.mimrl_op_lstm_backward
    sv = {s: torch.zeros(nsv, device="cuda") for s in "fr"}
    _lib.check(fwd(stream(), P(gx["f"]), P(gx["r"]), P(Wd["whh_f"]), P(Wd["whh_r"]), P(Wd["bhh_f"]), P(Wd["bhh_r"]), P(lens_d), P(out),
                   P(sv["f"]), P(sv["r"]), B, T, kernel))
    dg = {s: nan(B, T, 4 * H) for s in "fr"}
    hp = {s: nan(B, T, H) for s in "fr"}
    do = f32(dout)
    _lib.check(bwd(stream(), P(Wd["whh_f"]), P(Wd["whh_r"]), P(sv["f"]), P(sv["r"]), P(lens_d), P(out), P(do), P(dg["f"]), P(dg["r"]),
                   P(hp["f"]), P(hp["r"]), B, T, kernel))
    torch.cuda.synchronize()
    c = lambda t: t.cpu().double().numpy()
    return c(out), {s: (c(dg[s]), c(hp[s])) for s in "fr"}


def _grads(enc, x, W, bptt):
    """the layer's parameter and input gradients from the BPTT outputs (the engine's weight-gradient products, in float64):
    GRU dg = [dr'|dz'|dn'|dn'*r] (d gx = columns 0..3H, d(h W_hh^T + b_hh) = [dr'|dz'|dn'*r]); LSTM dg = d gx = d(h W_hh^T + b_hh)"""
    B, T, d = x.shape
    xr = x.reshape(B * T, d)
    out, dx = {}, 0.0
    for s, (dg, hp) in bptt.items():
        dg = dg.reshape(B * T, 4 * H)
        if enc == "gru":
            dgx, dgh = dg[:, :3 * H], np.concatenate([dg[:, :2 * H], dg[:, 3 * H:]], 1)
        else:
            dgx = dgh = dg
        out[f"dW_ih_{s}"], out[f"db_ih_{s}"] = dgx.T @ xr, dgx.sum(0)
        out[f"dW_hh_{s}"], out[f"db_hh_{s}"] = dgh.T @ hp.reshape(B * T, H), dgh.sum(0)
        dx = dx + dgx @ W["wih_" + s]
    out["dx"] = dx.reshape(B, T, d)
    return out


def _oracle_grads(enc, x, lens, W, dout):
    """float64 autograd of oracle.gru_direction / lstm_direction, both directions -> (out, gradients named as _grads)"""
    fn = R.gru_direction if enc == "gru" else R.lstm_direction
    xt = torch.from_numpy(x).requires_grad_(True)
    Wt = {k: torch.from_numpy(v).requires_grad_(True) for k, v in W.items()}
    lt = torch.from_numpy(lens.astype(np.int64))
    o = torch.cat([fn(xt, lt, Wt["wih_" + s], Wt["whh_" + s], Wt["bih_" + s], Wt["bhh_" + s], s == "r") for s in "fr"], -1)
    (o * torch.from_numpy(dout)).sum().backward()
    g = {"dx": xt.grad.numpy()}
    for s in "fr":
        g.update({f"dW_ih_{s}": Wt["wih_" + s].grad.numpy(), f"db_ih_{s}": Wt["bih_" + s].grad.numpy(),
                  f"dW_hh_{s}": Wt["whh_" + s].grad.numpy(), f"db_hh_{s}": Wt["bhh_" + s].grad.numpy()})
    return o.detach().numpy(), g


def _restated(enc, x, lens, W, dout, rq):
    """the hand-written restatement of the kernels (rounded_ref) with hook ``rq`` -> (out, {dir: (dg, hp)}) from its tape"""
    B, T, _ = x.shape
    lt = torch.from_numpy(lens.astype(np.int64))
    outs, bptt = [], {}
    for s, h0 in (("f", 0), ("r", H)):
        gx = torch.from_numpy(x @ W["wih_" + s].T + W["bih_" + s]).requires_grad_(True)
        tape = {}
        whh, bhh = torch.from_numpy(W["whh_" + s]), torch.from_numpy(W["bhh_" + s])
        if enc == "gru":
            o = Q._GruDirQ.apply(gx, whh, bhh, lt, s == "r", rq, Q.identity, Q.identity, tape)
        else:
            o = Q._LstmDirQ.apply(gx, whh, bhh, lt, s == "r", rq, tape)
        o.backward(torch.from_numpy(dout[..., h0:h0 + H]))
        outs.append(o.detach().numpy())
        bptt[s] = (tape["dg"].numpy(), tape["hp"].numpy())
    return np.concatenate(outs, -1), bptt


# (B, T, last-row length, rows per workgroup): btv 2 / 3 / 4 with tails of 1 / 2 / 3 rows; odd T = 13, T = 50 and T = 1
OPS = [(67, 13, 1, 2), (131, 13, "T", 3), (199, 13, 1, 4), (67, 50, "T", 2), (199, 50, 1, 4), (131, 1, 1, 3)]
# (encoder, kernel): GRU precision bit 0 = bf16; LSTM 0 scalar fp32, 1 fp32 MFMA, 2 bf16 MFMA
KERNELS = [("gru", 0), ("gru", 1), ("lstm", 0), ("lstm", 1), ("lstm", 2)]
BF16 = {("gru", 1), ("lstm", 2)}
# bands: max |error| / max |reference| of a tensor, 3x the worst error measured over OPS on the MI355X, for (out and h_prev, dg, the weight /
# bias / input gradients).  fp32: every kernel against float64 autograd of the oracle (worst 9.3e-7, dg of the GRU at T = 50) and the exact
# restatement.  bf16: against the rounded-operand restatement -- LSTM worst 1.5e-4 (its error against the un-rounded oracle: 9.3e-4);
# GRU out / h_prev 2.1e-4, gradients 5.2e-4 (vs the un-rounded oracle: 2.7e-3), and dg element by element 4.0e-3: gru.hip saves the
# gates ROUNDED to bf16 for the BPTT, and where the kernel's fp32 gate and the float64 one straddle a bf16 rounding midpoint the saved
# values differ by one bf16 ulp (2^-8 relative) -- amplified in dz = dh (h_prev - n) where h_prev ~ n.  The sums over B x T rows that the
# gradients are average those flips out.
OP_TOL = {"fp32": (3e-6, 3e-6, 3e-6), "lstm-bf16": (4.5e-4, 4.5e-4, 4.5e-4), "gru-bf16": (6.5e-4, 1.2e-2, 1.6e-3)}


@pytest.mark.parametrize("enc,kernel", KERNELS, ids=[f"{e}-{'bf16' if (e, k) in BF16 else ('scalar' if e == 'lstm' and k == 0 else 'fp32')}" for e, k in KERNELS])
@pytest.mark.parametrize("B,T,last,btv", OPS, ids=[f"B{b}-T{t}-last{l}-btv{v}" for b, t, l, v in OPS])
def test_recurrence_op_partial_tiles(lib, enc, kernel, B, T, last, btv):
    _tiling(lib, B, 1, btv)
    last = T if last == "T" else last
    lens = _lengths(B, T, btv, last, seed=B + T)
    x, W, dout = _op_inputs(enc, B, T, lens, seed=7 * B + T)
    out, bptt = _run_op(lib, enc, kernel, x, lens, W, dout)
    assert np.isfinite(out).all(), "forward: positions nobody wrote"
    for s, (dg, hp) in bptt.items():
        assert np.isfinite(dg).all() and np.isfinite(hp).all(), f"BPTT {s}: positions nobody wrote"
    bf16 = (enc, kernel) in BF16
    o_ref, g_ref = _oracle_grads(enc, x, lens, W, dout)
    r_out, r_bptt = _restated(enc, x, lens, W, dout, Q.r_bf16 if bf16 else Q.identity)
    got = {"out": out, **{f"{k}_{s}": v for s, pair in bptt.items() for k, v in zip(("dg", "hp"), pair)}, **_grads(enc, x, W, bptt)}
    restated = {"out": r_out, **{f"{k}_{s}": v for s, pair in r_bptt.items() for k, v in zip(("dg", "hp"), pair)}, **_grads(enc, x, W, r_bptt)}
    oracle = {"out": o_ref, **g_ref}
    key = f"op/{enc}-{'bf16' if bf16 else ('scalar' if enc == 'lstm' and kernel == 0 else 'fp32')}/B{B}-T{T}-last{last}-btv{btv}"
    rec = {n: {"vs_reference": errs(got[n], restated[n])["max_rel_scale"],
               "vs_unrounded_oracle": errs(got[n], oracle[n])["max_rel_scale"] if n in oracle else None} for n in got}
    _record(key, rec)
    bands = OP_TOL[f"{enc}-bf16" if bf16 else "fp32"]
    tol = {n: bands[0] if n in ("out", "hp_f", "hp_r") else bands[1] if n.startswith("dg") else bands[2] for n in rec}
    bad = {n: e["vs_reference"] for n, e in rec.items() if e["vs_reference"] > tol[n]}
    if not bf16:    # the fp32 kernels against autograd of the oracle itself too
        bad.update({f"{n} (oracle)": e["vs_unrounded_oracle"] for n, e in rec.items() if e["vs_unrounded_oracle"] is not None and e["vs_unrounded_oracle"] > tol[n]})
    assert not bad, (key, bad)


# ----------------------------------------------------------------------------------------------------------------------------------
# engine level
# ----------------------------------------------------------------------------------------------------------------------------------
def _pre_relu(p, opt, tb, rnd, rq, lstm_rnd, rec16):
    """the LayerNorm outputs in front of the encoders' ReLU (the margin filter of the upstream gradient)"""
    D = opt.d_common
    res = []
    for i, m in enumerate("av"):
        x, ln_ = tb[1 + i], R.infer_lengths(tb[1 + i])
        y = Q.bilstm1_q(p, f"rnn_{m}", x, ln_, lstm_rnd, rq) if opt.encoders == "lstm" else Q.bigru2_q(p, f"rnn_{m}", x, ln_, rnd, rq, Q.identity, rec16)
        res.append(F.layer_norm(y, (D,), p[f"ln_{m}.weight"], p[f"ln_{m}.bias"], 1e-6))
    return res


def _engine_case(enc, precision, env, B, T, btv, monkeypatch, seed=5):
    """mimrl_probe_encoders on a ragged synthetic batch against float64 autograd of the rounded oracle (tests/test_gpu_fused_oracle.py::
    _encoders_case at other shapes: perturbed biases, upstream gradient random in the cube input and the text mean, zero within 2e-3 of a
    ReLU kink)"""
    for k in env:
        monkeypatch.setenv(k, "1")
    opt = make_opt(dict(B=B, T=T, N=2 * B, seed=seed, critic="separate", cube=f"{T}-3-128=4-3-128", encoders=enc))
    t, a, v, y = synth.synthetic_batch(B, T, seed=seed, ragged=True)
    batch = tuple(torch.from_numpy(z) for z in (t, a, v, y))
    tb = tuple(z.double() for z in batch)
    lib = _lib.load()
    _tiling(lib, B, 2, btv)
    eng = HipEngine(opt, 768, 74, 35, seq_len=T, bank_capacity=2 * B, precision=precision)
    p = perturbed_params(opt, seed)
    eng.load_params(p)
    eng.set_batch(*batch)
    bf16 = precision == "bf16"
    rec16 = bf16 and enc == "gru" and os.environ.get("MIMRL_REC16", "1") != "0"
    rnd, rq, lrnd = (Q.F16_FWD, Q.r_bf16, Q.BF16) if bf16 else (Q.EXACT, Q.identity, Q.EXACT)
    g = torch.Generator().manual_seed(21)
    dcube = torch.randn(B, T, 3, 128, generator=g, dtype=torch.float64) / T
    dmean = torch.randn(3, B, 128, generator=g, dtype=torch.float64)
    with torch.no_grad():
        pre = _pre_relu(p, opt, tb, rnd, rq, lrnd, rec16)
    for i in range(2):
        dcube[:, :, 1 + i][pre[i].abs() < 2e-3] = 0.0
    dmean[1:] = 0.0
    x = eng.probe_encoders(dcube, dmean)
    torch.cuda.synchronize()
    names = [n for n in p if n.startswith(("W_t", "rnn_", "ln_a", "ln_v"))]
    assert len(names) == (37 if enc == "gru" else 21)

    def reference(rnd_, rq_, lrnd_, rec16_):
        leaves = {n: p[n].clone().requires_grad_(True) for n in names}
        xr, tf, af, vf = Q.encoders_q({**p, **leaves}, opt, tb[0], tb[1], tb[2], rnd_, rq_, rec16=rec16_, lstm_rnd=lrnd_)
        obj = (xr * dcube).sum() + (tf * dmean[0]).sum()
        return xr.detach(), torch.autograd.grad(obj, [leaves[n] for n in names])

    ref, gr = reference(rnd, rq, lrnd, rec16)
    exact, ge = reference(Q.EXACT, Q.identity, Q.EXACT, False) if bf16 else (ref, gr)
    key = f"engine/{enc}-{precision}{''.join('-' + k for k in env)}/B{B}-T{T}-btv{btv}"
    rec = {"cube_x": errs(x.cpu(), ref), "cube_x_vs_unrounded_oracle": errs(x.cpu(), exact)["max_rel_scale"]}
    worst = ("", 0.0)
    for n, gw, gx_ in zip(names, gr, ge):
        e = errs(eng.grads[n].cpu(), gw)
        e["vs_unrounded_oracle"] = errs(eng.grads[n].cpu(), gx_)["max_rel_scale"]
        rec[n] = e
        if e["max_rel_scale"] > worst[1]:
            worst = (n, e["max_rel_scale"])
    rec["worst_grad"] = worst
    _record(key, rec)
    eng.close()
    xtol, gtol = ENG_TOL[(enc, precision)]
    assert rec["cube_x"]["max_rel_scale"] <= xtol, (key, rec["cube_x"])
    bad = {n: e["max_rel_scale"] for n, e in rec.items() if isinstance(e, dict) and n in names and e["max_rel_scale"] > gtol}
    assert not bad, (key, bad)


# (cube_x, gradients) bands per (encoder, precision), max |error| / max |reference| of a tensor against the rounded float64 oracle, 3x the
# worst measured over ENG: GRU bf16 cube_x 2.1e-4 (B = 1025), gradients 3.0e-3 -- held to tests/test_gpu_fused_oracle.py's ENC_TOL, 2x --
# (against the un-rounded oracle: 9.5e-4 / 5.3e-3); LSTM bf16 1.2e-4 / 7.6e-4 (un-rounded: 3.8e-3 / 0.14 -- the LSTM path's input
# projection rounds its operands to bf16 where the GRU's uses fp16, so the un-rounded forward is 3.8e-3 away, beyond the 2e-3 margin of the
# upstream gradient: ReLU units flip between the two float64 evaluations; with a 2e-2 margin the two references differ by 3.7e-3);
# LSTM fp32 (scalar and MFMA kernels) 6.8e-7 / 4.6e-7
ENG_TOL = {("gru", "bf16"): (6.5e-4, 6e-3), ("lstm", "bf16"): (4e-4, 2.3e-3), ("lstm", "fp32"): (2e-6, 1.5e-6)}

# (encoder, precision, env, B, T, rows per workgroup): nmod = 2, btv 2 / 3 / 4 with tails of 1 / 1 / 3 rows, odd T.  The GRU bf16 cases
# run the fused layer-0 input projection (GruFwdArgs::xin_on, the default at these input widths); MIMRL_NO_XIN=1 the GEMM + gx path beside
# them.  LSTM fp32: the scalar kernels (the fp32 mode's default) and the fp32 MFMA kernels (MIMRL_LSTM_MFMA_FP32=1).  B = 1025: the wide
# batch of the per-rank ceiling with a last tile of one row.
ENG = ([("gru", "bf16", (), B, 13, v) for B, v in ((37, 2), (70, 3), (99, 4))] + [("gru", "bf16", ("MIMRL_NO_XIN",), 70, 13, 3)] +
       [("lstm", "bf16", (), B, 13, v) for B, v in ((37, 2), (70, 3), (99, 4))] +
       [("lstm", "fp32", env, B, 13, v) for env in ((), ("MIMRL_LSTM_MFMA_FP32",)) for B, v in ((37, 2), (70, 3), (99, 4))] +
       [("gru", "bf16", (), 1025, 11, 4), ("lstm", "bf16", (), 1025, 11, 4)])


@pytest.mark.parametrize("enc,precision,env,B,T,btv", ENG,
                         ids=[f"{e}-{pr}{''.join('-' + k for k in env)}-B{b}-T{t}" for e, pr, env, b, t, _ in ENG])
def test_encoders_partial_tiles_vs_rounded_oracle(enc, precision, env, B, T, btv, monkeypatch):
    monkeypatch.delenv("MIMRL_LSTM_SCALAR", raising=False)
    _engine_case(enc, precision, env, B, T, btv, monkeypatch)
