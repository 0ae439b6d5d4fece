"""-m gpu: --shuffle on the device.  mimrl_op_gather_rows against torch.index_select (bit-exact: it only moves bytes), the engine's
Rows upload (resident and pinned-host datasets, both input sets), and two epochs of Solver.train over a shuffling loader against the
same epochs over pre-gathered plain batches."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mimrl_amd import Parameters, _lib
from mimrl_amd.Solver import Solver
from mimrl_amd.data import Rows, get_data_loader
from tests.helpers import case, oracle_params

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

N_SRC = 7
SENTINEL = -12345.0
# row shapes: 16-byte rows (one partial chunk; three chunks with a partial tail), 888 B (8 bytes per lane), 420 B (4 bytes per lane),
# a label (4 B: shorter than one vector)
GROUPS = ([(12, 768), (3, 74), (3, 35), (1,)], [(4, 768), (3, 74), (3, 35), (1,)])
INDEX_SETS = ([3], [0, N_SRC - 1, 2, 2, 4], list(range(N_SRC - 1, -1, -1)))


def _offset_by_one_float(n, dev):
    """A float32 tensor of n elements that starts one float behind an aligned allocation."""
    buf = torch.empty(n + 1, dtype=torch.float32, device=dev)
    assert buf.data_ptr() % 16 == 0
    return buf[1:]


def gather(srcs, idx, max_workgroups=0, n_src=None, dst_offset=(), stream=None):
    """mimrl_op_gather_rows over ``srcs`` (device tensors [N, ...]) -> the gathered tensors; every destination lies between two runs of 64
    sentinel floats, which must come back untouched.  ``dst_offset``: positions whose destination starts one float off alignment."""
    lib = _lib.load()
    dev = srcs[0].device
    idx_t = torch.tensor(idx, dtype=torch.int32, device=dev)
    rows, n = len(idx), len(srcs)
    row = [int(s[0].numel()) for s in srcs]
    bufs, dsts = [], []
    for a in range(n):
        m = 64 + rows * row[a] + 64
        buf = _offset_by_one_float(m, dev) if a in dst_offset else torch.empty(m, dtype=torch.float32, device=dev)
        buf.fill_(SENTINEL)
        bufs.append(buf)
        dsts.append(buf[64:64 + rows * row[a]])
    s = torch.cuda.current_stream().cuda_stream if stream is None else stream
    rc = lib.mimrl_op_gather_rows(C.c_void_p(s), n, (C.c_void_p * n)(*(x.data_ptr() for x in srcs)), (C.c_void_p * n)(*(d.data_ptr() for d in dsts)),
                                  (C.c_int64 * n)(*(4 * r for r in row)), int(n_src if n_src is not None else srcs[0].shape[0]),
                                  C.c_void_p(idx_t.data_ptr()), rows, int(max_workgroups))
    _lib.check(rc)
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf[:64] == SENTINEL).all()) and bool((buf[-64:] == SENTINEL).all()), "the gather wrote outside its destination"
    return [d.reshape(rows, *srcs[a].shape[1:]) for a, d in enumerate(dsts)]


def sources(shapes, dev, seed=0, src_offset=()):
    g = torch.Generator().manual_seed(seed)
    out = []
    for a, sh in enumerate(shapes):
        x = torch.randn(N_SRC, *sh, generator=g)
        if a in src_offset:
            t = _offset_by_one_float(x.numel(), dev).view(N_SRC, *sh)
            t.copy_(x)
        else:
            t = x.to(dev)
        out.append(t)
    return out


def check_gather_exact():
    """The op-level exactness case (also run under the deterministic build by tests/shuffle_det_worker.py)."""
    dev = torch.device("cuda")
    n = 0
    for gi, shapes in enumerate(GROUPS):
        for src_off, dst_off in (((), ()), ((0, 1), ()), ((), (0, 2)), ((3,), (3,))):
            srcs = sources(shapes, dev, seed=gi, src_offset=src_off)
            assert all((s.data_ptr() % 16 == 4) == (a in src_off) for a, s in enumerate(srcs))
            for idx in INDEX_SETS:
                want = [s.index_select(0, torch.tensor(idx, device=dev)) for s in srcs]
                for mw in (1, 0):
                    got = gather(srcs, idx, mw, dst_offset=dst_off)                           # the four arrays of a batch in ONE call
                    for a in range(4):
                        assert torch.equal(got[a], want[a]), (shapes[a], idx, mw, src_off, dst_off)
                        one = gather([srcs[a]], idx, mw, dst_offset=(0,) if a in dst_off else ())[0]     # ... and one call per array
                        assert torch.equal(one, want[a]), (shapes[a], idx, mw, src_off, dst_off, "n_arrays=1")
                        n += 1
    return n


def test_gather_rows_equals_index_select():
    assert check_gather_exact() == 2 * 4 * 3 * 2 * 4


def test_gather_rows_out_of_range_rows_are_nan_and_bad_arguments_are_refused():
    dev = torch.device("cuda")
    lib = _lib.load()
    srcs = sources(GROUPS[0], dev, seed=7)
    for bad in (-1, N_SRC, 2 ** 30):
        idx = [bad, 2, bad, 0, 6]
        for mw in (1, 0):
            got = gather(srcs, idx, mw)
            for a, g in enumerate(got):
                assert bool(torch.isnan(g[0]).all()) and bool(torch.isnan(g[2]).all()), (bad, a)
                assert torch.equal(g[[1, 3, 4]], srcs[a][[2, 0, 6]]), (bad, a)
    # ... src_rows is the bound, not the allocation: rows >= src_rows of a longer array are out of range too
    got = gather(srcs, [5, 4], n_src=5)
    assert all(bool(torch.isnan(g[0]).all()) and torch.equal(g[1], s[4]) for g, s in zip(got, srcs))
    x = srcs[1]
    d = torch.empty_like(x)
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, I = lambda *p: (C.c_void_p * len(p))(*p), lambda *v: (C.c_int64 * len(v))(*v)
    ok = dict(n=1, src=P(x.data_ptr()), dst=P(d.data_ptr()), rb=I(888), idx=C.c_void_p(idx.data_ptr()), rows=4, mw=0)
    call = lambda **kw: (lambda a: lib.mimrl_op_gather_rows(s, a["n"], a["src"], a["dst"], a["rb"], N_SRC, a["idx"], a["rows"], a["mw"]))(dict(ok, **kw))
    assert call() == 0
    four = dict(src=P(*[x.data_ptr()] * 5), dst=P(*[d.data_ptr()] * 5), rb=I(*[888] * 5))
    for kw in (dict(rows=0), dict(rows=-3), dict(n=0), dict(n=5, **four), dict(src=None), dict(dst=None), dict(rb=None), dict(idx=None),
               dict(src=P(None)), dict(dst=P(None)), dict(rb=I(0)), dict(rb=I(-888)), dict(rb=I(886)), dict(rb=I(2)), dict(mw=-1),
               dict(src=P(x.data_ptr() + 2))):
        assert call(**kw) == -1, kw
        assert lib.mimrl_last_error().decode().startswith("gather_rows:"), kw
    torch.cuda.synchronize()


def test_deterministic_build_gathers_the_same_bytes():
    """The op-level exactness case once under MIMRL_DETERMINISTIC=1 (the library is chosen at import: its own process)."""
    env = dict(os.environ, MIMRL_DETERMINISTIC="1", PYTHONPATH=ROOT)
    env.pop("MIMRL_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "shuffle_det_worker.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "gather exact under the deterministic build" in r.stdout, r.stdout


@pytest.mark.parametrize("host", [False, True], ids=["resident", "pinned-host"])
def test_engine_uploads_rows_batches(host, monkeypatch):
    """stage_batch(Rows...) + commit_batch(): the bound inputs are base[idx], for a dataset in HBM (one gather launch on the upload stream)
    and in pinned host memory (host gather into the engine's staging tensors + H2D); two staged batches in a row use both input sets, a
    third reuses the first (and the staging tensors).  set_batch(Rows...) fills the bound set the same way."""
    from mimrl_amd.engine import HipEngine
    c, opt, batch, banks = case("tiny_sep")
    B, T, n = c["B"], c["T"], 3 * c["B"] + 1
    eng = HipEngine(opt, 768, 74, 35, seq_len=T, bank_capacity=c["N"])
    launches, native = [], eng.lib.mimrl_op_gather_rows
    monkeypatch.setattr(eng.lib, "mimrl_op_gather_rows", lambda *a: launches.append((a[0].value or 0, a[1])) or native(*a))
    g = torch.Generator().manual_seed(11)
    base = [torch.randn(n, T, 768, generator=g), torch.randn(n, T, 74, generator=g), torch.randn(n, T, 35, generator=g), torch.randn(n, 1, generator=g)]
    place = (lambda x: x.pin_memory()) if host else (lambda x: x.to(eng.device))
    dev = [place(x) for x in base]
    perm = torch.randperm(n, generator=g).to(torch.int32)
    bound = lambda: [x.cpu().reshape(B, -1) for x in (eng.text, eng.audio, eng.video, eng.labels)]
    seen = set()
    for i in range(3):
        idx = perm[i * B:(i + 1) * B]
        idx_d = idx if host else idx.to(eng.device)
        eng.stage_batch(*(Rows(x, idx_d) for x in dev))
        eng.commit_batch()
        torch.cuda.synchronize()
        seen.add(eng.text.data_ptr())
        for got, x in zip(bound(), base):
            assert torch.equal(got, x[idx.long()].reshape(B, -1)), (i, tuple(x.shape))
    assert len(seen) == 2
    # a resident batch is ONE launch for its four arrays, on the upload stream; a host batch launches nothing
    assert launches == ([] if host else [(eng._copy_stream.cuda_stream, 4)] * 3)
    idx = torch.arange(B - 1, -1, -1, dtype=torch.int32)
    idx_d = idx if host else idx.to(eng.device)
    eng.set_batch(*(Rows(x, idx_d) for x in dev))
    torch.cuda.synchronize()
    for got, x in zip(bound(), base):
        assert torch.equal(got, x[idx.long()].reshape(B, -1))
    assert launches[3:] == ([] if host else [(eng.stream.cuda_stream, 4)])
    # Rows that do not share ONE index tensor, or Rows beside plain tensors, are materialized and copied like tensors
    eng.set_batch(Rows(dev[0], idx_d), Rows(dev[1], idx_d.clone()), base[2][:B], Rows(dev[3], idx_d))
    torch.cuda.synchronize()
    for got, want in zip(bound(), (base[0][idx.long()], base[1][idx.long()], base[2][:B], base[3][idx.long()])):
        assert torch.equal(got, want.reshape(B, -1))
    # a batch of another size, or rows of another length, are refused before anything is launched
    short = idx_d[:B - 1]
    with pytest.raises(_lib.MimrlError):
        eng.set_batch(*(Rows(x, short) for x in dev))
    with pytest.raises(_lib.MimrlError):
        eng.set_batch(*(Rows(x, idx_d) for x in (dev[1], dev[1], dev[2], dev[3])))
    assert len(launches) == (0 if host else 4)
    eng.close()


def test_stage1_pass_takes_rows_batches():
    """HipEngine.stage1_pass (the opt-in look-ahead critic pass) over Rows batches: every step runs on base[idx] of its batch, bit for
    bit, and the pass gives the stage-1 losses of the same pass over plain device tensors (two runs of the same arithmetic: the loss band
    of test_gpu_boundary.py::test_resident_dataset_equals_host_dataset)."""
    from mimrl_amd.engine import HipEngine
    c, opt, batch, banks = case("tiny_sep")
    B, T, n = c["B"], c["T"], 3 * c["B"]
    g = torch.Generator().manual_seed(5)
    dev = torch.device("cuda")
    base = [torch.randn(n, T, 768, generator=g).to(dev), torch.randn(n, T, 74, generator=g).to(dev), torch.randn(n, T, 35, generator=g).to(dev),
            (6.0 * torch.rand(n, 1, generator=g) - 3.0).to(dev)]
    perm = torch.randperm(n, generator=g).to(torch.int32).to(dev)
    idxs = [perm[i * B:(i + 1) * B] for i in range(3)]
    out = {}
    for tag in ("rows", "tensors"):
        eng = HipEngine(opt, 768, 74, 35, seq_len=T, bank_capacity=c["N"], use_graph=True, device_anchors=True)
        eng.load_params(oracle_params(opt, c["seed"]))
        eng.set_banks(*(banks[k] for k in "CFTAV"))
        if tag == "rows":
            batches = [tuple(Rows(x, ix) for x in base) for ix in idxs]
        else:
            batches = [tuple(x.index_select(0, ix) for x in base) for ix in idxs]
        seen = []
        assert eng.stage1_pass(batches, lambda e: seen.append((e.scalars[_lib.S1_LOSS].clone(), [t.clone() for t in (e.text, e.audio, e.video, e.labels)]))) == 3
        torch.cuda.synchronize()
        for (loss, bound), ix in zip(seen, idxs):
            for got, x in zip(bound, base):
                assert torch.equal(got.reshape(B, -1), x.index_select(0, ix).reshape(B, -1)), tag
        out[tag] = np.array([float(l) for l, _ in seen])
        eng.close()
    assert np.isfinite(out["rows"]).all() and np.abs(out["rows"]).max() > 0
    np.testing.assert_allclose(out["rows"], out["tensors"], rtol=1e-5, atol=1e-7)


ARGV = ["--dataset", "synthetic", "--synthetic_n", "100", "--batch_size", "16", "--time_len", "12", "--d_hiddens", "12-3-128=4-3-128",
        "--d_outs", "12-3-128=4-3-128", "--bias", "--res_project", "1-1", "--dropout", "0.0-0.0-0.0-0.0", "--dropout_mlp", "0.0-0.0-0.0",
        "--loss_mi_coefficient1", "-".join(["1.0"] * 11), "--loss_mi_coefficient2", "-".join(["0.01"] * 8), "--learning_rate", "1e-4",
        "--task_name", "pytest_shuffle"]


def _solver(opt, loaders):
    opt.task_name, opt.seed, opt.epochs_num, opt.save_best_features = "pytest_shuffle", 0, 1, False
    opt.precision, opt.no_graph, opt.host_anchors = "fp32", False, False          # graphs on, device-drawn anchors
    sol = Solver(opt, loaders)
    sol.model.load_state_dict(oracle_params(opt, 3))
    return sol


def _two_epochs(sol, passes=None):
    """Two epochs of train + evaluate.  ``passes``: plain list loaders, one per pass in the order train() consumes them (epoch 0: the model
    pass; epoch 1: the critic pass, then the model pass)."""
    banks = ([], [], [], [], [])
    res, ck = [], None
    order = iter(passes) if passes is not None else None
    for ep in range(2):
        if order is not None:
            if ep > 0:
                sol.train_loader = next(order)
            model_pass = next(order)
        else:
            model_pass = sol.train_loader
        r = sol.train(ep, model_pass, *banks)
        banks = r[4:]
        e = sol.evaluate(sol.valid_loader, *banks)
        res.append((float(r[0]), float(r[1]), np.asarray(r[2], dtype=np.float64), float(e[0]), banks[1].cpu().numpy().copy(),
                    banks[0].cpu().numpy().copy()))
        if ep == 0:
            ck = sol.checkpoint(0)
    return res, ck


def _spy(loader):
    """Record the permutation of every pass the loader really starts."""
    seen, orig = [], loader.permutation
    def permutation(i):
        seen.append((int(i), orig(i).clone()))
        return seen[-1][1]
    loader.permutation = permutation
    return seen


@pytest.fixture(scope="module")
def shuffled_run():
    """(a): two epochs with --shuffle over the resident dataset."""
    opt = Parameters.parse_args(ARGV + ["--shuffle"])
    loaders = get_data_loader(opt)
    assert loaders[0].shuffle and loaders[0].t.is_cuda
    seen = _spy(loaders[0])
    sol = _solver(opt, loaders)
    res, ck = _two_epochs(sol)
    return dict(res=res, ck=ck, seen=seen, loader=loaders[0], valid=loaders[1:3])


def _assert_same_epochs(x, y):
    for a, b in zip(x, y):          # the bands of test_gpu_boundary.py::test_resident_dataset_equals_host_dataset (two runs of the same arithmetic)
        np.testing.assert_allclose(a[0], b[0], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(a[1], b[1], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(a[2], b[2], rtol=1e-4, atol=2e-4)
        np.testing.assert_allclose(a[3], b[3], rtol=1e-5, atol=1e-7)
        np.testing.assert_allclose(a[4], b[4], rtol=1e-4, atol=1e-5)
        np.testing.assert_array_equal(a[5], b[5])


def test_shuffled_epochs_equal_pregathered_epochs(shuffled_run):
    """(a) --shuffle, resident; (b) the same Solver over plain list loaders of host tensors gathered with index_select from the
    permutations (a)'s loader reported, one list per pass; (c) --shuffle --host_data.  Same losses, MI terms, validation loss and banks;
    the label bank is labels[perm] of the model pass; the permutations change from pass to pass."""
    ld, seen = shuffled_run["loader"], shuffled_run["seen"]
    assert [i for i, _ in seen] == [0, 1, 2]                       # epoch 0: model pass; epoch 1: critic pass + model pass
    perms = [p for _, p in seen]
    assert all(sorted(p.tolist()) == list(range(100)) for p in perms)
    assert not torch.equal(perms[1], perms[0]) and not torch.equal(perms[2], perms[0]) and not torch.equal(perms[2], perms[1])
    y = ld.y.cpu()
    for ep, p in ((0, perms[0]), (1, perms[2])):
        np.testing.assert_array_equal(shuffled_run["res"][ep][5].reshape(-1), y[p].numpy())
    t, a, v = ld.t.cpu(), ld.a.cpu(), ld.v.cpu()

    def listed(p):
        out = []
        for i in range(0, 100, 16):
            ix = p[i:i + 16]
            ones = torch.ones(len(ix), 12, dtype=torch.long)
            out.append((None, a.index_select(0, ix), v.index_select(0, ix), None, None, y.index_select(0, ix).reshape(-1, 1),
                        t.index_select(0, ix), torch.zeros_like(ones), ones, None, None))
        return out
    lists = [listed(p) for p in perms]
    opt = Parameters.parse_args(ARGV)
    sol = _solver(opt, (lists[0],) + tuple(shuffled_run["valid"]) + (768, 74, 35))
    res_b, _ = _two_epochs(sol, lists)
    _assert_same_epochs(shuffled_run["res"], res_b)

    opt = Parameters.parse_args(ARGV + ["--shuffle", "--host_data"])
    loaders = get_data_loader(opt)
    assert loaders[0].shuffle and loaders[0].t.is_pinned() and not loaders[0].t.is_cuda
    seen_c = _spy(loaders[0])
    res_c, _ = _two_epochs(_solver(opt, loaders))
    assert all(i == j and torch.equal(p, q) for (i, p), (j, q) in zip(seen, seen_c)) and len(seen_c) == 3
    _assert_same_epochs(shuffled_run["res"], res_c)


def test_resume_continues_the_permutation_sequence(shuffled_run, tmp_path):
    """A checkpoint written after epoch 0, through torch.save / load_checkpoint(path) (weights_only=True: ``loader_pass`` is a plain
    int), into a fresh Solver over a fresh shuffling loader: its next pass draws what the uninterrupted run drew for epoch 1."""
    assert shuffled_run["ck"]["loader_pass"] == 1 and type(shuffled_run["ck"]["loader_pass"]) is int
    path = str(tmp_path / "ck.pth.tar")
    torch.save(shuffled_run["ck"], path)
    opt = Parameters.parse_args(ARGV + ["--shuffle"])
    loaders = get_data_loader(opt)
    sol = _solver(opt, loaders)
    assert loaders[0].pass_index == 0
    assert sol.load_checkpoint(path) == 0
    assert loaders[0].state() == {"pass_index": 1}
    for want in shuffled_run["seen"][1:]:
        got = torch.cat([d[5].idx for d in loaders[0]]).cpu().long()
        assert torch.equal(got, want[1])
    # an unshuffled run's checkpoint has no such entry, and loads into a shuffling Solver without moving its loader
    plain_opt = Parameters.parse_args(ARGV)
    ck = _solver(plain_opt, get_data_loader(plain_opt)).checkpoint(0)
    assert "loader_pass" not in ck
    before = loaders[0].pass_index
    sol.load_checkpoint(ck)
    assert loaders[0].pass_index == before
