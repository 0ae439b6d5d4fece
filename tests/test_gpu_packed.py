"""-m gpu: --data_file on the device.  mimrl_op_gather_packed against data.Packed.materialize (bit-exact: it only moves bytes and writes
zeros), the engine's Packed upload (resident and pinned-host datasets, both input sets, a partial batch), two epochs of Solver.train over
a PackedLoader against the same epochs over pre-padded plain batches, and Main.py --data_file end to end."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from mimrl_amd import Parameters, _lib, synth
from mimrl_amd.data import Packed, PackedLoader, Rows, get_data_loader, pack_padded, save_packed
from tests.helpers import case
from tests.test_gpu_shuffle import ARGV, _assert_same_epochs, _offset_by_one_float, _solver, _spy, _two_epochs

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

N_SRC, T = 7, 12
SENTINEL = -12345.0
# frames of 3072 B (16 bytes per lane; a 36 KB row = three chunks, the frames / padding boundary inside a chunk), 296 B (8 bytes per
# lane), 140 B (4 bytes per lane), dense labels (4 B) -- and frames of 4096 B: a 48 KB row of exactly three chunks, length 4 puts the
# boundary ON a chunk edge (chunk 1 and 2 only store), length 8 on the next
GROUPS = ([(768,), (74,), (35,), None], [(1024,), (74,), (35,), None])
LENGTHS = ([0, 1, 5, 11, 12, 5, 12], [12, 0, 1, 5, 11, 12, 1], [11, 12, 0, 1, 5, 0, 12], None)
LENGTHS_1024 = [4, 0, 12, 1, 5, 11, 8]
INDEX_SETS = ([3], [0, N_SRC - 1, 2, 2, 4], list(range(N_SRC - 1, -1, -1)))


def _place(x, dev, offset):
    if not offset:
        return x.to(dev)
    t = _offset_by_one_float(x.numel(), dev).view(x.shape)
    t.copy_(x)
    return t


def sources(shapes, dev, seed=0, src_offset=()):
    """One source per array: (frames [F, d], start int64 [N], length int32 [N]) of a packed array, or a dense [N, 1] tensor."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for a, sh in enumerate(shapes):
        if sh is None:
            out.append(_place(torch.randn(N_SRC, 1, generator=g), dev, a in src_offset))
            continue
        ln = torch.tensor(LENGTHS_1024 if sh == (1024,) else LENGTHS[a], dtype=torch.int32)
        st = torch.cumsum(ln.long(), 0) - ln.long()
        out.append((_place(torch.randn(int(ln.sum()), *sh, generator=g), dev, a in src_offset), st.to(dev), ln.to(dev)))
    return out


def gather(srcs, idx, max_workgroups=0, n_src=None, dst_offset=(), frames=T, src_frames=None):
    """mimrl_op_gather_packed over ``srcs`` -> the padded / gathered tensors; every destination lies between two runs of 64 sentinel
    floats, which must come back untouched.  ``dst_offset``: positions whose destination starts one float off alignment."""
    lib = _lib.load()
    packed = [isinstance(s, tuple) for s in srcs]
    base = [s[0] if p else s for s, p in zip(srcs, packed)]
    dev = base[0].device
    idx_t = torch.tensor(idx, dtype=torch.int32, device=dev)
    rows, n = len(idx), len(srcs)
    fr = [frames if p else 1 for p in packed]
    width = [int(b.shape[1]) for b in base]
    row = [f * w for f, w in zip(fr, width)]
    bufs, dsts = [], []
    for a in range(n):
        m = 64 + rows * row[a] + 64
        buf = _offset_by_one_float(m, dev) if a in dst_offset else torch.empty(m, dtype=torch.float32, device=dev)
        buf.fill_(SENTINEL)
        bufs.append(buf)
        dsts.append(buf[64:64 + rows * row[a]])
    P = lambda v: (C.c_void_p * n)(*v)
    rc = lib.mimrl_op_gather_packed(C.c_void_p(torch.cuda.current_stream().cuda_stream), n, P(b.data_ptr() for b in base), P(d.data_ptr() for d in dsts),
                                    (C.c_int64 * n)(*(4 * w for w in width)), (C.c_int32 * n)(*fr),
                                    P(s[1].data_ptr() if p else None for s, p in zip(srcs, packed)),
                                    P(s[2].data_ptr() if p else None for s, p in zip(srcs, packed)),
                                    (C.c_int64 * n)(*(src_frames if src_frames is not None else [int(b.shape[0]) for b in base])),
                                    int(n_src if n_src is not None else N_SRC), C.c_void_p(idx_t.data_ptr()), rows, int(max_workgroups))
    _lib.check(rc)
    torch.cuda.synchronize()
    for buf in bufs:
        assert bool((buf[:64] == SENTINEL).all()) and bool((buf[-64:] == SENTINEL).all()), "the gather wrote outside its destination"
    return [d.reshape(rows, fr[a], width[a]) if packed[a] else d.reshape(rows, 1) for a, d in enumerate(dsts)]


def reference(s, idx, frames=T):
    """materialize() of one source: plain torch."""
    ix = torch.tensor(idx, dtype=torch.int32, device=(s[0] if isinstance(s, tuple) else s).device)
    return Packed(s[0], s[1], s[2], ix, frames).materialize() if isinstance(s, tuple) else Rows(s, ix).materialize()


def _same_bits(x, y):
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def check_gather_exact():
    """The op-level exactness case (also run under the deterministic build by tests/packed_det_worker.py)."""
    dev = torch.device("cuda")
    n = 0
    for gi, shapes in enumerate(GROUPS):
        for src_off, dst_off in (((), ()), ((0, 1), ()), ((), (0, 2)), ((3,), (3,))):
            srcs = sources(shapes, dev, seed=gi, src_offset=src_off)
            assert all(((s[0] if isinstance(s, tuple) else s).data_ptr() % 16 == 4) == (a in src_off) for a, s in enumerate(srcs))
            for idx in INDEX_SETS:
                want = [reference(s, idx) for s in srcs]
                for mw in (1, 0):
                    got = gather(srcs, idx, mw, dst_offset=dst_off)                           # the four arrays of a batch in ONE call
                    for a in range(4):
                        assert _same_bits(got[a], want[a]), (shapes[a], idx, mw, src_off, dst_off)
                        one = gather([srcs[a]], idx, mw, dst_offset=(0,) if a in dst_off else ())[0]     # ... and one call per array
                        assert _same_bits(one, want[a]), (shapes[a], idx, mw, src_off, dst_off, "n_arrays=1")
                        n += 1
    # a sample longer than the row keeps its first frames: frames = 8 against lengths of 11 and 12
    srcs = sources(GROUPS[1], dev, seed=5)
    got = gather(srcs, INDEX_SETS[2], frames=8)
    for a in range(4):
        assert _same_bits(got[a], reference(srcs[a], INDEX_SETS[2], frames=8))
    return n


def test_gather_packed_equals_materialize():
    assert check_gather_exact() == 2 * 4 * 3 * 2 * 4


def test_bad_samples_are_nan_rows_and_bad_arguments_are_refused():
    dev = torch.device("cuda")
    lib = _lib.load()
    srcs = sources(GROUPS[0], dev, seed=7)
    good = [reference(s, [2, 0, 6]) for s in srcs]

    def nan_rows_0_and_2(got, why):
        for a, g in enumerate(got):
            assert bool(torch.isnan(g[0]).all()) and bool(torch.isnan(g[2]).all()), (why, a)
            assert _same_bits(g[[1, 3, 4]], good[a]), (why, a)

    for bad in (-1, N_SRC, 2 ** 30):
        for mw in (1, 0):
            nan_rows_0_and_2(gather(srcs, [bad, 2, bad, 0, 6], mw), bad)
    # ... src_rows is the bound, not the allocation
    got = gather(srcs, [5, 4], n_src=5)
    assert all(bool(torch.isnan(g[0]).all()) and _same_bits(g[1:], reference(s, [4])) for g, s in zip(got, srcs))
    # a sample whose start or length cannot be honoured in ONE array is a NaN row in EVERY array; its neighbours stay exact
    F = [int(s[0].shape[0]) for s in srcs[:3]]
    for why, a, field, value in (("negative start", 1, 1, -1), ("negative length", 2, 2, -1), ("start past the frames", 0, 1, F[0] + 1),
                                 ("start + length past the frames", 1, 2, F[1] + 1), ("start + length overflows", 0, 1, 2 ** 63 - 1)):
        hurt = list(srcs)
        t = srcs[a][field].clone()
        t[3] = value
        hurt[a] = tuple(t if k == field else x for k, x in enumerate(srcs[a]))
        for mw in (1, 0):
            nan_rows_0_and_2(gather(hurt, [3, 2, 3, 0, 6], mw), why)
    # src_frames is the bound, not the allocation: one frame fewer, and the sample that owns the last frame is out (LENGTHS: sample 6)
    for a in range(3):
        assert int(srcs[a][2][6]) > 0
    got = gather(srcs, [6, 2, 6, 0, 5], src_frames=[F[0], F[1] - 1, F[2], 0])
    for a, g in enumerate(got):
        assert bool(torch.isnan(g[0]).all()) and bool(torch.isnan(g[2]).all()) and _same_bits(g[[1, 3, 4]], reference(srcs[a], [2, 0, 5])), a
    # every argument the launch cannot honour is refused before it
    x, st, ln = srcs[1]
    d = torch.empty(4, T, 74, device=dev)
    idx = torch.zeros(4, dtype=torch.int32, device=dev)
    s = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    P, I, J = lambda *p: (C.c_void_p * len(p))(*p), lambda *v: (C.c_int64 * len(v))(*v), lambda *v: (C.c_int32 * len(v))(*v)
    ok = dict(n=1, src=P(x.data_ptr()), dst=P(d.data_ptr()), fb=I(296), fr=J(T), st=P(st.data_ptr()), ln=P(ln.data_ptr()), sf=I(F[1]), sr=N_SRC,
              idx=C.c_void_p(idx.data_ptr()), rows=4, mw=0)
    call = lambda **kw: (lambda a: lib.mimrl_op_gather_packed(s, a["n"], a["src"], a["dst"], a["fb"], a["fr"], a["st"], a["ln"], a["sf"], a["sr"],
                                                              a["idx"], a["rows"], a["mw"]))(dict(ok, **kw))
    assert call() == 0
    five = dict(src=P(*[x.data_ptr()] * 5), dst=P(*[d.data_ptr()] * 5), fb=I(*[296] * 5), fr=J(*[T] * 5), st=P(*[st.data_ptr()] * 5),
                ln=P(*[ln.data_ptr()] * 5), sf=I(*[F[1]] * 5))
    for kw in (dict(rows=0), dict(rows=-3), dict(n=0), dict(n=5, **five), dict(src=None), dict(dst=None), dict(fb=None), dict(fr=None),
               dict(st=None), dict(ln=None), dict(sf=None), dict(idx=None), dict(src=P(None)), dict(dst=P(None)), dict(fb=I(0)), dict(fb=I(-296)),
               dict(fb=I(294)), dict(fb=I(2)), dict(fr=J(0)), dict(fr=J(-1)), dict(st=P(None)), dict(ln=P(None)), dict(sf=I(-1)), dict(mw=-1),
               dict(sr=-1), dict(src=P(x.data_ptr() + 2)), dict(st=P(st.data_ptr() + 4)), dict(ln=P(ln.data_ptr() + 2)),
               dict(fb=I(2 ** 33), fr=J(4))):
        assert call(**kw) == -1, kw
        assert lib.mimrl_last_error().decode().startswith("gather_packed:"), kw
    assert call(st=P(None), ln=P(None), fr=J(1), sr=F[1] // T) == 0           # (both NULL: the array is dense)
    torch.cuda.synchronize()


def test_deterministic_build_pads_the_same_bytes():
    """The op-level exactness case once under MIMRL_DETERMINISTIC=1 (the library is chosen at import: its own process)."""
    env = dict(os.environ, MIMRL_DETERMINISTIC="1", PYTHONPATH=ROOT)
    env.pop("MIMRL_LIB_PATH", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "packed_det_worker.py")], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "packed gather exact under the deterministic build" in r.stdout, r.stdout


def _packed_dataset(n, Tn, seed, place):
    """n ragged samples (lengths 0..Tn, sample 0 empty and sample 1 full in every modality) -> ([text, audio, video] as (frames, start,
    length) placed by ``place``, labels [n, 1], the padded host tensors)."""
    g = np.random.default_rng(seed)
    packed, padded = [], []
    for d in (768, 74, 35):
        ln = g.integers(0, Tn + 1, n)
        ln[0], ln[1] = 0, Tn
        x = g.standard_normal((n, Tn, d)).astype(np.float32)
        x[np.arange(Tn)[None, :] >= ln[:, None]] = 0.0
        frames, length = pack_padded(x)
        assert np.array_equal(length, ln)
        start = np.cumsum(length, dtype=np.int64) - length
        packed.append(tuple(place(torch.from_numpy(v)) for v in (frames, start, length)))
        padded.append(torch.from_numpy(x))
    y = torch.from_numpy(g.uniform(-3, 3, (n, 1)).astype(np.float32))
    padded.append(y)
    return packed, place(y), padded


@pytest.mark.parametrize("host", [False, True], ids=["resident", "pinned-host"])
def test_engine_uploads_packed_batches(host, monkeypatch):
    """stage_batch(Packed...) + commit_batch() and set_batch(Packed...): the bound inputs are materialize() of the batch, for a dataset in
    HBM (ONE mimrl_op_gather_packed on the upload stream, labels riding along) and in pinned host memory (padded on the host into the
    engine's staging tensors + H2D); staged batches use both input sets; a partial last batch goes through a sibling engine."""
    from mimrl_amd.engine import HipEngine
    c, opt, batch, banks = case("tiny_sep")
    B, Tn, n = c["B"], c["T"], 3 * c["B"] + 3
    eng = HipEngine(opt, 768, 74, 35, seq_len=Tn, bank_capacity=c["N"])
    launches, native = [], eng.lib.mimrl_op_gather_packed
    monkeypatch.setattr(eng.lib, "mimrl_op_gather_packed", lambda *a: launches.append((a[0].value or 0, a[1], a[-2])) or native(*a))
    dense = []
    monkeypatch.setattr(eng.lib, "mimrl_op_gather_rows", lambda *a: dense.append(a) or -1)
    place = (lambda x: x.pin_memory()) if host else (lambda x: x.to(eng.device))
    packed, y, padded = _packed_dataset(n, Tn, 11, place)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(11)).to(torch.int32)

    def sources_for(idx):
        idx_d = idx if host else idx.to(eng.device)
        return tuple(Packed(f, st, ln, idx_d, Tn) for f, st, ln in packed) + (Rows(y, idx_d),)

    def bound(e):
        return [x.cpu().reshape(len(e.labels), -1) for x in (e.text, e.audio, e.video, e.labels)]

    def check(e, idx, srcs, tag):
        torch.cuda.synchronize()
        for got, s, x in zip(bound(e), srcs, padded):
            assert torch.equal(got, s.materialize().cpu().reshape(len(idx), -1)), (tag, tuple(x.shape))
            assert torch.equal(got, x[idx.long()].reshape(len(idx), -1)), (tag, tuple(x.shape))        # ... which is host padding

    seen = set()
    for i in range(3):
        idx = perm[i * B:(i + 1) * B]
        srcs = sources_for(idx)
        eng.stage_batch(*srcs)
        eng.commit_batch()
        check(eng, idx, srcs, i)
        seen.add(eng.text.data_ptr())
    assert len(seen) == 2
    # a resident batch is ONE launch for its four arrays, on the upload stream; a host batch launches nothing
    assert launches == ([] if host else [(eng._copy_stream.cuda_stream, 4, B)] * 3)
    idx = torch.arange(B - 1, -1, -1, dtype=torch.int32)
    srcs = sources_for(idx)
    eng.set_batch(*srcs)
    check(eng, idx, srcs, "set_batch")
    assert launches[3:] == ([] if host else [(eng.stream.cuda_stream, 4, B)])
    # a partial last batch: a sibling engine of that batch size, through set_batch and through the staged path
    tail = HipEngine(opt, 768, 74, 35, seq_len=Tn, share=eng, batch=3)
    idx = perm[3 * B:]
    assert len(idx) == 3
    srcs = sources_for(idx)
    tail.set_batch(*srcs)
    check(tail, idx, srcs, "tail set_batch")
    srcs = sources_for(idx.flip(0).contiguous())
    tail.stage_batch(*srcs)
    tail.commit_batch()
    check(tail, idx.flip(0), srcs, "tail staged")
    n_launch = len(launches)
    assert n_launch == (0 if host else 6)
    # GATHER_ROWS = False, sources that do not share ONE index tensor, or Packed beside plain tensors: materialize() and copy
    idx = perm[:B]
    srcs = sources_for(idx)
    monkeypatch.setattr(HipEngine, "GATHER_ROWS", False)
    eng.set_batch(*srcs)
    check(eng, idx, srcs, "materialize")
    monkeypatch.setattr(HipEngine, "GATHER_ROWS", True)
    other = sources_for(idx.clone())
    eng.set_batch(srcs[0], other[1], padded[2][idx.long()], srcs[3])
    check(eng, idx, srcs, "mixed")
    assert len(launches) == n_launch
    # a batch of another size, a sequence length or a width the input does not have: refused before anything is launched
    with pytest.raises(_lib.MimrlError):
        eng.set_batch(*sources_for(perm[:B - 1]))
    idx_d = idx if host else idx.to(eng.device)
    with pytest.raises(_lib.MimrlError):
        eng.set_batch(Packed(*packed[0], idx_d, Tn - 1), *(Packed(f, st, ln, idx_d, Tn) for f, st, ln in packed[1:]), Rows(y, idx_d))
    with pytest.raises(_lib.MimrlError):
        eng.set_batch(*(Packed(f, st, ln, idx_d, Tn) for f, st, ln in (packed[1], packed[1], packed[2])), Rows(y, idx_d))
    assert len(launches) == n_launch and not dense       # (the dense gather is never asked for a packed batch)
    tail.close()
    eng.close()


N_TRAIN, N_VALID, N_TEST = 100, 32, 24


def _ragged_split(n, seed, with_class=False):
    """synth.synthetic_batch(n, 12, ragged=True) with the text made ragged too -> (packed split, padded arrays)."""
    t, a, v, y = synth.synthetic_batch(n, T, seed=seed, ragged=True)
    lt = np.random.default_rng(seed + 100).integers(1, T + 1, n)
    lt[0] = T
    t[np.arange(T)[None, :] >= lt[:, None]] = 0.0
    sp, lens = {}, []
    for m, x in (("text", t), ("audio", a), ("video", v)):
        sp[m], ln = pack_padded(x)
        lens.append(ln)
    assert np.array_equal(lens[0], lt) and min(l.min() for l in lens) >= 1 and all(l.min() < T for l in lens)
    sp["len"], sp["y"] = np.stack(lens, axis=1), y
    sp["y_class"] = synth.class_labels(y, 7).astype(np.int64) if with_class else None
    return sp, (t, a, v, y)


@pytest.fixture(scope="module")
def packed_file(tmp_path_factory):
    made = {s: _ragged_split(n, seed, with_class=True) for s, n, seed in (("train", N_TRAIN, 0), ("valid", N_VALID, 1), ("test", N_TEST, 2))}
    path = str(tmp_path_factory.mktemp("packed") / "ragged.npz")
    save_packed(path, {s: sp for s, (sp, _) in made.items()})
    return path, {s: padded for s, (_, padded) in made.items()}


def _run_and_close(sol, passes=None):
    """_two_epochs, then the Solver's engines are destroyed: nothing of this module stays on the device behind it."""
    try:
        return _two_epochs(sol, passes)[0]
    finally:
        for e in list(sol._tails.values()) + [sol.engine]:
            e.close()


def _listed(padded, order):
    """Pre-padded plain batches of 16 in ``order``: the 'Dec' tuple of host tensors."""
    t, a, v, y = (torch.from_numpy(x) for x in padded)
    out = []
    for i in range(0, len(order), 16):
        ix = order[i:i + 16]
        ones = torch.ones(len(ix), T, dtype=torch.long)
        out.append((None, a.index_select(0, ix), v.index_select(0, ix), None, None, y.index_select(0, ix).reshape(-1, 1), t.index_select(0, ix),
                    torch.zeros_like(ones), ones, None, None))
    return out


@pytest.mark.parametrize("shuffle", [False, True], ids=["in-order", "shuffle"])
def test_packed_epochs_equal_prepadded_epochs(shuffle, packed_file, monkeypatch):
    """Two epochs of train + evaluate from the packed file (resident: every batch padded by mimrl_op_gather_packed, a partial last batch
    of 4 included) against the same Solver over plain lists of the same samples padded on the host, in the same order."""
    path, padded = packed_file
    opt = Parameters.parse_args(ARGV + ["--data_file", path] + (["--shuffle"] if shuffle else []))
    loaders = get_data_loader(opt)
    assert isinstance(loaders[0], PackedLoader) and loaders[0].base["text"].is_cuda and loaders[0].shuffle == shuffle
    assert loaders[3:] == (768, 74, 35) and (loaders[0].n, loaders[1].n, loaders[2].n) == (N_TRAIN, N_VALID, N_TEST)
    seen = _spy(loaders[0])
    launches, lib = [], _lib.load()
    native = lib.mimrl_op_gather_packed
    monkeypatch.setattr(lib, "mimrl_op_gather_packed", lambda *a: launches.append(a[-2]) or native(*a))
    res_a = _run_and_close(_solver(opt, loaders))
    monkeypatch.undo()
    per_pass = [16] * 6 + [4]
    assert launches == per_pass + [16, 16] + (per_pass * 2 + [16, 16])         # epoch 0: train + valid; epoch 1: critic pass, train, valid
    if shuffle:
        assert [i for i, _ in seen] == [0, 1, 2]
        orders = [p for _, p in seen]
        np.testing.assert_array_equal(res_a[1][5].reshape(-1), padded["train"][3][orders[2].numpy()])
    else:
        assert not seen
        orders = [torch.arange(N_TRAIN)] * 3
        np.testing.assert_array_equal(res_a[1][5].reshape(-1), padded["train"][3])
    lists = [_listed(padded["train"], o) for o in orders]
    valid = _listed(padded["valid"], torch.arange(N_VALID))
    plain_opt = Parameters.parse_args(ARGV)
    res_b = _run_and_close(_solver(plain_opt, (lists[0], valid, valid, 768, 74, 35)), lists)
    _assert_same_epochs(res_a, res_b)
    assert all(np.isfinite(r[0]) and np.isfinite(r[3]) for r in res_a)


CLI = ["--batch_size", "16", "--time_len", "12", "--d_hiddens", "12-3-128=4-3-128", "--d_outs", "12-3-128=4-3-128", "--bias", "--res_project", "1-1",
       "--dropout", "0.0-0.0-0.0-0.0", "--dropout_mlp", "0.0-0.0-0.0", "--epochs_num", "2", "--stage1_n", "1", "--gradient_clip", "1.5",
       "--learning_rate", "1e-3", "--precision", "bf16"]
CLI_CASES = {"regression-normalized": ["--dataset", "mosi_Dec", "--normalize", "0-1-1", "--shuffle"],
             "classification": ["--dataset", "synthetic", "--task", "classification", "--num_class", "7", "--loss", "CE"]}


@pytest.mark.parametrize("name", list(CLI_CASES))
def test_main_cli_trains_from_a_data_file(name, packed_file, tmp_path):
    """`python Main.py --data_file F --epochs_num 2` (n = 100, B = 16, T = 12, bf16): with --normalize 0-1-1, and as a 7-class classifier
    on the file's class indices.  Both finish, write the result files and log no NaN -- and no word of synthetic data."""
    cmd = [sys.executable, os.path.join(ROOT, "Main.py"), "--data_file", packed_file[0], "--task_name", "cli_packed"] + CLI + CLI_CASES[name]
    r = subprocess.run(cmd, cwd=tmp_path, capture_output=True, text=True, timeout=600, env=dict(os.environ, PYTHONPATH=ROOT))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    out = tmp_path / "TaskRuning" / "cli_packed"
    log = (out / "Running.log").read_text()
    assert "Training complete." in log and "nan" not in log.lower() and "SYNTHETIC" not in log + r.stderr
    for f in ("predictions_val.npy", "predictions_test.npy", "targets_val.npy", "targets_test.npy", "best_valid_model.pth.tar"):
        assert (out / f).exists(), f
    targets = np.load(out / "targets_test.npy").reshape(-1)
    want = packed_file[1]["test"][3]
    want = synth.class_labels(want, 7) if name == "classification" else want
    assert np.array_equal(targets, want)                                     # the test split of the FILE, whole and in order
    assert np.isfinite(np.load(out / "predictions_test.npy")).all()
    if name == "classification":
        assert log.count("Val_7-class_acc:[") == 2
