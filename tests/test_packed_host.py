"""CPU tier: --data_file (train on a user's dataset from a packed file: per-sample frame runs, padded per batch).  The file format and
its load-time checks and transforms, data.Packed, data.PackedLoader, how Solver hands Packed batches on, tools/pack_dataset.py and the
exported symbol."""
import logging
import os
import re
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mimrl_amd import Parameters, _lib
from mimrl_amd.Solver import Solver
from mimrl_amd.data import (Packed, PackedLoader, Rows, SyntheticLoader, get_data_loader, load_packed, pack_padded, plain, prepare_packed,
                            save_packed)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T, DIMS = 6, (8, 5, 3)
ARGV = ["--dataset", "synthetic", "--batch_size", "8", "--time_len", str(T)]
MODS = ("text", "audio", "video")


def _split(n, seed, t_max=T, y_class=True):
    """One split: n samples with lengths in [0, t_max] per modality (sample 0 empty everywhere, sample 1 full everywhere)."""
    g = np.random.default_rng(seed)
    ln = g.integers(0, t_max + 1, size=(n, 3)).astype(np.int32)
    ln[0], ln[1] = 0, t_max
    sp = {m: g.standard_normal((int(ln[:, k].sum()), DIMS[k])).astype(np.float32) for k, m in enumerate(MODS)}
    sp["len"] = ln
    sp["y"] = g.uniform(-3, 3, n).astype(np.float32)
    sp["y_class"] = g.integers(0, 7, n).astype(np.int64) if y_class else None
    return sp


def _splits(n=(40, 10, 12), **kw):
    return {s: _split(m, i, **kw) for i, (s, m) in enumerate(zip(("train", "valid", "test"), n))}


def _padded(sp, m, k, t=T):
    """Host padding, sample by sample: the definition everything else is held to."""
    out = np.zeros((len(sp["y"]), t, sp[m].shape[1]), np.float32)
    at = 0
    for i, l in enumerate(sp["len"][:, k]):
        out[i, :min(l, t)] = sp[m][at:at + min(l, t)]
        at += l
    return out


def _file(tmp_path, splits=None, **override):
    path = str(tmp_path / "data.npz")
    save_packed(path, splits if splits is not None else _splits())
    if override:
        with np.load(path) as z:
            d = {k: z[k] for k in z.files}
        for k, v in override.items():
            if v is None:
                d.pop(k)
            else:
                d[k] = v
        np.savez(path, **d)
    return path


def _bits(x):
    return np.ascontiguousarray(np.asarray(x, dtype=np.float32)).view(np.int32)


def test_flag_parses_and_defaults_empty():
    assert Parameters.parse_args(ARGV).data_file == ""
    assert Parameters.parse_args(ARGV + ["--data_file", "x.npz"]).data_file == "x.npz"


def test_save_load_round_trip(tmp_path):
    splits = _splits()
    got = load_packed(_file(tmp_path, splits))
    for s, sp in splits.items():
        for m in MODS:
            assert got[s][m].dtype == np.float32 and np.array_equal(got[s][m], sp[m])
        assert got[s]["len"].dtype == np.int32 and np.array_equal(got[s]["len"], sp["len"])
        assert np.array_equal(got[s]["y"], sp["y"]) and np.array_equal(got[s]["y_class"], sp["y_class"]) and got[s]["y_class"].dtype == np.int64
    with np.load(_file(tmp_path, splits), allow_pickle=False) as z:              # a plain .npz of the documented keys and dtypes
        assert z["format"].dtype == np.int32 and int(z["format"]) == 1
        assert z["train_len"].dtype == np.int32 and z["train_len"].shape == (40, 3) and z["train_y_class"].dtype == np.int64
    # y_class is optional
    got = load_packed(_file(tmp_path, _splits(y_class=False)))
    assert all(got[s]["y_class"] is None for s in got)


def test_pack_padded_then_materialize_is_the_padded_input_bit_for_bit():
    g = np.random.default_rng(3)
    x = g.standard_normal((6, 5, 3)).astype(np.float32)
    lengths = [0, 5, 3, 1, 4, 5]                         # empty, full, and in between
    for i, l in enumerate(lengths):
        x[i, l:] = 0.0
    x[2, 1] = 0.0                                        # a zero row INSIDE sample 2: still one of its frames
    x[4, 0] = 0.0                                        # ... and as a first frame
    x[5, 2, 1] = np.nan                                  # (a NaN is not zero)
    frames, length = pack_padded(x)
    assert length.dtype == np.int32 and length.tolist() == lengths and frames.shape == (sum(lengths), 3) and frames.dtype == np.float32
    f2, l2 = pack_padded(torch.from_numpy(x))
    assert np.array_equal(_bits(f2), _bits(frames)) and np.array_equal(l2, length)
    start = np.zeros(6, np.int64)
    start[1:] = np.cumsum(length[:-1])
    base, st, ln = torch.from_numpy(frames), torch.from_numpy(start), torch.from_numpy(length)
    for idx in ([0, 1, 2, 3, 4, 5], [5, 5, 0], [2], [3, 2, 1, 0]):
        p = Packed(base, st, ln, torch.tensor(idx, dtype=torch.int32), 5)
        got = p.materialize()
        assert isinstance(p, Rows) and len(p) == len(idx) and got.shape == (len(idx), 5, 3)
        assert np.array_equal(_bits(got.numpy()), _bits(x[idx]))
        out = torch.full((len(idx), 5, 3), 7.0)
        assert p.materialize(out=out) is out and np.array_equal(_bits(out.numpy()), _bits(x[idx]))
        assert np.array_equal(_bits(plain(p).numpy()), _bits(x[idx]))
    # a shorter T crops, a longer one pads
    assert np.array_equal(_bits(Packed(base, st, ln, torch.arange(6, dtype=torch.int32), 2).materialize().numpy()), _bits(x[:, :2]))
    wide = Packed(base, st, ln, torch.arange(6, dtype=torch.int32), 8).materialize().numpy()
    assert np.array_equal(_bits(wide[:, :5]), _bits(x)) and not wide[:, 5:].any()
    # no frames at all
    none = Packed(torch.zeros(0, 3), torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), torch.tensor([1, 0], dtype=torch.int32), 4)
    assert none.materialize().shape == (2, 4, 3) and not none.materialize().any()
    with pytest.raises(ValueError, match="pack_padded"):
        pack_padded(np.zeros((3, 4)))


def test_every_refusal_fires_by_name(tmp_path):
    opt = lambda path, *more: Parameters.parse_args(ARGV + ["--data_file", path] + list(more))
    with pytest.raises(ValueError, match="'format' is 2"):
        load_packed(_file(tmp_path, format=np.asarray(2, np.int32)))
    with pytest.raises(ValueError, match="'format' is None"):
        load_packed(_file(tmp_path, format=None))
    ln = _splits()["valid"]["len"].copy()
    ln[3, 1] += 1
    with pytest.raises(ValueError, match=r"valid_len sums to \d+ audio frames, valid_audio holds \d+"):
        load_packed(_file(tmp_path, valid_len=ln))
    with pytest.raises(ValueError, match="test_len has a negative entry"):
        bad = _splits()["test"]["len"].copy()
        bad[2, 0], bad[3, 0] = -1, bad[3, 0] + bad[2, 0] + 1
        load_packed(_file(tmp_path, test_len=bad))
    with pytest.raises(ValueError, match=r"train_len has shape \(39, 3\)"):
        load_packed(_file(tmp_path, train_len=_splits()["train"]["len"][:39]))
    with pytest.raises(ValueError, match="missing test_y"):
        load_packed(_file(tmp_path, test_y=None))
    with pytest.raises(ValueError, match="test_video is 4 wide, train_video is 3 wide: feature widths differ between splits"):
        v = _splits()["test"]["video"]
        load_packed(_file(tmp_path, test_video=np.concatenate([v, v[:, :1]], axis=1)))
    # --task classification: the class indices must be there and inside [0, num_class)
    cls = ["--task", "classification", "--num_class", "7", "--loss", "CE"]
    with pytest.raises(ValueError, match="--task classification needs train_y_class"):
        get_data_loader(opt(_file(tmp_path, _splits(y_class=False)), *cls))
    yc = _splits()["valid"]["y_class"].copy()
    yc[4] = 7
    with pytest.raises(ValueError, match=r"valid_y_class has a class index outside \[0, 7\)"):
        get_data_loader(opt(_file(tmp_path, valid_y_class=yc), *cls))
    yc[4] = -1
    with pytest.raises(ValueError, match=r"valid_y_class has a class index outside \[0, 7\)"):
        get_data_loader(opt(_file(tmp_path, valid_y_class=yc), *cls))
    assert get_data_loader(opt(_file(tmp_path), *cls))[0].n == 40
    # --normalize of a constant modality, and --log_scale
    const = _splits()
    const["valid"]["audio"][:] = 0.25
    with pytest.raises(ValueError, match="--normalize: the audio frames of the valid split are constant"):
        get_data_loader(opt(_file(tmp_path, const), "--normalize", "0-1-0"))
    assert get_data_loader(opt(_file(tmp_path, const), "--normalize", "1-0-1"))[1].n == 10
    with pytest.raises(NotImplementedError, match="--log_scale with --data_file"):
        get_data_loader(opt(_file(tmp_path), "--log_scale", "0-0-1"))
    # without --data_file both flags are accepted as before
    plain_opt = Parameters.parse_args(ARGV + ["--synthetic_n", "16", "--log_scale", "1-1-1", "--normalize", "1-1-1"])
    assert isinstance(get_data_loader(plain_opt)[0], SyntheticLoader)


def test_nonfinite_features_become_zero_and_long_samples_are_cut_with_one_warning(tmp_path, caplog):
    splits = _splits(t_max=9)                            # lengths up to 9 against --time_len 6
    splits["train"]["text"][5, 2] = np.nan
    splits["train"]["video"][7, 0] = np.inf
    splits["test"]["audio"][1, 1] = -np.inf
    want = {s: {m: _padded(sp, m, k) for k, m in enumerate(MODS)} for s, sp in splits.items()}
    for s in want:
        for m in MODS:
            want[s][m][~np.isfinite(want[s][m])] = 0.0
    cut = {s: [int((sp["len"][:, k] > T).sum()) for k in range(3)] for s, sp in splits.items()}
    assert all(min(c) > 0 for c in cut.values())
    path = _file(tmp_path, splits)
    with caplog.at_level(logging.WARNING):
        loaders = get_data_loader(Parameters.parse_args(ARGV + ["--data_file", path, "--batch_size", "64"]))
    warned = [r.getMessage() for r in caplog.records if "keep their first" in r.getMessage()]
    assert len(warned) == 1
    for s, c in cut.items():
        assert f"{s} {c[0]}/{c[1]}/{c[2]}" in warned[0]
    for ld, s in zip(loaders[:3], ("train", "valid", "test")):
        d = next(iter(ld))
        for k, m in ((6, "text"), (1, "audio"), (2, "video")):
            assert int(d[k].length.max()) == T and np.array_equal(d[k].materialize().numpy(), want[s][m])
            assert d[k].base.shape[0] == int(np.minimum(splits[s]["len"][:, MODS.index(m)], T).sum())     # the tails are not kept
    # nothing to cut: no warning
    caplog.clear()
    with caplog.at_level(logging.WARNING):
        get_data_loader(Parameters.parse_args(ARGV + ["--data_file", _file(tmp_path)]))
    assert not [r for r in caplog.records if "keep their first" in r.getMessage()]


def test_normalize_uses_the_real_frames_only(tmp_path):
    splits = _splits()
    for sp in splits.values():
        sp["audio"] += 4.0                               # all positive: the zeros of a padded array would BE its minimum
        sp["video"] -= 5.0                               # all negative: ... its maximum
    path = _file(tmp_path, splits)
    loaders = get_data_loader(Parameters.parse_args(ARGV + ["--data_file", path, "--normalize", "0-1-1", "--batch_size", "64"]))
    for ld, (s, sp) in zip(loaders[:3], splits.items()):
        d = next(iter(ld))
        assert np.array_equal(d[6].base.numpy(), sp["text"])                      # not asked for: untouched
        for k, slot, m in ((1, 1, "audio"), (2, 2, "video")):
            x = sp[m]
            lo, hi = x.min(), x.max()
            want = 2.0 * (x.astype(np.float64) - lo) / (np.float64(hi) - lo) - 1.0
            got = d[slot].base.numpy()
            # float32 evaluation: four roundings (x - min, max - min, the product, the quotient), each 2^-24 relative, of a value in
            # [0, 2], and one of the result in [-1, 1]: at most 9 * 2^-24
            np.testing.assert_allclose(got, want, rtol=0, atol=9 * 2.0 ** -24)
            assert got.min() == -1.0 and got.max() == 1.0
            padded = _padded(sp, m, k)                   # the same formula over the PADDED array is another function of x
            plo, phi = padded.min(), padded.max()
            assert (plo, phi) != (lo, hi)
            over_padded = 2.0 * (x.astype(np.float64) - plo) / (np.float64(phi) - plo) - 1.0
            assert np.abs(over_padded - got).max() > 0.1
            # ... and the padding itself stays zero
            batch = d[slot].materialize().numpy()
            real = np.arange(T)[None, :] < sp["len"][:, k][:, None]
            assert not batch[~real].any()
    out, cut = prepare_packed(splits["train"], T, (False, False, False))
    assert cut == [0, 0, 0] and all(np.array_equal(out[m], splits["train"][m]) for m in MODS)


def _loader(n=100, **kw):
    kw = dict(dict(batch_size=16, T=T, seed=4), **kw)
    return PackedLoader(_split(n, 9), kw.pop("batch_size"), kw.pop("T"), **kw), _split(n, 9)


def _pass(loader):
    batches = list(loader)
    return [b[5].idx.clone() for b in batches], batches


def test_loader_batches_are_the_dec_tuple_of_packed_sharing_one_index_tensor():
    ld, sp = _loader()
    assert (len(ld), ld.num_samples(), ld.n, ld.shuffle) == (7, 100, 100, False)
    for _ in range(2):                                   # every unshuffled pass the same, and no pass counted
        p, batches = _pass(ld)
        assert torch.equal(torch.cat(p), torch.arange(100, dtype=torch.int32)) and [len(x) for x in p] == [16] * 6 + [4]
        for d in batches:
            assert len(d) == 11 and d[0] is d[3] is d[4] is d[9] is d[10] is None
            assert all(type(d[k]) is Packed for k in (1, 2, 6)) and type(d[5]) is Rows
            assert all(d[k].idx is d[5].idx for k in (1, 2, 6)) and d[5].idx.dtype == torch.int32
            assert d[7].shape == d[8].shape == (len(d[5]), T) and all(d[k].T == T for k in (1, 2, 6))
            assert d[5].idx.untyped_storage().data_ptr() == ld._arange.untyped_storage().data_ptr()        # slices of ONE arange
        for k, slot, m in ((0, 6, "text"), (1, 1, "audio"), (2, 2, "video")):
            assert batches[0][slot].base is ld.base[m] and ld.start[m].dtype == torch.int64 and ld.length[m].dtype == torch.int32
            got = torch.cat([d[slot].materialize() for d in batches]).numpy()
            assert np.array_equal(got, _padded(sp, m, k))
        assert np.array_equal(torch.cat([d[5].materialize() for d in batches]).numpy().reshape(-1), sp["y"])
    assert ld.pass_index == 0 and ld.state() == {"pass_index": 0}
    assert ld.packed_bytes() == sum(sp[m].nbytes for m in MODS) + 3 * 100 * 12 + 400
    # drop_last, and a last batch with fewer than k_neighbor rows is not produced
    assert len(_loader(drop_last=True)[0]) == 6 and _loader(drop_last=True)[0].num_samples() == 96
    assert [len(x) for x in _pass(_loader(n=98, k_neighbor=3)[0])[0]] == [16] * 6 and _loader(n=98, k_neighbor=3)[0].n == 96
    assert [len(x) for x in _pass(_loader(n=98, k_neighbor=2)[0])[0]] == [16] * 6 + [2]
    # labels="y_class": the class indices as floats
    cls = PackedLoader(sp, 16, T, labels="y_class")
    assert cls.y.dtype == torch.float32 and np.array_equal(cls.y.numpy(), sp["y_class"].astype(np.float32))


def test_shuffled_passes_are_permutations_and_a_pure_function_of_seed_rank_pass():
    ld, sp = _loader(shuffle=True)
    p0, b0 = _pass(ld)
    p1, _ = _pass(ld)
    p2, _ = _pass(ld)
    for p in (p0, p1, p2):
        assert [len(x) for x in p] == [16] * 6 + [4] and sorted(torch.cat(p).tolist()) == list(range(100))
        assert all(x.dtype == torch.int32 for x in p)
    assert not torch.equal(torch.cat(p0), torch.cat(p1)) and not torch.equal(torch.cat(p1), torch.cat(p2))
    assert ld.state() == {"pass_index": 3}
    for i, p in enumerate((p0, p1, p2)):
        assert torch.equal(ld.permutation(i), torch.cat(p).long())
    # the rule is SyntheticLoader's: the same (seed, rank, pass, n) give the same order
    synth_ld = SyntheticLoader(100, 16, 3, d_t=4, d_a=3, d_v=2, seed=4, shuffle=True)
    assert all(torch.equal(synth_ld.permutation(i), ld.permutation(i)) for i in range(3))
    # the batches are the permuted samples
    order = torch.cat(p0).long().numpy()
    assert np.array_equal(torch.cat([d[1].materialize() for d in b0]).numpy(), _padded(sp, "audio", 1)[order])
    assert np.array_equal(torch.cat([d[5].materialize() for d in b0]).numpy().reshape(-1), sp["y"][order])
    torch.manual_seed(99)                                # the global RNG plays no part
    same = _loader(shuffle=True)[0]
    for p in (p0, p1, p2):
        assert torch.equal(torch.cat(_pass(same)[0]), torch.cat(p))
    assert not torch.equal(_loader(shuffle=True, seed=5)[0].permutation(0), ld.permutation(0))
    assert not torch.equal(_loader(shuffle=True, rank=1)[0].permutation(0), ld.permutation(0))
    a, b = _loader(shuffle=True)[0], _loader(shuffle=True)[0]
    _pass(a); _pass(a)
    b.load_state(a.state())
    assert b.pass_index == 2 and torch.equal(torch.cat(_pass(b)[0]), torch.cat(_pass(a)[0]))
    c = _loader(shuffle=True)[0]
    iter(c)
    assert c.pass_index == 1                             # drawn and counted when iter() is called


def test_world_2_shards_are_repacked_disjoint_and_full():
    n, B = 101, 16
    sp = _split(n, 9)
    seen = []
    for r in (0, 1):
        ld = PackedLoader(sp, B, T, seed=4, rank=r, world=2, shuffle=True)
        keep = np.arange(n)[r::2][:n // 2]
        assert ld.n == 50 and len(ld) == 3 and ld.drop_last and np.array_equal(ld.y.numpy(), sp["y"][keep])
        for k, m in enumerate(MODS):                     # re-packed: the shard's frames only, starts from 0
            assert ld.base[m].shape[0] == int(sp["len"][keep, k].sum()) and int(ld.start[m][0]) == 0
            whole = Packed(ld.base[m], ld.start[m], ld.length[m], torch.arange(50, dtype=torch.int32), T).materialize().numpy()
            assert np.array_equal(whole, _padded(sp, m, k)[keep])
        for _ in range(2):
            p, batches = _pass(ld)
            assert len(p) == 3 and all(len(x) == B for x in p) and len(set(torch.cat(p).tolist())) == 48 and int(torch.cat(p).max()) < 50
        seen.append({float(x) for d in batches for x in d[5].materialize().reshape(-1)})
    assert not (seen[0] & seen[1])


def test_get_data_loader_reads_the_file_under_every_dataset_name(tmp_path, caplog):
    path = _file(tmp_path)
    for name in ("synthetic", "mosi_Dec", "mosei_Dec"):
        caplog.clear()
        with caplog.at_level(logging.WARNING):
            tr, va, te, d_t, d_a, d_v = get_data_loader(Parameters.parse_args(ARGV + ["--data_file", path, "--dataset", name, "--shuffle"]))
        assert not [r for r in caplog.records if "SYNTHETIC" in r.getMessage()]
        assert (d_t, d_a, d_v) == DIMS and all(isinstance(x, PackedLoader) for x in (tr, va, te))
        assert (tr.n, va.n, te.n) == (40, 10, 12) and (tr.shuffle, va.shuffle, te.shuffle) == (True, False, False)
    with pytest.raises(NotImplementedError):
        get_data_loader(Parameters.parse_args(ARGV + ["--data_file", path, "--dataset", "mosi_SDK"]))
    # the training split is sharded, valid and test are replicated
    tr, va, te = get_data_loader(Parameters.parse_args(ARGV + ["--data_file", path]), rank=1, world=2)[:3]
    assert (tr.n, va.n, te.n) == (20, 10, 12)
    assert np.array_equal(tr.y.numpy(), _splits()["train"]["y"][1::2])


def test_iter_loaded_hands_packed_batches_to_the_engine_in_the_lookahead_order():
    """tests/test_shuffle_host.py's hand-over test with a PackedLoader: the engine gets the Packed / Rows themselves (never a padded
    copy), the partial-batch engine is picked from len(labels)."""
    log = []

    class FakeEngine:
        def __init__(self, b):
            self.cfg = SimpleNamespace(batch=b)
        def _seen(self, what, t, a, v, y):
            assert all(type(x) is Packed for x in (t, a, v)) and type(y) is Rows and all(x.idx is y.idx for x in (t, a, v))
            log.append((what, self.cfg.batch, int(y.idx[0])))
        def set_batch(self, *b): self._seen("set", *b)
        def stage_batch(self, *b): self._seen("stage", *b)
        def commit_batch(self): log.append(("commit", self.cfg.batch))

    engines = {}
    sol = Solver.__new__(Solver)
    sol._engine_for = lambda b, training=True: engines.setdefault(b, FakeEngine(b))
    ld = PackedLoader(_split(14, 2), 4, T)
    for e, datas in sol._iter_loaded(ld):
        log.append(("step", e.cfg.batch, int(datas[5].idx[0])))
    assert log == [("set", 4, 0), ("step", 4, 0), ("stage", 4, 4), ("commit", 4), ("step", 4, 4), ("stage", 4, 8), ("commit", 4),
                   ("step", 4, 8), ("set", 2, 12), ("step", 2, 12)], log


def test_pipelined_stage1_pass_leaves_a_packed_loader_alone(monkeypatch):
    monkeypatch.setenv("MIMRL_EPOCH_PIPE", "1")
    sol = Solver.__new__(Solver)
    sol.world = 1
    sol.engine = SimpleNamespace(cfg=SimpleNamespace(use_graph=1, device_anchors=1, batch=16))
    sol.train_loader = _loader(shuffle=True)[0]
    assert sol._stage1_pass_pipelined(None) is False and sol.train_loader.pass_index == 0
    sol.train_loader = _loader()[0]                      # unshuffled: it shows Packed batches and is left to the sequential pass
    assert sol._stage1_pass_pipelined(None) is False


def test_pack_dataset_tool_converts_a_padded_file(tmp_path):
    splits = _splits(n=(9, 4, 5))
    padded = {}
    for s, sp in splits.items():
        for k, m in enumerate(MODS):
            padded[f"{s}_{m}"] = _padded(sp, m, k, t=T + k)                       # (T may differ between modalities)
        padded[f"{s}_y"], padded[f"{s}_y_class"] = sp["y"], sp["y_class"]
    src, dst = str(tmp_path / "padded.npz"), str(tmp_path / "packed.npz")
    np.savez(src, **padded)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "pack_dataset.py"), src, dst], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "train: 9 samples" in r.stdout and "test: 5 samples" in r.stdout
    got = load_packed(dst)
    for s, sp in splits.items():
        # a sample whose last frames happen to be all zero would come back shorter; random normal frames never are
        assert np.array_equal(got[s]["len"], sp["len"]) and all(np.array_equal(got[s][m], sp[m]) for m in MODS)
        assert np.array_equal(got[s]["y"], sp["y"]) and np.array_equal(got[s]["y_class"], sp["y_class"])


def test_library_exports_the_packed_gather():
    assert hasattr(_lib.load(), "mimrl_op_gather_packed") and "mimrl_op_gather_packed" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "mimrl.h")).read()
    assert re.search(r"\bint mimrl_op_gather_packed\s*\(void\* stream, int n_arrays, const void\* const\* src, void\* const\* dst,\s*"
                     r"const int64_t\* frame_bytes,\s*const int32_t\* frames, const int64_t\* const\* start, const int32_t\* const\* length,\s*"
                     r"const int64_t\* src_frames,\s*int64_t src_rows, const int32_t\* idx, int rows, int max_workgroups\);", header)
    assert len(_lib.load().mimrl_op_gather_packed.argtypes) == 13
    assert _lib.load().mimrl_abi_version() == 6
