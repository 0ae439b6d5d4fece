"""CPU tier: --shuffle (a fresh permutation of the training set every pass, like the reference's shuffle=True training loaders):
the flag, the loader's permutations as a pure function of (seed, rank, pass_index), data.Rows, and how Solver hands Rows batches on."""
import os
import re
from types import SimpleNamespace

import torch

from mimrl_amd import Parameters, _lib
from mimrl_amd.Solver import Solver
from mimrl_amd.data import Rows, SyntheticLoader, get_data_loader, plain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARGV = ["--dataset", "synthetic", "--synthetic_n", "40", "--batch_size", "8", "--time_len", "4"]


def _loader(**kw):
    kw = dict(dict(n=100, batch_size=16, T=3, d_t=8, d_a=5, d_v=3, seed=4), **kw)
    return SyntheticLoader(kw.pop("n"), kw.pop("batch_size"), kw.pop("T"), **kw)


def _pass(loader):
    """One pass -> (the row numbers of every batch, the batches)."""
    batches = list(loader)
    return [b[5].idx.clone() for b in batches], batches


def test_flag_parses_and_defaults_off():
    assert Parameters.parse_args(ARGV).shuffle is False
    assert Parameters.parse_args(ARGV + ["--shuffle"]).shuffle is True


def test_only_the_training_loader_shuffles():
    tr, va, te = get_data_loader(Parameters.parse_args(ARGV + ["--shuffle"]))[:3]
    assert (tr.shuffle, va.shuffle, te.shuffle) == (True, False, False)
    assert isinstance(next(iter(tr))[5], Rows) and torch.is_tensor(next(iter(va))[5]) and torch.is_tensor(next(iter(te))[5])
    assert not any(x.shuffle for x in get_data_loader(Parameters.parse_args(ARGV))[:3])


def test_unshuffled_loader_yields_todays_slices():
    ld = _loader()
    assert ld.shuffle is False
    for _ in range(2):                                   # every pass the same
        got = list(ld)
        assert len(got) == 7
        for i, d in enumerate(got):
            s = slice(16 * i, min(16 * i + 16, 100))
            for k, want in ((1, ld.a[s]), (2, ld.v[s]), (5, ld.y[s].reshape(-1, 1)), (6, ld.t[s])):
                assert torch.is_tensor(d[k]) and torch.equal(d[k], want)
            assert d[7].shape == d[8].shape == (s.stop - s.start, 3) and d[0] is d[3] is d[9] is None
    assert ld.pass_index == 0


def test_shuffled_passes_are_permutations_and_a_pure_function_of_seed_rank_pass():
    ld = _loader(shuffle=True)
    p0, b0 = _pass(ld)
    p1, _ = _pass(ld)
    p2, _ = _pass(ld)
    for p in (p0, p1, p2):
        assert [len(x) for x in p] == [16] * 6 + [4]
        assert sorted(torch.cat(p).tolist()) == list(range(100))
        assert all(x.dtype == torch.int32 for x in p)
    assert not torch.equal(torch.cat(p0), torch.cat(p1)) and not torch.equal(torch.cat(p1), torch.cat(p2))
    assert ld.state() == {"pass_index": 3}
    for i, p in enumerate((p0, p1, p2)):
        assert torch.equal(ld.permutation(i), torch.cat(p).long())
    # the 11-tuple: Rows in slots 1, 2, 5, 6 over the loader's own arrays, one index tensor per batch
    d = b0[0]
    assert all(isinstance(d[k], Rows) for k in (1, 2, 5, 6)) and all(d[k].idx is d[5].idx for k in (1, 2, 6))
    assert d[1].base is ld.a and d[2].base is ld.v and d[6].base is ld.t and len(d[5]) == 16 and len(b0[-1][5]) == 4
    assert torch.equal(d[5].materialize(), ld.y[p0[0].long()].reshape(-1, 1)) and d[7].shape == (16, 3)
    # same (seed, rank): the same sequence of passes; the global RNG plays no part
    torch.manual_seed(99)
    same = _loader(shuffle=True)
    for p in (p0, p1, p2):
        assert torch.equal(torch.cat(_pass(same)[0]), torch.cat(p))
    for other in (_loader(shuffle=True, seed=5), _loader(shuffle=True, n=200, rank=1, world=2)):
        assert not torch.equal(other.permutation(0), ld.permutation(0)[:other.n]) and not torch.equal(other.permutation(1), ld.permutation(1)[:other.n])
    assert not torch.equal(_loader(shuffle=True, rank=1).permutation(0), ld.permutation(0))
    # load_state(state()) on a fresh loader continues the sequence
    a, b = _loader(shuffle=True), _loader(shuffle=True)
    _pass(a); _pass(a)
    b.load_state(a.state())
    assert b.pass_index == 2 and torch.equal(torch.cat(_pass(b)[0]), torch.cat(_pass(a)[0])) and torch.equal(torch.cat(_pass(b)[0]), torch.cat(_pass(a)[0]))
    # the pass is drawn and counted when iter() is called
    c = _loader(shuffle=True)
    iter(c)
    assert c.pass_index == 1


def test_shards_stay_disjoint_and_full():
    n, B = 100, 16
    shards = [_loader(n=n, batch_size=B, shuffle=True, rank=r, world=2) for r in (0, 1)]
    full = _loader(n=n, batch_size=B)
    seen = []
    for r, ld in enumerate(shards):
        assert torch.equal(ld.y, full.y[r::2][:n // 2])             # static sharding: a rank permutes its own shard
        for _ in range(2):
            p, batches = _pass(ld)
            assert len(p) == n // 2 // B and all(len(x) == B for x in p)
            assert len(set(torch.cat(p).tolist())) == len(p) * B and int(torch.cat(p).max()) < n // 2
        seen.append({float(x) for d in batches for x in d[5].materialize().reshape(-1)})
    assert not (seen[0] & seen[1])


def test_rows_materialize_and_plain():
    base = torch.arange(60, dtype=torch.float32).reshape(10, 2, 3)
    idx = torch.tensor([9, 0, 3, 3], dtype=torch.int32)
    r = Rows(base, idx)
    assert len(r) == 4 and torch.equal(r.materialize(), base[idx.long()])
    assert torch.equal(plain(r), base[idx.long()]) and plain(base) is base and plain(None) is None


def test_iter_loaded_hands_rows_to_the_engine_in_the_lookahead_order():
    """The order tests/test_cli_and_host.py::test_upload_lookahead_order_and_host_data_flag pins for tensors, with Rows batches: the
    engine gets the Rows themselves (never a materialized copy), the partial-batch engine is picked from len(labels)."""
    log = []

    class FakeEngine:
        def __init__(self, b):
            self.cfg = SimpleNamespace(batch=b)
        def set_batch(self, t, a, v, y):
            assert all(isinstance(x, Rows) for x in (t, a, v, y)); log.append(("set", self.cfg.batch, int(y.idx[0])))
        def stage_batch(self, t, a, v, y):
            assert all(isinstance(x, Rows) for x in (t, a, v, y)); log.append(("stage", self.cfg.batch, int(y.idx[0])))
        def commit_batch(self): log.append(("commit", self.cfg.batch))

    engines = {}
    sol = Solver.__new__(Solver)
    sol._engine_for = lambda b, training=True: engines.setdefault(b, FakeEngine(b))
    base = {k: torch.zeros(20, 2, d) for k, d in ((1, 3), (2, 3), (6, 4))}
    base[5] = torch.zeros(20, 1)

    def mk(i, b):
        idx = torch.arange(i, i + b, dtype=torch.int32)
        return (None, Rows(base[1], idx), Rows(base[2], idx), None, None, Rows(base[5], idx), Rows(base[6], idx), None, None, None, None)
    loader = [mk(0, 4), mk(1, 4), mk(2, 4), mk(3, 2)]
    for e, datas in sol._iter_loaded(loader):
        log.append(("step", e.cfg.batch, int(datas[5].idx[0])))
    assert log == [("set", 4, 0), ("step", 4, 0), ("stage", 4, 1), ("commit", 4), ("step", 4, 1), ("stage", 4, 2), ("commit", 4),
                   ("step", 4, 2), ("set", 2, 3), ("step", 2, 3)], log


def test_pipelined_stage1_pass_leaves_a_shuffling_loader_alone(monkeypatch):
    monkeypatch.setenv("MIMRL_EPOCH_PIPE", "1")
    sol = Solver.__new__(Solver)
    sol.world = 1
    sol.engine = SimpleNamespace(cfg=SimpleNamespace(use_graph=1, device_anchors=1, batch=16))
    sol.train_loader = _loader(shuffle=True)
    assert sol._stage1_pass_pipelined(None) is False
    assert sol.train_loader.pass_index == 0
    # ... and so does a loader of another kind once it shows Rows
    sol.train_loader = list(_loader(n=32, shuffle=True))
    assert sol._stage1_pass_pipelined(None) is False


def test_library_exports_the_gather():
    assert hasattr(_lib.load(), "mimrl_op_gather_rows") and "mimrl_op_gather_rows" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "mimrl.h")).read()
    assert re.search(r"\bint mimrl_op_gather_rows\s*\(void\* stream, int n_arrays,", header)
    assert _lib.load().mimrl_abi_version() == 6
