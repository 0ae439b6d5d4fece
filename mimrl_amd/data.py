"""Synthetic MOSI/MOSEI-shaped loader (the datasets, BERT weights and DataLoaderLocal are not shipped; SURVEY.md
section 0 item 8).  Batches use the reference's ``mosi_Dec`` 11-tuple layout (Customization.py:46, Solver.py:273-275)
with one substitution: slot 6 (``bert_sentences``) carries the precomputed BERT last-hidden-state features
[B,T,d_t] instead of token ids -- BERT itself is outside the hot path."""
import logging

import torch

from . import synth


class Rows:
    """Rows ``idx`` of a dataset tensor ``base`` [N, ...] that have not been gathered yet: what a shuffling loader yields in place of a
    batch tensor.  ``idx`` is an int32 tensor of row numbers on ``base``'s device.  HipEngine.set_batch / stage_batch gather such a
    batch straight into an input set (mimrl_op_gather_rows); ``materialize()`` is the plain tensor for everybody else."""
    __slots__ = ("base", "idx")

    def __init__(self, base, idx):
        self.base, self.idx = base, idx

    def __len__(self):
        return len(self.idx)

    def materialize(self):
        return self.base.index_select(0, self.idx)


def plain(x):
    """``x`` as a tensor: a ``Rows`` is gathered, anything else is handed back."""
    return x.materialize() if isinstance(x, Rows) else x


def _mix64(x):
    x = (x + 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF                     # splitmix64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & 0xFFFFFFFFFFFFFFFF
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 31)


class SyntheticLoader:
    """In-memory loader.  ``rank``/``world`` shard the samples by stride (rank, rank+world, ...) the way a
    DistributedSampler would, so that data-parallel replicas see disjoint data; a sharded loader always drops the ragged
    tail so that every rank runs the same number of (full) batches and collectives stay matched.  ``drop_last=False`` (the
    reference's default, Parameters.py:21) yields a shorter last batch.

    ``shuffle=True`` (the reference's training loaders, DataLoaderUniversal.py:25-85): every ``__iter__`` call draws a new permutation of
    this loader's own samples and yields ``Rows`` (row numbers into the resident arrays) in slots 1, 2, 5 and 6 instead of slices.  The
    permutation of a pass is ``torch.randperm`` under a generator seeded from (seed, rank, pass_index) -- ``pass_index`` counts the
    ``__iter__`` calls -- so the order is a pure function of those three numbers (``permutation``); no global RNG is touched.  Under
    ``world > 1`` each rank permutes ITS OWN shard: the sharding stays static, samples never move between ranks.  ``state()`` /
    ``load_state()`` carry ``pass_index`` through a checkpoint."""

    def __init__(self, n, batch_size, T, d_t=768, d_a=74, d_v=35, seed=0, drop_last=False, device=None, ragged=False,
                 rank=0, world=1, pin=False, num_class=None, shuffle=False):
        t, a, v, y = synth.synthetic_batch(n, T, d_t, d_a, d_v, seed=seed, ragged=ragged)
        if num_class is not None:           # --task classification: class indices derived from the regression label
            y = synth.class_labels(y, num_class)
        if world > 1:
            per = n // world
            t, a, v, y = (x[rank::world][:per] for x in (t, a, v, y))
            drop_last = True
        mk = lambda x: torch.from_numpy(x.copy()).to(device) if device else (torch.from_numpy(x.copy()).pin_memory() if pin else torch.from_numpy(x.copy()))
        self.t, self.a, self.v, self.y = mk(t), mk(a), mk(v), mk(y)
        self.n, self.bs, self.drop_last, self.T = int(self.y.shape[0]), batch_size, drop_last, T
        self.shuffle, self.seed, self.rank, self.pass_index = bool(shuffle), int(seed), int(rank), 0

    def __len__(self):
        return self.n // self.bs if self.drop_last else (self.n + self.bs - 1) // self.bs

    def num_samples(self):
        return len(self) * self.bs if self.drop_last else self.n

    def permutation(self, pass_index):
        """The order of pass ``pass_index`` of a shuffling loader (host int64 tensor, a permutation of range(n))."""
        g = torch.Generator()
        g.manual_seed(_mix64(_mix64(_mix64(self.seed & 0xFFFFFFFFFFFFFFFF) ^ self.rank) ^ int(pass_index)) >> 1)
        return torch.randperm(self.n, generator=g)

    def state(self):
        return {"pass_index": int(self.pass_index)}

    def load_state(self, d):
        self.pass_index = int(d["pass_index"])

    def __iter__(self):
        if self.shuffle:
            return self._iter_shuffled()
        return self._iter_slices()

    def _iter_slices(self):
        for i in range(len(self)):
            s = slice(i * self.bs, min((i + 1) * self.bs, self.n))
            B = s.stop - s.start
            ones = torch.ones(B, self.T, dtype=torch.long)
            yield (None, self.a[s], self.v[s], None, None, self.y[s].reshape(-1, 1), self.t[s], torch.zeros_like(ones), ones,
                   None, None)

    def _iter_shuffled(self):
        # (the permutation is drawn and the pass counted when iter() is called, not at the first next())
        perm = self.permutation(self.pass_index).to(torch.int32)
        self.pass_index += 1
        perm = perm.to(self.y.device)                    # one upload per pass; a batch's row numbers are a slice of it
        y = self.y.reshape(-1, 1)

        def batches():
            for i in range(len(self)):
                idx = perm[i * self.bs:min((i + 1) * self.bs, self.n)]
                ones = torch.ones(len(idx), self.T, dtype=torch.long)
                yield (None, Rows(self.a, idx), Rows(self.v, idx), None, None, Rows(y, idx), Rows(self.t, idx), torch.zeros_like(ones),
                       ones, None, None)
        return batches()


def get_data_loader(opt, rank=0, world=1):
    """-> (train, valid, test, d_t, d_a, d_v) like DataLoaderUniversal.get_data_loader (DataLoaderUniversal.py:10-95).
    Only synthetic data exists here: ``--dataset synthetic`` is the honest name; the reference's ``mosi_Dec`` / ``mosei_Dec``
    names are accepted (they select the 'Dec' batch layout) but produce SYNTHETIC data too, and say so loudly.
    The training set is sharded over data-parallel ranks; valid / test are replicated (every rank evaluates all of it)."""
    if opt.dataset not in ("synthetic", "mosi_Dec", "mosei_Dec"):
        raise NotImplementedError(f"--dataset {opt.dataset}: only synthetic MOSI/MOSEI-shaped data is available "
                                  f"(the reference's pickles and DataLoaderLocal are not shipped)")
    if opt.dataset != "synthetic":
        logging.warning("--dataset %s: the %s pickles are not shipped; training on SYNTHETIC %s-shaped random triples "
                        "(scores are NOT dataset results). Use --dataset synthetic to silence this.", opt.dataset,
                        opt.dataset, opt.dataset.split("_")[0])
    n = int(getattr(opt, "synthetic_n", 1284))
    d_t, d_a, d_v = int(getattr(opt, "d_t", 768)), int(getattr(opt, "d_a", 74)), int(getattr(opt, "d_v", 35))
    drop = bool(getattr(opt, "drop_last", False))
    pin = torch.cuda.is_available()
    # 288 GB of HBM: MOSI-sized features are 0.2 GB, MOSEI-sized 2.9 GB -- the whole dataset lives on the device and a batch is a
    # device-to-device slice copy on the upload stream (no PCIe on the step path) unless --host_data or it would not fit
    device = None
    if pin and not getattr(opt, "host_data", False):
        need = 1.5 * n * opt.time_len * (d_t + d_a + d_v) * 4
        if need < 0.25 * torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory:
            device = torch.device("cuda", torch.cuda.current_device())
    k = int(getattr(opt, "k_neighbor", 2))
    ncls = int(getattr(opt, "num_class", 1)) if getattr(opt, "task", "regression") == "classification" else None

    def mk(m, seed, r, w, shuffle=False):
        if 0 < m % opt.batch_size < k:      # a last batch with fewer than k_neighbor rows has no kNN product sample (the
            m -= m % opt.batch_size          # reference's sklearn call raises on it, Model.py:85-86): do not generate one
        return SyntheticLoader(m, opt.batch_size, opt.time_len, d_t, d_a, d_v, seed=seed, drop_last=drop, rank=r, world=w, pin=pin,
                               device=device, num_class=ncls, shuffle=shuffle)

    # --shuffle: the TRAINING loader only, like the reference (DataLoaderUniversal.py: shuffle=True on the train split alone)
    return (mk(n, opt.seed, rank, world, bool(getattr(opt, "shuffle", False))), mk(max(n // 6, opt.batch_size), opt.seed + 1, 0, 1),
            mk(max(n // 3, opt.batch_size), opt.seed + 2, 0, 1), d_t, d_a, d_v)
