"""Loaders: synthetic MOSI/MOSEI-shaped data (the datasets, BERT weights and DataLoaderLocal are not shipped; SURVEY.md
section 0 item 8) and a user's own dataset from a packed file (``--data_file``: ``load_packed`` / ``PackedLoader``).
Batches use the reference's ``mosi_Dec`` 11-tuple layout (Customization.py:46, Solver.py:273-275) with one substitution: slot 6 (``bert_sentences``) carries the precomputed BERT last-hidden-state features
[B,T,d_t] instead of token ids -- BERT itself is outside the hot path."""
import logging

import numpy as np
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


class Packed(Rows):
    """Samples ``idx`` of a PACKED modality that have not been padded yet: ``base`` [F, d] holds the frames of all samples back to back,
    sample i owns the ``length[i]`` (int32 [N]) frames from frame ``start[i]`` (int64 [N]) on.  A batch is [len(idx), T, d]: every sample's
    first min(length, T) frames, then zero rows.  HipEngine pads such a batch straight into an input set (mimrl_op_gather_packed);
    ``materialize()`` is the same tensor in plain torch, on whichever device the four tensors share."""
    __slots__ = ("start", "length", "T")

    def __init__(self, base, start, length, idx, T):
        super().__init__(base, idx)
        self.start, self.length, self.T = start, length, int(T)

    def materialize(self, out=None):
        n, T, d = len(self.idx), self.T, int(self.base.shape[1])
        if out is None:
            out = torch.empty(n, T, d, dtype=self.base.dtype, device=self.base.device)
        if self.base.shape[0] == 0 or n == 0:
            return out.zero_()
        ix = self.idx.long()
        t = torch.arange(T, device=ix.device)
        real = t[None, :] < self.length.index_select(0, ix)[:, None]                     # [n, T]: a frame of the sample, not padding
        frame = torch.where(real, self.start.index_select(0, ix)[:, None] + t[None, :], torch.zeros((), dtype=torch.int64, device=ix.device))
        torch.index_select(self.base, 0, frame.reshape(-1), out=out.view(n * T, d))
        return out.masked_fill_(~real[:, :, None], 0.0)


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


SPLITS = ("train", "valid", "test")
MODALITIES = ("text", "audio", "video")
PACKED_FORMAT = 1


def pack_padded(x):
    """Padded [N, T, d] (numpy or tensor) -> (frames float32 [F, d], length int32 [N]).  A sample's length is the index of its last
    non-zero row + 1 (the engine's own rule for a padded batch), so a zero row INSIDE a sample stays a frame."""
    x = np.asarray(x.detach().cpu() if torch.is_tensor(x) else x, dtype=np.float32)
    if x.ndim != 3:
        raise ValueError(f"pack_padded: a padded [N, T, d] array is needed, got shape {x.shape}")
    N, T, d = x.shape
    nz = (x != 0).any(axis=2)                                                            # [N, T]
    length = np.where(nz.any(axis=1), T - np.argmax(nz[:, ::-1], axis=1), 0).astype(np.int32)
    keep = np.arange(T)[None, :] < length[:, None]
    return np.ascontiguousarray(x[keep].reshape(-1, d)), length


def save_packed(path, splits):
    """Write a packed dataset file (README, "Datasets").  ``splits``: {"train" | "valid" | "test": {"text": frames [F_t, d_t], "audio":
    frames, "video": frames, "len": int [N, 3] (frames per sample in text, audio, video), "y": [N], optionally "y_class": int [N]}}."""
    out = {"format": np.asarray(PACKED_FORMAT, dtype=np.int32)}
    for s in SPLITS:
        sp = splits[s]
        for m in MODALITIES:
            out[f"{s}_{m}"] = np.ascontiguousarray(np.asarray(sp[m], dtype=np.float32))
        out[f"{s}_len"] = np.ascontiguousarray(np.asarray(sp["len"], dtype=np.int32))
        out[f"{s}_y"] = np.asarray(sp["y"], dtype=np.float32).reshape(-1)
        if sp.get("y_class") is not None:
            out[f"{s}_y_class"] = np.asarray(sp["y_class"], dtype=np.int64).reshape(-1)
    with open(path, "wb") as fh:
        np.savez(fh, **out)


def load_packed(path):
    """Read and check a packed dataset file -> {split: {"text" | "audio" | "video": float32 [F, d], "len": int32 [N, 3], "y": float32 [N],
    "y_class": int64 [N] or None}}.  Everything a loader could not honour is refused here, by name."""
    with np.load(path, allow_pickle=False) as z:
        if "format" not in z.files or int(np.asarray(z["format"]).reshape(-1)[0]) != PACKED_FORMAT:
            got = int(np.asarray(z["format"]).reshape(-1)[0]) if "format" in z.files else None
            raise ValueError(f"{path}: 'format' is {got}, this build reads packed format {PACKED_FORMAT}")
        out = {}
        for s in SPLITS:
            need = [f"{s}_{k}" for k in MODALITIES + ("len", "y")]
            missing = [k for k in need if k not in z.files]
            if missing:
                raise ValueError(f"{path}: missing {', '.join(missing)}")
            sp = {m: np.ascontiguousarray(z[f"{s}_{m}"], dtype=np.float32) for m in MODALITIES}
            sp["len"] = np.ascontiguousarray(z[f"{s}_len"]).astype(np.int64)
            sp["y"] = np.ascontiguousarray(z[f"{s}_y"], dtype=np.float32).reshape(-1)
            sp["y_class"] = np.ascontiguousarray(z[f"{s}_y_class"]).astype(np.int64).reshape(-1) if f"{s}_y_class" in z.files else None
            out[s] = sp
    for s, sp in out.items():
        N = len(sp["y"])
        if sp["len"].ndim != 2 or sp["len"].shape != (N, 3):
            raise ValueError(f"{path}: {s}_len has shape {sp['len'].shape}, [N, 3] with N = len({s}_y) = {N} is needed")
        if (sp["len"] < 0).any():
            raise ValueError(f"{path}: {s}_len has a negative entry")
        if sp["y_class"] is not None and len(sp["y_class"]) != N:
            raise ValueError(f"{path}: {s}_y_class has {len(sp['y_class'])} entries, {s}_y has {N}")
        for k, m in enumerate(MODALITIES):
            if sp[m].ndim != 2 or sp[m].shape[1] < 1:
                raise ValueError(f"{path}: {s}_{m} has shape {sp[m].shape}, frames [F, d] are needed")
            if int(sp["len"][:, k].sum()) != sp[m].shape[0]:
                raise ValueError(f"{path}: {s}_len sums to {int(sp['len'][:, k].sum())} {m} frames, {s}_{m} holds {sp[m].shape[0]}")
            if sp[m].shape[1] != out["train"][m].shape[1]:
                raise ValueError(f"{path}: {s}_{m} is {sp[m].shape[1]} wide, train_{m} is {out['train'][m].shape[1]} wide: feature widths "
                                 f"differ between splits")
        sp["len"] = sp["len"].astype(np.int32)
    return out


def _starts(length):
    """First frame of every sample (int64 [N]) from the frames per sample."""
    st = np.zeros(len(length), dtype=np.int64)
    np.cumsum(length[:-1], out=st[1:])
    return st


def _select(frames, length, keep, T=None):
    """Re-pack: the samples ``keep`` (row numbers) of a packed modality, each cut to its first ``T`` frames -> (frames, length)."""
    start = _starts(length)[keep]
    ln = length[keep].astype(np.int64)
    if T is not None:
        ln = np.minimum(ln, T)
    total = int(ln.sum())
    own = np.repeat(np.arange(len(ln)), ln)                                              # the sample of every kept frame
    src = np.arange(total, dtype=np.int64) - np.repeat(_starts(ln), ln) + start[own]
    return np.ascontiguousarray(frames[src]), ln.astype(np.int32)


def prepare_packed(sp, T, normalize=(False, False, False), name="split"):
    """The load-time transforms of one split, in this order: non-finite features -> 0 (DataLoaderCMUSDK.py:93); samples longer than ``T``
    keep their first ``T`` frames; ``normalize[m]``: x -> 2 (x - min) / (max - min) - 1 over the split's remaining frames of modality m
    (DataLoaderCMUSDK.py:104-112; real frames only: there is no padding to pull the minimum to zero).  -> (split, truncated per modality)."""
    out, cut = dict(sp), []
    everyone = np.arange(len(sp["y"]))
    lens = []
    for k, m in enumerate(MODALITIES):
        x, ln = sp[m], sp["len"][:, k]
        if not np.isfinite(x).all():
            x = np.where(np.isfinite(x), x, np.float32(0.0))
        cut.append(int((ln > T).sum()))
        if cut[-1]:
            x, ln = _select(x, ln, everyone, T)
        if normalize[k]:
            if x.shape[0] == 0 or float(x.max()) == float(x.min()):
                raise ValueError(f"--normalize: the {m} frames of the {name} split are constant (or there are none): max - min = 0")
            lo, hi = np.float32(x.min()), np.float32(x.max())
            x = (np.float32(2.0) * (x - lo) / (hi - lo) - np.float32(1.0)).astype(np.float32)
        out[m] = np.ascontiguousarray(x, dtype=np.float32)
        lens.append(ln.astype(np.int32))
    out["len"] = np.stack(lens, axis=1)
    return out, cut


class PackedLoader:
    """Loader over one split of a packed dataset (``prepare_packed``'s output), with ``SyntheticLoader``'s surface.  Every batch is the
    'Dec' 11-tuple with ``Packed`` in slots 1, 2 and 6 and ``Rows`` labels in slot 5, all four over ONE int32 tensor of sample numbers:
    slices of an ``arange`` made once, or -- ``shuffle=True`` -- of the pass's permutation, drawn by ``SyntheticLoader.permutation``'s
    (seed, rank, pass_index) rule.  ``rank`` / ``world`` keep samples rank, rank + world, ... (the first n // world of them), re-packed on
    the host, and drop the ragged tail.  ``labels``: "y", or "y_class" (--task classification: the class indices as floats)."""

    def __init__(self, split, batch_size, T, seed=0, drop_last=False, device=None, rank=0, world=1, pin=False, shuffle=False, labels="y",
                 k_neighbor=0):
        n = len(split["y"])
        keep = np.arange(n)
        if world > 1:
            keep = keep[rank::world][:n // world]
            drop_last = True
        if 0 < len(keep) % batch_size < k_neighbor:     # (get_data_loader: a last batch with fewer than k_neighbor rows is not produced)
            keep = keep[:len(keep) - len(keep) % batch_size]
        y = np.asarray(split[labels], dtype=np.float32).reshape(-1)[keep]
        put = lambda x: x.to(device) if device else (x.pin_memory() if pin else x)
        mk = lambda x: put(torch.from_numpy(np.ascontiguousarray(x)))
        self.base, self.start, self.length = {}, {}, {}
        for k, m in enumerate(MODALITIES):
            frames, ln = split[m], split["len"][:, k]
            if len(keep) != n:
                frames, ln = _select(frames, ln, keep)
            self.base[m], self.start[m], self.length[m] = mk(frames), mk(_starts(ln)), mk(ln.astype(np.int32))
        self.y = mk(y)
        self.n, self.bs, self.drop_last, self.T = int(len(keep)), int(batch_size), bool(drop_last), int(T)
        self.shuffle, self.seed, self.rank, self.pass_index = bool(shuffle), int(seed), int(rank), 0
        self._arange = put(torch.arange(self.n, dtype=torch.int32))

    __len__ = SyntheticLoader.__len__
    num_samples = SyntheticLoader.num_samples
    permutation = SyntheticLoader.permutation
    state = SyntheticLoader.state
    load_state = SyntheticLoader.load_state

    def packed_bytes(self):
        """Bytes this loader keeps resident: frames, starts, lengths and labels."""
        return int(sum(x.numel() * x.element_size() for d in (self.base, self.start, self.length) for x in d.values()) +
                   self.y.numel() * self.y.element_size())

    def __iter__(self):
        # (as in SyntheticLoader: the permutation is drawn and the pass counted when iter() is called)
        order = self._arange
        if self.shuffle:
            order = self.permutation(self.pass_index).to(torch.int32).to(self.y.device)
            self.pass_index += 1
        y = self.y.reshape(-1, 1)

        def batches():
            for i in range(len(self)):
                idx = order[i * self.bs:min((i + 1) * self.bs, self.n)]
                ones = torch.ones(len(idx), self.T, dtype=torch.long)
                a, v, t = (Packed(self.base[m], self.start[m], self.length[m], idx, self.T) for m in ("audio", "video", "text"))
                yield (None, a, v, None, None, Rows(y, idx), t, torch.zeros_like(ones), ones, None, None)
        return batches()


def _packed_loaders(opt, rank, world):
    """get_data_loader under --data_file."""
    path = opt.data_file
    if any(getattr(opt, "log_scale", ())):
        raise NotImplementedError("--log_scale with --data_file: it needs the reference's per-dataset minimum tables, which a packed file does "
                                  "not carry; apply it before packing")
    splits = load_packed(path)
    classify = getattr(opt, "task", "regression") == "classification"
    if classify:
        C = max(int(getattr(opt, "num_class", 1)), 2) if getattr(opt, "loss", "CE") == "BCE" else int(getattr(opt, "num_class", 1))
        for s, sp in splits.items():
            if sp["y_class"] is None:
                raise ValueError(f"{path}: --task classification needs {s}_y_class")
            if len(sp["y_class"]) and (int(sp["y_class"].min()) < 0 or int(sp["y_class"].max()) >= C):
                raise ValueError(f"{path}: {s}_y_class has a class index outside [0, {C})")
    T = int(opt.time_len)
    norm = tuple(bool(x) for x in getattr(opt, "normalize", (False, False, False)))
    cuts = {}
    for s in SPLITS:
        splits[s], cut = prepare_packed(splits[s], T, norm, name=s)
        if any(cut):
            cuts[s] = cut
    if cuts:
        logging.warning("--data_file %s: samples longer than --time_len %d keep their first %d frames (text/audio/video samples cut: %s)",
                        path, T, T, ", ".join(f"{s} {c[0]}/{c[1]}/{c[2]}" for s, c in cuts.items()))
    d_t, d_a, d_v = (int(splits["train"][m].shape[1]) for m in MODALITIES)
    pin = torch.cuda.is_available()
    device = None
    if pin and not getattr(opt, "host_data", False):
        need = 1.5 * sum(sp[m].nbytes for sp in splits.values() for m in MODALITIES)
        if need < 0.25 * torch.cuda.get_device_properties(torch.cuda.current_device()).total_memory:
            device = torch.device("cuda", torch.cuda.current_device())
    k = int(getattr(opt, "k_neighbor", 2))
    drop = bool(getattr(opt, "drop_last", False))

    def mk(s, seed, r, w, shuffle=False):
        return PackedLoader(splits[s], opt.batch_size, T, seed=seed, drop_last=drop, device=device, rank=r, world=w, pin=pin,
                            shuffle=shuffle, labels="y_class" if classify else "y", k_neighbor=k)
    return (mk("train", opt.seed, rank, world, bool(getattr(opt, "shuffle", False))), mk("valid", opt.seed + 1, 0, 1),
            mk("test", opt.seed + 2, 0, 1), d_t, d_a, d_v)


def get_data_loader(opt, rank=0, world=1):
    """-> (train, valid, test, d_t, d_a, d_v) like DataLoaderUniversal.get_data_loader (DataLoaderUniversal.py:10-95).
    ``--data_file PATH`` trains on the packed dataset file PATH (``load_packed``; d_t, d_a, d_v come from the file, --normalize is applied,
    samples are cut to --time_len).  Without it only synthetic data exists here: ``--dataset synthetic`` is the honest name; the reference's ``mosi_Dec`` / ``mosei_Dec``
    names are accepted (they select the 'Dec' batch layout) but produce SYNTHETIC data too, and say so loudly.
    The training set is sharded over data-parallel ranks; valid / test are replicated (every rank evaluates all of it)."""
    if opt.dataset not in ("synthetic", "mosi_Dec", "mosei_Dec"):
        raise NotImplementedError(f"--dataset {opt.dataset}: only synthetic MOSI/MOSEI-shaped data is available "
                                  f"(the reference's pickles and DataLoaderLocal are not shipped)")
    if getattr(opt, "data_file", ""):       # the user's own dataset, whichever of the three names selects the 'Dec' batch layout
        return _packed_loaders(opt, rank, world)
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
