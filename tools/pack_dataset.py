"""Convert a dataset of PADDED arrays into the packed file that --data_file reads (README, "Datasets").
usage: python tools/pack_dataset.py PADDED.npz PACKED.npz

PADDED.npz holds, for s in train, valid, test: {s}_text [N, T, d_t], {s}_audio [N, T, d_a], {s}_video [N, T, d_v] (float; a sample's
frames first, zero rows behind them -- T may differ between modalities and splits), {s}_y [N] and optionally {s}_y_class [N] (int).
A sample's length in a modality is the index of its last non-zero row + 1 (mimrl_amd.data.pack_padded).  The file is read without pickle."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mimrl_amd.data import MODALITIES, SPLITS, load_packed, pack_padded, save_packed      # noqa: E402


def convert(src, dst):
    splits = {}
    with np.load(src, allow_pickle=False) as z:
        for s in SPLITS:
            sp, lens = {}, []
            for m in MODALITIES:
                sp[m], ln = pack_padded(z[f"{s}_{m}"])
                lens.append(ln)
            if len({len(ln) for ln in lens}) != 1:
                raise ValueError(f"{src}: {s}_text / {s}_audio / {s}_video hold {[len(ln) for ln in lens]} samples")
            sp["len"] = np.stack(lens, axis=1)
            sp["y"] = np.asarray(z[f"{s}_y"], dtype=np.float32).reshape(-1)
            sp["y_class"] = np.asarray(z[f"{s}_y_class"]) if f"{s}_y_class" in z.files else None
            splits[s] = sp
    save_packed(dst, splits)
    return load_packed(dst)                   # (every load-time check, before anybody trains on it)


def main(argv):
    if len(argv) != 2:
        print(__doc__)
        return 2
    out = convert(*argv)
    for s in SPLITS:
        sp = out[s]
        padded = sum(len(sp["y"]) * int(sp["len"][:, k].max(initial=0)) * sp[m].shape[1] * 4 for k, m in enumerate(MODALITIES))
        print("%s: %d samples, %d / %d / %d frames, %.1f MB packed (%.1f MB padded to the longest sample)"
              % (s, len(sp["y"]), *(sp[m].shape[0] for m in MODALITIES), sum(sp[m].nbytes for m in MODALITIES) / 1e6, padded / 1e6))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
