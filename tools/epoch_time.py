"""Diagnostic: wall time of Solver.train epochs (the reference's epoch-ordered schedule: a stage-1 pass over the loader, then a stage-2
pass -- Solver.py:194-247) at cfg2 on synthetic MOSI-sized data, dataset resident in HBM (default) against --host_data (pinned host
memory, one H2D per batch).  usage: python tools/epoch_time.py [n_samples] [epochs] [--shuffle] [--gather-workgroups N] [--materialize]
[--packed MODE] [--resident-only] [--json PATH]
  --shuffle             pass --shuffle to the runner (a fresh permutation every pass; batches reach the engine as data.Rows)
  --gather-workgroups N HipEngine.GATHER_MAX_WORKGROUPS for this run (the max_workgroups of mimrl_op_gather_rows)
  --materialize         HipEngine.GATHER_ROWS = False: Rows batches go through index_select + copy instead of the gather kernel
  --packed MODE         write a seeded PACKED dataset file at the same shape (lengths uniform in [1, T] per sample and modality) and train on it:
                        "file": through --data_file (batches padded by mimrl_op_gather_packed; with --materialize by Packed.materialize());
                        "padded": the same samples padded on the host into resident [N, T, d] arrays (the dense path: slices / gather_rows)
  --resident-only       skip the --host_data run
  --json PATH           append one JSON line per run to PATH (--tag NAME labels it): profiles/shuffle_epoch.json is made of these"""
import argparse, atexit, json, os, shutil, sys, tempfile, time, numpy as np, torch
sys.path.insert(0, os.getcwd())
from mimrl_amd import Parameters
from mimrl_amd.Solver import Solver
from mimrl_amd.data import MODALITIES, Packed, SyntheticLoader, get_data_loader, load_packed, save_packed
from mimrl_amd.engine import HipEngine

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", default="1284")
ap.add_argument("epochs", nargs="?", type=int, default=6)
ap.add_argument("--shuffle", action="store_true")
ap.add_argument("--gather-workgroups", type=int, default=None)
ap.add_argument("--materialize", action="store_true")
ap.add_argument("--packed", choices=["file", "padded"], default=None)
ap.add_argument("--resident-only", action="store_true")
ap.add_argument("--json", default=None)
ap.add_argument("--tag", default=None)
a = ap.parse_args()
n, epochs = a.n, a.epochs
if a.gather_workgroups is not None:
    HipEngine.GATHER_MAX_WORKGROUPS = a.gather_workgroups
if a.materialize:
    HipEngine.GATHER_ROWS = False
argv = ["--dataset", "synthetic", "--synthetic_n", n, "--batch_size", "128", "--time_len", "50", "--d_hiddens", "50-3-128=10-3-128",
        "--d_outs", "50-3-128=10-3-128", "--bias", "--res_project", "1-1", "--dropout", "0.1-0.1-0.1-0.1", "--dropout_mlp", "0.0-0.0-0.0",
        "--loss_mi_coefficient1", "-".join(["1.0"] * 11), "--loss_mi_coefficient2", "-".join(["0.01"] * 8), "--learning_rate", "1e-4",
        "--precision", "bf16", "--task_name", "epoch_time", "--stage1_n", "1"] + (["--shuffle"] if a.shuffle else [])
T, DIMS = 50, (768, 74, 35)


def write_packed(path, n):
    """Train / valid / test of n, n // 6, n // 3 samples (the synthetic loaders' sizes), N(0, 1) frames, U(-3, 3) labels."""
    splits = {}
    for k, (s, m) in enumerate((("train", n), ("valid", max(n // 6, 128)), ("test", max(n // 3, 128)))):
        g = np.random.default_rng([k, n])
        ln = g.integers(1, T + 1, size=(m, 3)).astype(np.int32)
        splits[s] = dict({mod: g.standard_normal((int(ln[:, j].sum()), DIMS[j]), dtype=np.float32) for j, mod in enumerate(MODALITIES)},
                         len=ln, y=g.uniform(-3.0, 3.0, m).astype(np.float32))
    save_packed(path, splits)


def padded_loaders(opt, path):
    """The samples of the packed file as the dense loaders the padded dataset would get: same sizes, seeds and placement rule."""
    pin, dev = torch.cuda.is_available(), None if opt.host_data else torch.device("cuda", torch.cuda.current_device())
    out = []
    for k, (s, sp) in enumerate(load_packed(path).items()):
        ld = SyntheticLoader(2, opt.batch_size, T, 4, 4, 4, seed=opt.seed + k, shuffle=bool(opt.shuffle) and s == "train")
        m = len(sp["y"])
        full = []
        for j, mod in enumerate(MODALITIES):
            ln = torch.from_numpy(sp["len"][:, j].copy())
            full.append(Packed(torch.from_numpy(sp[mod]), torch.cumsum(ln.long(), 0) - ln.long(), ln, torch.arange(m, dtype=torch.int32), T).materialize())
        ld.t, ld.a, ld.v, ld.y = ((x.to(dev) if dev else x.pin_memory()) for x in full + [torch.from_numpy(sp["y"])])
        ld.n = m
        out.append(ld)
    return (*out, *DIMS)


def resident_bytes(loaders):
    return int(sum(ld.packed_bytes() if hasattr(ld, "packed_bytes") else sum(x.numel() * x.element_size() for x in (ld.t, ld.a, ld.v, ld.y))
                   for ld in loaders[:3]))


data_file = None
if a.packed:
    data_file = os.path.join(tempfile.mkdtemp(prefix="epoch_time_"), "packed.npz")
    atexit.register(shutil.rmtree, os.path.dirname(data_file), True)
    write_packed(data_file, int(n))
for host in (False,) if a.resident_only else (False, True):
    opt = Parameters.parse_args(argv + (["--host_data"] if host else []) + (["--data_file", data_file] if a.packed == "file" else []))
    opt.seed, opt.save_best_features = 0, False
    loaders = padded_loaders(opt, data_file) if a.packed == "padded" else get_data_loader(opt)
    sol = Solver(opt, loaders)
    banks = ([], [], [], [], [])
    ts = []
    for ep in range(epochs):
        torch.cuda.synchronize(); t = time.perf_counter()
        r = sol.train(ep, sol.train_loader, *banks)
        torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
        banks = r[4:]
    nb = len(sol.train_loader)
    best = min(ts[2:])
    print("%s data: %d batches/epoch, epoch %.2f ms (best of %d after 2 warm-up epochs) = %.3f ms per batch (stage-1 + stage-2 pass) = %.0f two-stage iterations/s"
          % ("host    " if host else "resident", nb, 1e3 * best, epochs - 2, 1e3 * best / nb, nb / best))
    if a.json:
        with open(a.json, "a") as fh:
            fh.write(json.dumps({"tag": a.tag, "host_data": host, "shuffle": a.shuffle, "materialize": a.materialize,
                                 "gather_workgroups": getattr(HipEngine, "GATHER_MAX_WORKGROUPS", None), "n": int(n), "batches": nb,
                                 "epoch_ms": [round(1e3 * x, 3) for x in ts], "ms_per_pair_best": round(1e3 * best / nb, 4),
                                 "ms_per_pair_median": round(1e3 * sorted(ts[2:])[len(ts[2:]) // 2] / nb, 4), "packed": a.packed,
                                 "resident_bytes": None if host else resident_bytes(loaders)}) + "\n")
