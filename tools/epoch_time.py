"""Diagnostic: wall time of Solver.train epochs (the reference's epoch-ordered schedule: a stage-1 pass over the loader, then a stage-2
pass -- Solver.py:194-247) at cfg2 on synthetic MOSI-sized data, dataset resident in HBM (default) against --host_data (pinned host
memory, one H2D per batch).  usage: python tools/epoch_time.py [n_samples] [epochs] [--shuffle] [--gather-workgroups N] [--materialize]
[--resident-only] [--json PATH]
  --shuffle             pass --shuffle to the runner (a fresh permutation every pass; batches reach the engine as data.Rows)
  --gather-workgroups N HipEngine.GATHER_MAX_WORKGROUPS for this run (the max_workgroups of mimrl_op_gather_rows)
  --materialize         HipEngine.GATHER_ROWS = False: Rows batches go through index_select + copy instead of the gather kernel
  --resident-only       skip the --host_data run
  --json PATH           append one JSON line per run to PATH (--tag NAME labels it): profiles/shuffle_epoch.json is made of these"""
import argparse, json, os, sys, time, torch
sys.path.insert(0, os.getcwd())
from mimrl_amd import Parameters
from mimrl_amd.Solver import Solver
from mimrl_amd.data import get_data_loader
from mimrl_amd.engine import HipEngine

ap = argparse.ArgumentParser()
ap.add_argument("n", nargs="?", default="1284")
ap.add_argument("epochs", nargs="?", type=int, default=6)
ap.add_argument("--shuffle", action="store_true")
ap.add_argument("--gather-workgroups", type=int, default=None)
ap.add_argument("--materialize", action="store_true")
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
for host in (False,) if a.resident_only else (False, True):
    opt = Parameters.parse_args(argv + (["--host_data"] if host else []))
    opt.seed, opt.save_best_features = 0, False
    sol = Solver(opt, get_data_loader(opt))
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
                                 "ms_per_pair_median": round(1e3 * sorted(ts[2:])[len(ts[2:]) // 2] / nb, 4)}) + "\n")
