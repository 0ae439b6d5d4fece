"""A/B of the task-loss kinds (--loss): the captured combined two-stage step at configs[1] (bench workload cfg2: B = 128, T = 50, bf16,
stage-2 prefetch, device-drawn anchors; the stage boundary -- and with it the task loss -- inside the critic clip + Adam launch) with each
kind, in alternating fresh child processes.  Prints one JSON line per child and a summary line (median ms per step per kind, and each kind's
median minus MAE's in us).

    python tools/task_loss_ab.py [--rounds 3] [--steps 200] [--warmup 20] [--out profiles/task_loss_ab.json]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = ["MAE", "MSE", "RMSE", "SIMSE", "CCC"]


def child(kind, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    from tests.test_gpu_step import _bench_engine
    from mimrl_amd import _lib
    opt, N, batch, banks, eng = _bench_engine("cfg2", "bf16", True, dropout=0.1)
    eng.set_task_loss(_lib.TASK_LOSSES[kind])
    eng.set_stage2_prefetch(1)
    for _ in range(warmup):
        eng.step()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(steps):
        eng.step()
    t1.record()
    torch.cuda.synchronize()
    s = eng.read_scalars()
    ok = bool(all(map(lambda x: x == x, s[:64])))
    eng.close()
    print(json.dumps({"kind": kind, "ms_per_step": t0.elapsed_time(t1) / steps, "steps": steps, "task": float(s[_lib.S2_TASK]), "finite": ok}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.steps, a.warmup)
    runs = []
    for r in range(a.rounds):
        for kind in (KINDS if r % 2 == 0 else KINDS[::-1]):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", kind, "--steps", str(a.steps), "--warmup", str(a.warmup)],
                               capture_output=True, text=True, timeout=600, cwd=ROOT)
            if p.returncode != 0:
                sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
                sys.exit(p.returncode if p.returncode > 0 else 1)   # a failed child ends the A/B: nothing more is started
            line = json.loads(p.stdout.strip().splitlines()[-1])
            line["round"] = r
            print(json.dumps(line), flush=True)
            runs.append(line)
    med = {k: statistics.median(x["ms_per_step"] for x in runs if x["kind"] == k) for k in KINDS}
    summary = {"workload": "cfg2 bf16 captured combined step", "rounds": a.rounds, "steps": a.steps, "median_ms": med,
               "delta_vs_mae_us": {k: 1e3 * (med[k] - med["MAE"]) for k in KINDS[1:]}}
    print(json.dumps(summary))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"runs": runs, "summary": summary}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
