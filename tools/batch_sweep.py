"""Batch-size sweep of one GPU: ms per captured two-stage step and samples/s at the bench workload's shape (cfg2: T = 50, MOSI-sized banks,
bf16, stage-2 prefetch, device-drawn anchors) with the per-rank batch B in {128, 512, 1024, 2048}, separable critic.  The concat critic
only reports its workspace at its ceiling (MIMRL_MAX_BATCH_CONCAT = 1024: created, not stepped) and its refusal at 2048.  Each point
runs in a fresh child process.  Prints one JSON line per
point and writes them all to --out.

    python tools/batch_sweep.py [--steps 50] [--warmup 10] [--out profiles/batch_sweep.json]
"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POINTS = [("separate", 128), ("separate", 512), ("separate", 1024), ("separate", 2048), ("concat", 1024), ("concat", 2048)]


def child(critic, B, steps, warmup):
    sys.path.insert(0, ROOT)
    import torch
    import bench
    from mimrl_amd import _lib, synth
    from mimrl_amd.engine import HipEngine
    opt, N = bench.workload("cfg2")
    opt.batch_size, opt.critic_type = B, critic
    T = opt.time_len
    try:
        eng = HipEngine(opt, 768, 74, 35, seq_len=T, bank_capacity=N, precision="bf16", use_graph=True, seed=1, device_anchors=True)
    except _lib.MimrlError as e:
        print(json.dumps({"critic": critic, "B": B, "refused": str(e)}))
        return
    if critic == "concat":
        print(json.dumps({"critic": critic, "B": B, "workspace_bytes": int(eng.workspace_bytes())}))
        eng.close()
        return
    eng.load_params(synth.default_state([(n, tuple(v.shape)) for n, v in eng.params.items()], 0))
    eng.set_batch(*synth.synthetic_batch(B, T, seed=0))
    banks = synth.synthetic_banks(N, seed=0)
    eng.set_banks(*(banks[k] for k in "CFTAV"))
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
    ms = t0.elapsed_time(t1) / steps
    line = {"critic": critic, "B": B, "T": T, "N": N, "ms_per_step": ms, "samples_per_s": B / ms * 1e3, "steps": steps,
            "workspace_bytes": int(eng.workspace_bytes()), "s1_loss": float(s[_lib.S1_LOSS]), "s2_loss": float(s[_lib.S2_LOSS]),
            "finite": bool(all(x == x for x in s[:64]))}
    eng.close()
    print(json.dumps(line))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--child", nargs=2, default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], int(a.child[1]), a.steps, a.warmup)
    runs = []
    for critic, B in POINTS:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", critic, str(B), "--steps", str(a.steps), "--warmup",
                            str(a.warmup)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        if p.returncode != 0:
            sys.stderr.write(p.stdout[-2000:] + p.stderr[-2000:])
            sys.exit(p.returncode if p.returncode > 0 else 1)   # a failed child ends the sweep: nothing more is started
        line = json.loads(p.stdout.strip().splitlines()[-1])
        print(json.dumps(line), flush=True)
        runs.append(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        json.dump({"workload": "cfg2 shape, bf16, captured two-stage step, stage-2 prefetch", "runs": runs}, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
