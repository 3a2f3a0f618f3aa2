"""KL control on one GPU: what the gated optimizer
step costs the flagship PPO loop (65,536 envs, T = 32, batch 65,536, 10
epochs: 320 optimizer steps per iteration).

  python scripts/kl_bench.py [--rounds 3] [--parent-root DIR]

Cases, each in a fresh process, alternating over --rounds rounds on one box:

  parent     the parent commit's package (--parent-root DIR: a checkout of it
             with its library built), every setting absent
  off        this tree, every setting at its default (the parent's launches)
  target     target_kl = 1e9: the gate in every step, never trips, one
             readback of the steps taken per iteration
  adaptive   lr_schedule = "adaptive": the gate in every step, no readback

"off" must lie inside the parent's min-max range widened by that range's width
(DESIGN.md section 20's rule); the summary line says whether it does.  The
gated cases are reported as measured; readback_ms_per_iter is the host time
spent waiting for the steps-taken word per iteration (it waits for the
training work enqueued one rollout earlier).

One JSON line per measurement and a summary line; printed, and written to
--out (default profiles/kl_bench.jsonl)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=12, help="timed PPO iterations per process")
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "kl_bench.jsonl"))
ap.add_argument("--mode", choices=["all", "ppo"], default="all")
ap.add_argument("--root", default=ROOT, help="--mode ppo: the tree whose package is measured")
ap.add_argument("--case", choices=["parent", "off", "target", "adaptive"], default="off")
a = ap.parse_args()

SETTINGS = {"parent": {}, "off": {}, "target": dict(target_kl=1e9),
            "adaptive": dict(lr_schedule="adaptive")}


def measure_ppo():
    import time

    import torch
    sys.path.insert(0, a.root)
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    tr = PPOTrainer(PPOConfig(num_envs=a.envs, n_steps=32, batch_size=65536, n_epochs=10,
                              seed=0, **SETTINGS[a.case]))
    wait = [0.0]
    if a.case == "target":
        taken = tr._kl_taken

        def timed():
            t = time.perf_counter()
            n = taken()
            wait[0] += time.perf_counter() - t
            return n

        tr._kl_taken = timed
    for _ in range(a.warmup):
        tr.learn_step()
    torch.cuda.synchronize()
    wait[0] = 0.0
    t0 = time.perf_counter()
    for _ in range(a.iters):
        tr.learn_step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    es = tr.episode_stats()
    out = {"what": "ppo", "case": a.case, "iters": a.iters,
           "updates_per_s": round(a.iters / dt, 4),
           "env_steps_per_s": round(a.iters * a.envs * 32 / dt, 1),
           "ep_rew_mean": round(es["ep_rew_mean"], 3)}
    if a.case != "parent":
        out.update(n_updates_taken=es["n_updates_taken"], lr=es["lr"])
    if a.case == "target":
        out["readback_ms_per_iter"] = round(wait[0] / a.iters * 1e3, 4)
    tr.close()
    return out


def child(args):
    """A fresh process per measurement (no state shared between the cases)."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} failed with {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


if a.mode == "ppo":
    print(json.dumps(measure_ppo()), flush=True)
else:
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    common = ["--envs", str(a.envs), "--iters", str(a.iters), "--warmup", str(a.warmup)]
    cases = [("off", ROOT), ("target", ROOT), ("adaptive", ROOT)]
    if a.parent_root:
        cases.insert(0, ("parent", os.path.abspath(a.parent_root)))
    rates = {name: [] for name, _ in cases}
    waits = []
    for rnd in range(a.rounds):
        for name, root in cases:
            r = child(["--mode", "ppo", "--root", root, "--case", name] + common)
            r.update(round=rnd)
            rates[name].append(r["updates_per_s"])
            if "readback_ms_per_iter" in r:
                waits.append(r["readback_ms_per_iter"])
            emit(r)
    med = {k: statistics.median(v) for k, v in rates.items()}
    summary = {"what": "summary", "envs": a.envs, "rounds": a.rounds,
               "updates_per_s_median": {k: round(v, 4) for k, v in med.items()},
               "updates_per_s_range": {k: [min(v), max(v)] for k, v in rates.items()},
               "target_over_off": round(med["target"] / med["off"], 4),
               "adaptive_over_off": round(med["adaptive"] / med["off"], 4),
               "readback_ms_per_iter_median": round(statistics.median(waits), 4)}
    if "parent" in med:
        lo, hi = min(rates["parent"]), max(rates["parent"])
        summary["off_over_parent"] = round(med["off"] / med["parent"], 4)
        summary["parent_range_widened"] = [round(lo - (hi - lo), 4), round(hi + (hi - lo), 4)]
        summary["off_within_parent_range"] = bool(
            lo - (hi - lo) <= min(rates["off"]) and max(rates["off"]) <= hi + (hi - lo))
    emit(summary)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
