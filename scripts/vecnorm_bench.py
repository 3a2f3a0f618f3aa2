"""VecNormalize on one GPU: what one dr_vecnorm_step
costs, and what the normalisation costs the PPO loop.

  python scripts/vecnorm_bench.py [--envs 65536] [--dim 15] [--rounds 3]
                                  [--parent-root DIR]

1. One training step (partials, finish, normalise) at --envs x --dim: per
   kernel the mean time between its dispatch's start and end timestamps (the
   profiler's kernel records, a run of its own), the three summed, and the
   back-to-back time per step between two device events, stated against the
   algorithmic bytes (what the spec has to move: obs in and out once, rewards
   in and out, dones, returns in and out) and the bytes this implementation
   moves (it reads obs twice: once for the moments, once to normalise).
2. PPO updates/s of the flagship trainer (65,536 envs, T = 32, batch 65,536,
   10 epochs) with both norms on and with both off, alternating, each in a
   fresh process.  With --parent-root DIR (a checkout of the parent commit
   with its library built) the off case is also measured on the parent's code
   in the same alternation.

One JSON line per measurement and a summary line; printed, and written to
--out (default profiles/vecnorm_bench.jsonl)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12           # B/s, MI355X

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--dim", type=int, default=15)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=12, help="timed PPO iterations per process")
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vecnorm_bench.jsonl"))
ap.add_argument("--mode", choices=["all", "step", "ppo"], default="all")
ap.add_argument("--root", default=ROOT, help="--mode ppo: the tree whose package is measured")
ap.add_argument("--normalize", type=int, default=0)
a = ap.parse_args()


def step_bytes(n, d):
    algorithmic = n * (4 * d + 4 * d + 4 + 4 + 1 + 8 + 8)
    moved = algorithmic + n * 4 * d + n * (4 + 1)     # obs, rewards, dones read twice
    return algorithmic, moved


def measure_step():
    import torch
    sys.path.insert(0, ROOT)
    from drone_rl_amd import ppo_kernels as K
    n, d = a.envs, a.dim
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    sets = 4                        # distinct inputs cycled over the launches
    obs = torch.randn(sets, n, d, generator=g, device=dev) * 3.0 + 1.0
    rew = torch.randn(sets, n, generator=g, device=dev)
    done = (torch.rand(sets, n, generator=g, device=dev) < 0.03).to(torch.uint8)
    obs_out, rew_out = torch.empty(n, d, device=dev), torch.empty(n, device=dev)
    vn = K.VecNormalize(n, d, dev)
    vn.reset(obs[0], out=obs_out)

    def step(i):
        vn.step(obs[i % sets], rew[i % sets], done[i % sets], obs_out=obs_out, rew_out=rew_out)

    for i in range(20):
        step(i)
    torch.cuda.synchronize()
    reps = 2000
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spans = []
    for _ in range(5):
        e0.record()
        for i in range(reps):
            step(i)
        e1.record()
        torch.cuda.synchronize()
        spans.append(e0.elapsed_time(e1) * 1e3 / reps)
    # the same steps captured: without the host's launch cost between kernels
    gr = torch.cuda.CUDAGraph()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs), torch.cuda.graph(gr, stream=cs):
        for i in range(100):
            step(i)
    torch.cuda.current_stream().wait_stream(cs)
    gr.replay()
    torch.cuda.synchronize()
    gspans = []
    for _ in range(5):
        e0.record()
        for _ in range(10):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        gspans.append(e0.elapsed_time(e1) * 1e3 / 1000)
    # kernel records: start / end of each dispatch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(200):
            step(i)
        torch.cuda.synchronize()
    kern = {}
    for ev in prof.events():
        key = next((k for k in ("partial", "finish", "apply") if "vecnorm_" + k in ev.name), None)
        if key is not None:
            kern.setdefault(key, []).append(ev.device_time if hasattr(ev, "device_time")
                                            else ev.cuda_time)
    if sorted(kern) != ["apply", "finish", "partial"]:
        raise SystemExit(f"the profiler returned no record of the step's kernels: {sorted(kern)}")
    alg, moved = step_bytes(n, d)
    ks = {k: round(statistics.mean(v), 3) for k, v in kern.items()}
    total = sum(ks.values())
    return {"what": "step", "envs": n, "dim": d, "device": torch.cuda.get_device_name(0),
            "kernel_us": ks, "kernel_us_sum": round(total, 3),
            "kernel_launches": {k: len(v) for k, v in kern.items()},
            "step_us_eager": round(statistics.median(spans), 3),
            "step_us_graph": round(statistics.median(gspans), 3),
            "algorithmic_bytes": alg, "moved_bytes": moved,
            "algorithmic_hbm_us": round(alg / HBM_PEAK * 1e6, 3),
            "hbm_fraction_of_kernel_time": round(alg / HBM_PEAK * 1e6 / total, 4) if total else None}


def measure_ppo():
    import time

    import torch
    sys.path.insert(0, a.root)
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    kw = dict(normalize_obs=True, normalize_reward=True) if a.normalize else {}
    tr = PPOTrainer(PPOConfig(num_envs=a.envs, n_steps=32, batch_size=65536, n_epochs=10,
                              seed=0, **kw))
    for _ in range(a.warmup):
        tr.learn_step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.iters):
        tr.learn_step()
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    es = tr.episode_stats()
    tr.close()
    return {"what": "ppo", "normalize": bool(a.normalize), "iters": a.iters,
            "updates_per_s": round(a.iters / dt, 4),
            "env_steps_per_s": round(a.iters * a.envs * 32 / dt, 1),
            "ep_rew_mean": round(es["ep_rew_mean"], 3)}


def child(args):
    """A fresh process per measurement (no state shared between the cases)."""
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True,
                       text=True, timeout=600)
    if p.returncode != 0:
        sys.stderr.write(p.stdout[-2000:] + p.stderr[-4000:])
        raise SystemExit(f"child {args} failed with {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


if a.mode == "step":
    print(json.dumps(measure_step()), flush=True)
elif a.mode == "ppo":
    print(json.dumps(measure_ppo()), flush=True)
else:
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)

    common = ["--envs", str(a.envs), "--dim", str(a.dim), "--iters", str(a.iters),
              "--warmup", str(a.warmup)]
    st = child(["--mode", "step"] + common)
    emit(st)
    cases = [("off", ROOT, 0), ("on", ROOT, 1)]
    if a.parent_root:
        cases.append(("parent_off", os.path.abspath(a.parent_root), 0))
    rates = {name: [] for name, _, _ in cases}
    for rnd in range(a.rounds):
        for name, root, norm in cases:
            r = child(["--mode", "ppo", "--root", root, "--normalize", str(norm)] + common)
            r.update(case=name, round=rnd)
            rates[name].append(r["updates_per_s"])
            emit(r)
    med = {k: statistics.median(v) for k, v in rates.items()}
    summary = {"what": "summary", "envs": a.envs, "rounds": a.rounds,
               "updates_per_s_median": {k: round(v, 4) for k, v in med.items()},
               "updates_per_s_range": {k: [min(v), max(v)] for k, v in rates.items()},
               "on_over_off": round(med["on"] / med["off"], 4),
               "step_kernel_us_sum": st["kernel_us_sum"], "step_us_graph": st["step_us_graph"]}
    if "parent_off" in med:
        summary["off_over_parent_off"] = round(med["off"] / med["parent_off"], 4)
    emit(summary)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
