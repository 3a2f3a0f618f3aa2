"""The sensor model on one GPU: what one dr_sensor_step
costs, and what the wrapper costs the PPO loop.

  python scripts/sensor_bench.py [--dim 15] [--rounds 3] [--parent-root DIR]

1. One step at 65,536 and 4,194,304 envs x --dim, delays (0, 0) and (0, 4),
   with the gym columns' noise and bias and 3 % of the envs done per step: the
   kernel's mean time between its dispatch's start and end timestamps (the
   profiler's kernel records), and the back-to-back time per step between two
   device events, eager and replayed from a graph, stated against the
   algorithmic bytes (what the spec has to move per env: the clean row in, a
   ring row written, a ring row read, the row out, 20 bytes of counters) and
   the bytes this implementation moves (it also reads the bias row, and with
   delay_hi = 0 reads no ring row).
2. PPO updates/s of the flagship trainer (65,536 envs, T = 32, batch 65,536,
   10 epochs) with the sensor model on and off, alternating, each in a fresh
   process.  With --parent-root DIR (a checkout of the parent commit with its
   library built) the off case is also measured on the parent's code in the
   same alternation.

One JSON line per measurement and a summary line; printed, and written to
--out (default profiles/sensor_bench.jsonl)."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12           # B/s, MI355X
NOISE, BIAS = (0.02, 0.05, 0.02, 0.1), (0.02, 0.0, 0.01, 0.0)

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, default=65536)
ap.add_argument("--dim", type=int, default=15)
ap.add_argument("--delay", default="0,0")
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=12, help="timed PPO iterations per process")
ap.add_argument("--warmup", type=int, default=4)
ap.add_argument("--parent-root", default=None)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sensor_bench.jsonl"))
ap.add_argument("--mode", choices=["all", "step", "ppo"], default="all")
ap.add_argument("--root", default=ROOT, help="--mode ppo: the tree whose package is measured")
ap.add_argument("--sensor", type=int, default=0)
a = ap.parse_args()


def step_bytes(n, d, delay_hi):
    algorithmic = n * (4 * 4 * d + 20)
    # rows: obs in, ring write, out, the bias row, the ring read unless L = 1;
    # counters: ep, s, d read, s written, the done byte
    moved = n * (4 * d * (5 if delay_hi else 4) + 16 + 1)
    return algorithmic, moved


def measure_step():
    import torch
    sys.path.insert(0, ROOT)
    from drone_rl_amd import ppo_kernels as K
    n, d = a.envs, a.dim
    delay = tuple(int(x) for x in a.delay.split(","))
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(0)
    sets = 4                        # distinct inputs cycled over the launches
    obs = torch.randn(sets, n, d, generator=g, device=dev)
    done = (torch.rand(sets, n, generator=g, device=dev) < 0.03).to(torch.uint8)
    out = torch.empty(n, d, device=dev)
    cols = K.sensor_columns("gym", NOISE, BIAS) if d == 15 else \
        ([0.05] * d, [0.02] * d, [-1] * d)
    sm = K.SensorModel(n, d, dev, columns=cols, delay=delay, seed=1)
    sm.reset(obs[0], out=out)

    def step(i):
        sm.step(obs[i % sets], done[i % sets], obs_out=out)

    for i in range(20):
        step(i)
    torch.cuda.synchronize()
    reps = 2000 if n <= 1 << 20 else 200
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
        for _ in range(reps // 100):
            gr.replay()
        e1.record()
        torch.cuda.synchronize()
        gspans.append(e0.elapsed_time(e1) * 1e3 / (reps // 100 * 100))
    # kernel records: start / end of each dispatch
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(100):
            step(i)
        torch.cuda.synchronize()
    kern = [ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            for ev in prof.events() if "sensor_kernel" in ev.name]
    if not kern:
        raise SystemExit("the profiler returned no record of the step's kernel")
    alg, moved = step_bytes(n, d, delay[1])
    k_us = statistics.mean(kern)
    return {"what": "step", "envs": n, "dim": d, "delay": list(delay),
            "device": torch.cuda.get_device_name(0),
            "kernel_us": round(k_us, 3), "kernel_launches": len(kern),
            "step_us_eager": round(statistics.median(spans), 3),
            "step_us_graph": round(statistics.median(gspans), 3),
            "algorithmic_bytes": alg, "moved_bytes": moved,
            "algorithmic_hbm_us": round(alg / HBM_PEAK * 1e6, 3),
            "hbm_fraction_of_kernel_time": round(alg / HBM_PEAK * 1e6 / k_us, 4),
            "moved_bytes_per_s_of_kernel_time": round(moved / (k_us * 1e-6), 1)}


def measure_ppo():
    import time

    import torch
    sys.path.insert(0, a.root)
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    kw = dict(obs_noise=NOISE, obs_bias=BIAS, obs_delay=(0, 2)) if a.sensor else {}
    tr = PPOTrainer(PPOConfig(num_envs=65536, n_steps=32, batch_size=65536, n_epochs=10,
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
    return {"what": "ppo", "sensor": bool(a.sensor), "iters": a.iters,
            "updates_per_s": round(a.iters / dt, 4),
            "env_steps_per_s": round(a.iters * 65536 * 32 / dt, 1),
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

    common = ["--dim", str(a.dim), "--iters", str(a.iters), "--warmup", str(a.warmup)]
    steps = {}
    for envs in (65536, 4194304):
        for delay in ("0,0", "0,4"):
            st = child(["--mode", "step", "--envs", str(envs), "--delay", delay] + common)
            steps[f"{envs}:{delay}"] = st["kernel_us"]
            emit(st)
    cases = [("off", ROOT, 0), ("on", ROOT, 1)]
    if a.parent_root:
        cases.append(("parent_off", os.path.abspath(a.parent_root), 0))
    rates = {name: [] for name, _, _ in cases}
    for rnd in range(a.rounds):
        # the order rotates with the round: no case always follows the same one
        for name, root, on in cases[rnd % len(cases):] + cases[:rnd % len(cases)]:
            r = child(["--mode", "ppo", "--root", root, "--sensor", str(on)] + common)
            r.update(case=name, round=rnd)
            rates[name].append(r["updates_per_s"])
            emit(r)
    med = {k: statistics.median(v) for k, v in rates.items()}
    summary = {"what": "summary", "rounds": a.rounds,
               "updates_per_s_median": {k: round(v, 4) for k, v in med.items()},
               "updates_per_s_range": {k: [min(v), max(v)] for k, v in rates.items()},
               "on_over_off": round(med["on"] / med["off"], 4), "step_kernel_us": steps}
    if "parent_off" in med:
        summary["off_over_parent_off"] = round(med["off"] / med["parent_off"], 4)
    emit(summary)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
