"""The MPPI planner on one GPU: what one dr_mppi_step
costs, stated as model env-steps per second (N * S * H per call), beside
dr_rollout_random on N * S gym f64 envs for K = H steps in the same session.
The rollout is the yardstick: the same physics_step, but it writes 65 B per
env-step (obs, reward, done) where the planner writes none inside the horizon.

  python scripts/planner_bench.py [--envs 256,4096] [--samples 256] [--horizon 16]

Per N: the kernel's mean time between its dispatch's start and end timestamps
(the profiler's kernel records), and the time per call between two device
events, eager and replayed from a graph.  One JSON line per measurement;
printed, and written to --out (default profiles/planner_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch.profiler import ProfilerActivity, profile  # noqa: E402

from drone_rl_amd import DroneBatch, MPPIPlanner  # noqa: E402


def timed(call, reps, rounds=5):
    """Median over `rounds` of the device-event time per call, in us."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    spans = []
    for _ in range(rounds):
        e0.record()
        for i in range(reps):
            call(i)
        e1.record()
        torch.cuda.synchronize()
        spans.append(e0.elapsed_time(e1) * 1e3 / reps)
    return statistics.median(spans)


def kernel_us(call, reps, name):
    """Mean device time of the dispatches whose kernel name holds `name`,
    summed per call, in us."""
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for i in range(reps):
            call(i)
        torch.cuda.synchronize()
    kern = [ev.device_time if hasattr(ev, "device_time") else ev.cuda_time
            for ev in prof.events() if name in ev.name]
    if not kern:
        raise SystemExit(f"the profiler returned no record of a {name} kernel")
    return sum(kern) / reps, len(kern) // reps


def graphed(call, per_graph):
    g = torch.cuda.CUDAGraph()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(cs), torch.cuda.graph(g, stream=cs):
        for i in range(per_graph):
            call(i)
    torch.cuda.current_stream().wait_stream(cs)
    g.replay()
    torch.cuda.synchronize()
    return g


def measure_planner(n, S, H, reps):
    dev = torch.device("cuda", 0)
    env = DroneBatch(n, "gym", device=dev, seed=1)
    sets = 4                        # distinct observations cycled over the launches
    obs = torch.stack([env.reset().clone()] + [env.step(torch.full((n, 4), 2.5, device=dev))[0]
                                               .clone() for _ in range(sets - 1)])
    env.close()
    pl = MPPIPlanner(n, dev, samples=S, horizon=H, seed=1)
    act = torch.empty(n, 4, device=dev)
    call = lambda i: pl.plan(obs[i % sets], out=act)
    for i in range(10):
        call(i)
    torch.cuda.synchronize()
    eager = timed(call, reps)
    per = 20
    g = graphed(call, per)
    graph = timed(lambda i: g.replay(), max(reps // per, 1)) / per
    k_us, launches = kernel_us(call, 20, "mppi_step_kernel")
    steps = n * S * H
    return {"what": "mppi_step", "envs": n, "samples": S, "horizon": H,
            "device": torch.cuda.get_device_name(0), "model_env_steps_per_call": steps,
            "kernel_us": round(k_us, 2), "launches_per_call": launches,
            "call_us_eager": round(eager, 2), "call_us_graph": round(graph, 2),
            "env_steps_per_s_kernel": round(steps / (k_us * 1e-6), 1),
            "env_steps_per_s_graph": round(steps / (graph * 1e-6), 1)}


def measure_rollout(n_envs, K, reps):
    dev = torch.device("cuda", 0)
    env = DroneBatch(n_envs, "gym", device=dev, seed=1)
    env.reset()
    obs = torch.empty(K, n_envs, 15, device=dev)
    rew = torch.empty(K, n_envs, device=dev)
    done = torch.empty(K, n_envs, dtype=torch.uint8, device=dev)
    call = lambda i: env.rollout(K, None, seed=3, step0=K * i, obs_out=obs, rew_out=rew,
                                 done_out=done)
    for i in range(5):
        call(i)
    torch.cuda.synchronize()
    eager = timed(call, reps)
    per = 5
    g = graphed(call, per)
    graph = timed(lambda i: g.replay(), max(reps // per, 1)) / per
    k_us, launches = kernel_us(call, 10, "rollout")
    env.close()
    steps = n_envs * K
    return {"what": "rollout_random", "envs": n_envs, "k": K, "env_steps_per_call": steps,
            "written_bytes_per_env_step": 65,
            "kernel_us": round(k_us, 2), "launches_per_call": launches,
            "call_us_eager": round(eager, 2), "call_us_graph": round(graph, 2),
            "env_steps_per_s_kernel": round(steps / (k_us * 1e-6), 1),
            "env_steps_per_s_graph": round(steps / (graph * 1e-6), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,4096")
    ap.add_argument("--samples", type=int, default=256)
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "planner_bench.jsonl"))
    a = ap.parse_args()
    lines = []
    for n in (int(x) for x in a.envs.split(",")):
        reps = 200 if n <= 1024 else 40
        p = measure_planner(n, a.samples, a.horizon, reps)
        r = measure_rollout(n * a.samples, a.horizon, reps)
        ratio = {"what": "planner_over_rollout", "envs": n,
                 "kernel": round(p["env_steps_per_s_kernel"] / r["env_steps_per_s_kernel"], 4),
                 "graph": round(p["env_steps_per_s_graph"] / r["env_steps_per_s_graph"], 4)}
        for obj in (p, r, ratio):
            lines.append(json.dumps(obj))
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
