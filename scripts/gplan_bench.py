"""The gradient planner on one GPU: what one
dr_gplan_step costs, stated as model steps per second (N * H * I forward steps
plus as many adjoint steps per call), beside dr_mppi_step (N * S * H forward
steps) and dr_rollout_random in the same session, and the bytes one call moves
through its workspace against what HBM could carry in the kernel's time.

  python scripts/gplan_bench.py [--envs 256,4096,65536] [--horizon 16] [--iterations 10]

Per N: the kernel's mean time between its dispatch's start and end timestamps
(the profiler's kernel records, taken after the event timings, not during
them), and the time per call between two device events, eager and replayed
from a graph.  One thread plans one env, so below 65,536 envs the grid has
fewer waves than the chip has SIMDs: "simds_used_frac" says how few.  One JSON
line per measurement; printed, and written to --out (default
profiles/gplan_bench.jsonl)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from drone_rl_amd import DroneBatch, GradPlanner  # noqa: E402
from planner_bench import graphed, kernel_us, measure_planner, measure_rollout, timed  # noqa: E402

HBM_PEAK = 8.0e12            # bytes / s, the MI355X's specified HBM3E bandwidth
SIMDS = 256 * 4              # CUs x SIMDs: one wave of 64 envs occupies one


def workspace_traffic(n, H, I):
    """Bytes one call reads and writes in its workspace and nominal, counted
    from the kernel's loops: the nominal in and out (4 H f32 each way, and its
    word-major copy); per sweep the tape out and back (12 (H - 1) f64 each
    way), U read twice and written once (4 H f32), m and s written (4 H f64
    each) and, after the first sweep, read."""
    per_sweep = 2 * 12 * (H - 1) * 8 + 3 * 4 * H * 4 + 2 * 4 * H * 8
    return n * (I * per_sweep + (I - 1) * 2 * 4 * H * 8 + 4 * (4 * H * 4))


def measure_gplan(n, H, I, reps):
    dev = torch.device("cuda", 0)
    env = DroneBatch(n, "gym", device=dev, seed=1)
    sets = 4                        # distinct observations cycled over the launches
    obs = torch.stack([env.reset().clone()] + [env.step(torch.full((n, 4), 2.5, device=dev))[0]
                                               .clone() for _ in range(sets - 1)])
    env.close()
    pl = GradPlanner(n, dev, horizon=H, iterations=I)
    act = torch.empty(n, 4, device=dev)
    call = lambda i: pl.plan(obs[i % sets], out=act)
    for i in range(10):
        call(i)
    torch.cuda.synchronize()
    eager = timed(call, reps)
    per = 20
    g = graphed(call, per)
    graph = timed(lambda i: g.replay(), max(reps // per, 1)) / per
    k_us, launches = kernel_us(call, 20, "gplan_step_kernel")
    steps = 2 * n * H * I
    moved = workspace_traffic(n, H, I)
    return {"what": "gplan_step", "envs": n, "horizon": H, "iterations": I,
            "device": torch.cuda.get_device_name(0), "model_steps_per_call": steps,
            "kernel_us": round(k_us, 2), "launches_per_call": launches,
            "call_us_eager": round(eager, 2), "call_us_graph": round(graph, 2),
            "model_steps_per_s_kernel": round(steps / (k_us * 1e-6), 1),
            "model_steps_per_s_graph": round(steps / (graph * 1e-6), 1),
            "simds_used_frac": round(min(1.0, -(-n // 64) / SIMDS), 4),
            "workspace_bytes": pl.workspace_bytes, "bytes_moved_per_call": moved,
            "bytes_per_s_kernel": round(moved / (k_us * 1e-6), 1),
            "hbm_bound_us": round(moved / HBM_PEAK * 1e6, 2),
            "hbm_bound_over_kernel": round(moved / HBM_PEAK * 1e6 / k_us, 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", default="256,4096,65536")
    ap.add_argument("--horizon", type=int, default=16)
    ap.add_argument("--iterations", type=int, default=10)
    ap.add_argument("--mppi-envs", default="256,4096",
                    help="dr_mppi_step (S = 256) and dr_rollout_random on N * 256 envs at these N")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gplan_bench.jsonl"))
    a = ap.parse_args()
    lines = []

    def emit(obj):
        lines.append(json.dumps(obj))
        print(lines[-1], flush=True)
    for n in (int(x) for x in a.envs.split(",")):
        emit(measure_gplan(n, a.horizon, a.iterations, 200 if n <= 4096 else 40))
    for n in (int(x) for x in a.mppi_envs.split(",") if x):
        reps = 200 if n <= 1024 else 40
        emit(measure_planner(n, 256, a.horizon, reps))
        emit(measure_rollout(n * 256, a.horizon, reps))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
