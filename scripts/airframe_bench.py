"""The gym env with airframe randomisation enabled beside the plain gym env on
one GPU: dr_rollout (K steps per launch, actions read from HBM,
both in the one-role kernel form: run with DRONERL_ROLLOUT_WS=0) and dr_step,
f64 state, the two alternating within each round so both see the same box and
clocks.  The plain gym env's kernels are the parent's, instruction for
instruction.

  DRONERL_ROLLOUT_WS=0 python scripts/airframe_bench.py [--envs 65536 4194304]
                                                        [--k 32] [--rounds 3]
One JSON line per (size, round), then one summary line with the medians, the
algorithmic bytes per env-step and the fraction of the HBM peak they reach;
printed, and written to --out (default profiles/airframe_bench.jsonl)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_rl_amd import DroneBatch, random_actions  # noqa: E402

HBM_PEAK = 8.0e12           # B/s, MI355X
AIRFRAME = dict(mass_spread=0.3, inertia_spread=0.3, motor_spread=0.1)
OD = 15

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[65536, 1 << 22])
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dtype", default="f64")
ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(
    os.path.abspath(__file__))), "profiles", "airframe_bench.jsonl"))
a = ap.parse_args()
dev = torch.device("cuda", 0)
dt = torch.float64 if a.dtype == "f64" else torch.float32
sb = 8 if a.dtype == "f64" else 4


def bytes_per_env_step(airframe, k):
    """Algorithmic traffic: what the law has to move, not what was measured.
    The gym's (scripts/rk4_bench.py): a step reads the 15 state words, the
    episode counter, the action and the step counter and writes the 12 dynamic
    words, the obs row, reward, done and the step counter; a K-step launch
    moves the state once and per step the obs row, reward, done and the
    action.  The airframe adds six f32 words read and none written outside a
    reset: 24 B per dr_step, 24 / K per rollout step."""
    step = (15 * sb + 4 + 16 + 4) + (12 * sb + 4 * OD + 4 + 1 + 4)
    roll = 4 * OD + 4 + 1 + 16 + (15 * sb + 4 + 12 * sb + 4) / k
    if airframe:
        step += 24
        roll += 24 / k
    return step, roll


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


lines = []


def emit(obj):
    lines.append(json.dumps(obj))
    print(lines[-1], flush=True)


summary = {"ws": os.environ.get("DRONERL_ROLLOUT_WS", "auto"), "dtype": a.dtype, "k": a.k,
           "airframe": AIRFRAME, "device": torch.cuda.get_device_name(0)}
for n in a.envs:
    k = a.k
    big = n > 1 << 20
    sets_n = 1 if big else 4            # distinct action buffers cycled over the launches
    reps_roll, reps_step = (10, 50) if big else (40, 400)
    obs = torch.empty(k, n, OD, device=dev)
    rew = torch.empty(k, n, device=dev)
    done = torch.empty(k, n, dtype=torch.uint8, device=dev)
    sets = torch.empty(sets_n, k, n, 4, device=dev)
    for r in range(sets_n):
        for t in range(k):
            random_actions(n, seed=7, step=r * k + t, out=sets[r, t])
    rows = {v: {"rollout_us": [], "step_us": []} for v in ("gym", "airframe")}
    for rnd in range(a.rounds):
        line = {"envs": n, "round": rnd}
        for name in ("gym", "airframe"):
            b = DroneBatch(n, "gym", dtype=dt, device=dev, seed=1,
                           **(AIRFRAME if name == "airframe" else {}))
            assert b.airframe_enabled == (name == "airframe")
            b.reset()
            cyc = [0]

            def nxt():
                cyc[0] = (cyc[0] + 1) % sets_n
                return sets[cyc[0]]
            us_roll = timed(lambda: b.rollout(k, nxt(), obs_out=obs, rew_out=rew, done_out=done),
                            reps_roll)
            acts = sets[0]
            tt = [0]

            def one_step():
                tt[0] = (tt[0] + 1) % k
                b.step(acts[tt[0]])
            us_step = timed(one_step, reps_step)
            rows[name]["rollout_us"].append(us_roll)
            rows[name]["step_us"].append(us_step)
            line[name] = {"rollout_us": round(us_roll, 2), "step_us": round(us_step, 2),
                          "done_per_step": round(done.float().mean().item(), 4)}
            b.close()
        emit(line)
    out = {}
    for name in ("gym", "airframe"):
        b_step, b_roll = bytes_per_env_step(name == "airframe", k)
        ur = statistics.median(rows[name]["rollout_us"])
        us = statistics.median(rows[name]["step_us"])
        out[name] = {
            "rollout_us_median": round(ur, 2), "step_us_median": round(us, 2),
            "rollout_env_steps_per_s": round(n * k / ur * 1e6, 1),
            "step_env_steps_per_s": round(n / us * 1e6, 1),
            "rollout_bytes_per_env_step": round(b_roll, 1), "step_bytes_per_env_step": b_step,
            "rollout_hbm_fraction": round(n * k * b_roll / (ur * 1e-6) / HBM_PEAK, 4),
            "step_hbm_fraction": round(n * b_step / (us * 1e-6) / HBM_PEAK, 4)}
    out["airframe_over_gym"] = {
        "rollout": round(out["airframe"]["rollout_us_median"] /
                         out["gym"]["rollout_us_median"], 3),
        "step": round(out["airframe"]["step_us_median"] / out["gym"]["step_us_median"], 3),
        "rollout_bytes": round(out["airframe"]["rollout_bytes_per_env_step"] /
                               out["gym"]["rollout_bytes_per_env_step"], 3),
        "step_bytes": round(out["airframe"]["step_bytes_per_env_step"] /
                            out["gym"]["step_bytes_per_env_step"], 3)}
    summary[f"n{n}"] = out
    del obs, rew, done, sets
    torch.cuda.empty_cache()
emit(summary)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
