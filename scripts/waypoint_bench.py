"""The gym env on waypoint courses beside the plain gym env on one GPU
(DESIGN.md section 18): dr_rollout (K steps per launch, actions read from HBM,
both in the one-role kernel form: run with DRONERL_ROLLOUT_WS=0) and dr_step,
f64 state, every env at curriculum eps 1, the two alternating within each
round so both see the same box and clocks.  The plain gym env's kernels are
the parent's.

  DRONERL_ROLLOUT_WS=0 python scripts/waypoint_bench.py [--envs 65536 4194304]
                                                        [--k 32] [--rounds 3]
                                                        [--reach-radius 0.25]
One JSON line per (size, round), then one summary line with the medians, the
algorithmic bytes per env-step and the fraction of the HBM peak they reach."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from drone_rl_amd import DroneBatch, random_actions  # noqa: E402

HBM_PEAK = 8.0e12           # B/s, MI355X
OD = 15

ap = argparse.ArgumentParser()
ap.add_argument("--envs", type=int, nargs="+", default=[65536, 1 << 22])
ap.add_argument("--k", type=int, default=32)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--dtype", default="f64")
ap.add_argument("--reach-radius", type=float, default=0.25)
ap.add_argument("--reach-bonus", type=float, default=1.0)
ap.add_argument("--eps", type=float, default=1.0)
a = ap.parse_args()
COURSE = dict(reach_radius=a.reach_radius, reach_bonus=a.reach_bonus)
dev = torch.device("cuda", 0)
dt = torch.float64 if a.dtype == "f64" else torch.float32
sb = 8 if a.dtype == "f64" else 4


def bytes_per_env_step(course, k):
    """Algorithmic traffic: what the law has to move, not what was measured.
    The gym's (scripts/rk4_bench.py): a step reads the 15 state words, the
    episode counter, the action and the step counter and writes the 12 dynamic
    words, the obs row, reward, done and the step counter; a K-step launch
    moves the state once and per step the obs row, reward, done and the
    action.  A course adds two i32 words read and two written: 16 B per
    dr_step, 16 / K per rollout step (the target a reach rewrites is not
    counted: it is an event, not a per-step cost)."""
    step = (15 * sb + 4 + 16 + 4) + (12 * sb + 4 * OD + 4 + 1 + 4)
    roll = 4 * OD + 4 + 1 + 16 + (15 * sb + 4 + 12 * sb + 4) / k
    if course:
        step += 16
        roll += 16 / k
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


summary = {"ws": os.environ.get("DRONERL_ROLLOUT_WS", "auto"), "dtype": a.dtype, "k": a.k,
           "course": COURSE, "eps": a.eps, "device": torch.cuda.get_device_name(0)}
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
    rows = {v: {"rollout_us": [], "step_us": []} for v in ("gym", "waypoint")}
    for rnd in range(a.rounds):
        line = {"envs": n, "round": rnd}
        for name in ("gym", "waypoint"):
            b = DroneBatch(n, "gym", dtype=dt, device=dev, seed=1,
                           **(COURSE if name == "waypoint" else {}))
            assert b.waypoints_enabled == (name == "waypoint")
            b.set("eps", torch.full((n,), a.eps, dtype=torch.float64))
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
            if name == "waypoint":
                steps = (reps_roll + 1) * k + reps_step + 1
                line[name]["reaches_per_env_step"] = round(
                    b.get("waypoint")[:, 1].double().mean().item() / steps, 5)
            b.close()
        print(json.dumps(line), flush=True)
    out = {}
    for name in ("gym", "waypoint"):
        b_step, b_roll = bytes_per_env_step(name == "waypoint", k)
        ur = statistics.median(rows[name]["rollout_us"])
        us = statistics.median(rows[name]["step_us"])
        out[name] = {
            "rollout_us_median": round(ur, 2), "step_us_median": round(us, 2),
            "rollout_env_steps_per_s": round(n * k / ur * 1e6, 1),
            "step_env_steps_per_s": round(n / us * 1e6, 1),
            "rollout_bytes_per_env_step": round(b_roll, 1), "step_bytes_per_env_step": b_step,
            "rollout_hbm_fraction": round(n * k * b_roll / (ur * 1e-6) / HBM_PEAK, 4),
            "step_hbm_fraction": round(n * b_step / (us * 1e-6) / HBM_PEAK, 4)}
    out["waypoint_over_gym"] = {
        "rollout": round(out["waypoint"]["rollout_us_median"] / out["gym"]["rollout_us_median"], 3),
        "step": round(out["waypoint"]["step_us_median"] / out["gym"]["step_us_median"], 3),
        "rollout_bytes": round(out["waypoint"]["rollout_bytes_per_env_step"] /
                               out["gym"]["rollout_bytes_per_env_step"], 3),
        "step_bytes": round(out["waypoint"]["step_bytes_per_env_step"] /
                            out["gym"]["step_bytes_per_env_step"], 3)}
    summary[f"n{n}"] = out
    del obs, rew, done, sets
    torch.cuda.empty_cache()
print(json.dumps(summary))
