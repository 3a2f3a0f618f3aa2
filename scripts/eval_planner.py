"""Fly the MPPI planner or, with --planner grad, the
gradient planner (section 25) on N fresh gym envs at a fixed curriculum
level: the baseline row that is not learned, with eval_policy.py's
option flags and metrics.  The loop is env step -> optional sensor model ->
plan; the planner sees the 15-float observation a policy would see, and plans
on the nominal airframe in still air whatever the env flies.  Prints one JSON
line: mean return and length of the episodes that ended, the share of them
that ended by crashing (before the 200-step limit), the share of steps inside
the 5 cm bonus radius, and cost_spread_mean: the mean over plan steps and envs
of the standard deviation of the samples' returns (--planner grad:
cost_mean instead, the mean cost of the incoming nominal).

  python scripts/eval_planner.py --eps 1.0 [--envs 4096 --steps 400]
                                 [--planner grad --horizon 16 --iterations 10 --lr 0.05
                                  --w-pos 1 --w-pos-final 10 ...]
                                 [--samples 256 --horizon 16 --sigma 0.3 --temperature 0.05
                                  --gamma 1 --crash-cost 10 --terminal-weight 1]
                                 [--drag 0.5 --wind-speed 2 --gust-sigma 0.5 --gust-rate 0.1]
                                 [--reach-radius 0.25 --reach-bonus 1]
                                 [--mass-spread 0.3 --inertia-spread 0.3 --motor-spread 0.1]
                                 [--fixed-airframe 1.3,1,0.9,1,1,1]
                                 [--obs-noise 0.02,0.05,0.02,0.1 --obs-bias 0.02,0,0.01,0
                                  --obs-delay 0,2]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

import torch  # noqa: E402

from drone_rl_amd import DroneBatch, GradPlanner, MPPIPlanner  # noqa: E402
from eval_policy import (AIRFRAME, COURSE, HELP, NO_SENSOR, WIND, course_of,  # noqa: E402
                         sensor_front, sensor_of, values_of)

PLANNER_FLAGS = (("samples", int, 256), ("horizon", int, 16), ("sigma", float, 0.3),
                 ("temperature", float, 0.05), ("gamma", float, 1.0), ("crash_cost", float, 10.0),
                 ("terminal_weight", float, 1.0))
# --planner grad: its own flags (horizon is shared)
GRAD_FLAGS = (("horizon", int, 16), ("iterations", int, 10), ("lr", float, 0.05),
              ("beta1", float, 0.9), ("beta2", float, 0.999), ("adam_eps", float, 1e-8),
              ("w_pos", float, 1.0), ("w_vel", float, 0.05), ("w_att", float, 0.05),
              ("w_rate", float, 0.005), ("w_effort", float, 0.0), ("w_pos_final", float, 10.0),
              ("w_vel_final", float, 1.0))


@torch.no_grad()
def evaluate(planner_kw, eps, envs, steps, seed, wind=(0.0,) * 4, course=(None, None),
             airframe=(0.0,) * 3, fixed_airframe=None, sensor=NO_SENSOR, planner="mppi"):
    dev = torch.device("cuda", 0)
    env = DroneBatch(envs, "gym", device=dev, seed=seed, env_id_offset=1 << 40, monitor=True,
                     **dict(zip(WIND.keys, wind)), **dict(zip(COURSE.keys, course)),
                     **dict(zip(AIRFRAME.keys, airframe)))
    fixed = None
    if fixed_airframe is not None:
        # one airframe for every env and episode (eval_policy.evaluate)
        env.set_airframe(0.5, 0.5, 0.5)
        env.set_airframe(0.0, 0.0, 0.0)
        fixed = torch.tensor(fixed_airframe, dtype=torch.float32, device=dev).repeat(envs, 1)
    env.set("eps", torch.full((envs,), float(eps), dtype=torch.float64))
    grad = planner == "grad"
    if grad:
        pl = GradPlanner(envs, dev, **planner_kw)
        costs = torch.empty(envs, dtype=torch.float64, device=dev)
        plan = lambda o, d=None: pl.plan(o, dones=d, out=act, cost_out=costs)
    else:
        pl = MPPIPlanner(envs, dev, seed=seed, env_id_offset=1 << 40, **planner_kw)
        costs = torch.empty(envs, pl.samples, dtype=torch.float64, device=dev)
        plan = lambda o, d=None: pl.plan(o, dones=d, out=act, costs_out=costs)
    see_reset, see_step = sensor_front("gym", sensor, envs, 15, dev, seed)
    act = torch.empty(envs, 4, dtype=torch.float32, device=dev)
    plan(see_reset(env.reset()))
    ret_sum = len_sum = n_done = n_crash = in_bonus = spread = 0.0
    ep_ret = torch.empty(envs, device=dev)
    ep_len = torch.empty(envs, dtype=torch.int32, device=dev)
    env.ep_ret, env.ep_len = ep_ret, ep_len
    for _ in range(steps):
        spread += float(costs.nan_to_num(0.0).mean() if grad
                        else costs.std(1).nan_to_num(0.0).mean())
        if fixed is not None:
            env.set("airframe", fixed)
        o, r, d = env.step(act)
        plan(see_step(o, d), d)
        db = d.bool()
        in_bonus += float((r > 0).float().mean())      # +1 - 0.01 d > 0 only within 5 cm
        n_done += float(db.sum())
        ret_sum += float(ep_ret[db].sum())
        len_sum += float(ep_len[db].float().sum())
        n_crash += float((db & (ep_len < 200)).sum())
    reaches = float(env.get("waypoint")[:, 1].sum()) if env.waypoints_enabled else None
    env.close()
    n = max(n_done, 1.0)
    out = {"episodes": int(n_done), "ep_rew_mean": ret_sum / n, "ep_len_mean": len_sum / n,
           "crash_frac": n_crash / n, "bonus_step_frac": in_bonus / steps,
           ("cost_mean" if grad else "cost_spread_mean"): spread / steps}
    if reaches is not None:
        out["waypoints_per_episode"] = reaches / n
    return out


def build_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=123)
    ap.add_argument("--planner", choices=("mppi", "grad"), default="mppi",
                    help="MPPIPlanner (DESIGN.md section 24) or GradPlanner (section 25)")
    for name, kind, default in PLANNER_FLAGS:
        ap.add_argument("--" + name.replace("_", "-"), type=kind, default=default,
                        help="the planner's %s (DESIGN.md section 24)" % name)
    for name, kind, default in GRAD_FLAGS[1:]:
        ap.add_argument("--" + name.replace("_", "-"), type=kind, default=default,
                        help="--planner grad: its %s (DESIGN.md section 25)" % name)
    for option, texts in HELP.items():
        for k, text in zip(option.keys, texts):
            ap.add_argument("--" + k.replace("_", "-"), type=float, default=None,
                            help=text.replace("gym checkpoints: ", "").replace(
                                "the checkpoint's", "off"))
    ap.add_argument("--fixed-airframe", default=None,
                    help="m,s,g0,g1,g2,g3 -- fly every episode on this one airframe (not "
                         "together with the spreads)")
    ap.add_argument("--obs-noise", default=None, metavar="P,V,A,R",
                    help="sensor model: noise std of the position, velocity, attitude and "
                         "body-rate observations")
    ap.add_argument("--obs-bias", default=None, metavar="P,V,A,R",
                    help="sensor model: half-width of the per-episode bias of the same four")
    ap.add_argument("--obs-delay", default=None, metavar="LO,HI",
                    help="sensor model: per-episode observation latency drawn from LO..HI steps")
    return ap


def settings_from_args(ap, a):
    """The JSON line's header and evaluate()'s keyword arguments, every value
    checked on the host by the rules eval_policy.py applies."""
    from drone_rl_amd.grad_planner import check_gplan
    from drone_rl_amd.planner import check_mppi
    flags, check = (GRAD_FLAGS, check_gplan) if a.planner == "grad" else (PLANNER_FLAGS, check_mppi)
    planner_kw = {name: getattr(a, name) for name, _, _ in flags}
    check(**planner_kw)
    out = {"planner": a.planner, "eps": a.eps, "envs": a.envs, "steps": a.steps, **planner_kw}
    cfg = {}                                    # no checkpoint: every option defaults to off
    sensor = sensor_of(cfg, a)
    if sensor != NO_SENSOR:
        out.update(zip(("obs_noise", "obs_bias", "obs_delay"), sensor))
    wind = values_of(WIND, cfg, a)
    out.update(zip(WIND.keys, WIND.check("gym", *wind)))
    course = course_of(cfg, a)
    rb = COURSE.check("gym", *course, wind=wind)
    if rb is not None:
        out.update(zip(COURSE.keys, rb))
    fixed = None
    if a.fixed_airframe is not None:
        fixed = [float(x) for x in a.fixed_airframe.split(",")]
        if len(fixed) != 6 or not (0 < fixed[0] < float("inf") and 0 < fixed[1] < float("inf")):
            ap.error("--fixed-airframe takes m,s,g0,g1,g2,g3 with m, s positive and finite")
        if any(getattr(a, k) for k in AIRFRAME.keys):
            ap.error("--fixed-airframe and the spreads exclude each other")
    airframe = AIRFRAME.defaults if fixed is not None else values_of(AIRFRAME, cfg, a)
    out.update(zip(AIRFRAME.keys,
                   AIRFRAME.check("gym", *(airframe if fixed is None else (0.5,) * 3),
                                  wind=wind, waypoints=rb)))
    if fixed is not None:
        out.update(zip(AIRFRAME.keys, AIRFRAME.defaults))
        out["fixed_airframe"] = fixed
    return out, dict(planner_kw=planner_kw, eps=a.eps, envs=a.envs, steps=a.steps, seed=a.seed,
                     wind=wind, course=course, airframe=airframe, fixed_airframe=fixed,
                     sensor=sensor, planner=a.planner)


def main():
    ap = build_parser()
    out, kw = settings_from_args(ap, ap.parse_args())
    out["result"] = evaluate(**kw)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
