"""Evaluate a trained policy (a PPOTrainer checkpoint) on N fresh gym envs at
a fixed curriculum level, the way the reference's test.py does
(model.predict(obs, deterministic=True): the Gaussian's mean clipped to the
action space) and with sampled actions (the training-time policy), for S
steps with DummyVecEnv auto-reset.  Prints one JSON line: mean return and
length of the episodes that ended, the fraction of steps inside the 5 cm
bonus radius, the fraction of episodes that ended by crashing (before
the 200-step limit), and cmd_dev_sq_mean: the mean over env-steps of
|command - motor force|^2 (N^2), how abruptly the policy drives the motors.

A checkpoint trained on variant "smooth" is evaluated on that variant with
the motor_alpha / rate_penalty of its config (the motor force is the env's
lagged one, obs[:, 15:19]).  For a gym checkpoint the motors follow the
command at once, so the force before a step is the previous clipped command,
or HOVER on the first step of an episode -- what the smooth variant holds at
its neutral parameters.

A checkpoint trained on variant "tag"  is evaluated
in self-play on that variant with the tag_radius / crash_penalty of its
config: per role the mean return of the episodes that ended and the share of
them in which that drone crashed, and per pair tag_fraction (the share of
steps with the two closer than tag_radius) and the mean distance.

A gym checkpoint is evaluated under wind, gusts and linear drag (DESIGN.md
section 17) with --drag / --wind-speed / --gust-sigma / --gust-rate; a flag
not given takes the value of the checkpoint's config (0 for checkpoints from
before the option), so a wind-trained policy is by default evaluated under
its training conditions and any gym policy can be put under any wind (the
wind is not observed: the two kinds of policy are interchangeable).

A gym checkpoint is flown on waypoint courses with
--reach-radius / --reach-bonus; a flag not given takes the checkpoint's value
(off for checkpoints trained without the option; giving one enables it with
the other at its default).  The obs is the gym's 15 floats, so any gym policy
flies a course and a course policy flies the plain gym env
(--reach-radius 0 switches a course checkpoint's option off).  On a course the
result adds waypoints_per_episode, the reach counters' sum over the episodes
that ended.

A gym checkpoint is flown on randomised airframes
with --mass-spread / --inertia-spread / --motor-spread; a flag not given takes
the checkpoint's value (0 for checkpoints from before the option).  The
airframe is not observed, so any gym policy can be put on any airframe.
--fixed-airframe m,s,g0,g1,g2,g3 flies every env and every episode on that one
airframe instead (written through set("airframe") ahead of each step).

A checkpoint with VecNormalize statistics ("vecnorm")
is evaluated through them, frozen: the policy sees normalize_obs(obs) of the
raw env's observations, and every reported reward is the env's raw one.
--no-normalize feeds the raw observations instead.

Any checkpoint is put behind a sensor model with
--obs-noise P,V,A,R / --obs-bias P,V,A,R / --obs-delay LO,HI: the policy sees
the env's observation with that noise, per-episode bias and latency (ahead of
the frozen VecNormalize statistics, if any); every reported figure is of the
true state.  A flag not given takes the checkpoint's value (neutral for
checkpoints from before the option), so `--obs-noise 0,0,0,0 --obs-bias
0,0,0,0 --obs-delay 0,0` flies a sensor-trained policy on exact state.

  python scripts/eval_policy.py CKPT --eps 1.0 [--envs 65536 --steps 400]
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

import torch  # noqa: E402

from drone_rl_amd import DroneBatch  # noqa: E402
from drone_rl_amd.env import ENV_OPTION, HOVER, MOTOR_MAX, OBS_DIM, check_tag  # noqa: E402
from drone_rl_amd.policy import ActorCritic, PolicyInference  # noqa: E402


WIND, COURSE, AIRFRAME = ENV_OPTION["wind"], ENV_OPTION["waypoints"], ENV_OPTION["airframe"]
# the help of each gym option's flags here (one text for all of an option's
# flags, or one per flag)
HELP = {
    WIND: ("gym checkpoints: evaluate under this wind parameter (default: the checkpoint's)",) * 4,
    COURSE: ("gym checkpoints: fly waypoint courses with this reach radius "
             "(default: the checkpoint's; 0 = the plain gym env)",
             "gym checkpoints: the reward added in the step of a reach"),
    AIRFRAME: ("gym checkpoints: fly on airframes drawn with this spread "
               "(default: the checkpoint's)",) * 3,
}


def values_of(option, cfg, args):
    """An option's values, per keyword the command line's, else the
    checkpoint's (its off value for checkpoints from before the option)."""
    return tuple(cfg.get(k, d) if getattr(args, k) is None else getattr(args, k)
                 for k, d in zip(option.keys, option.defaults))


def course_of(cfg, args):
    """(reach_radius, reach_bonus) or (None, None): values_of the course, but
    --reach-radius 0 switches the option off."""
    if args.reach_radius is not None and args.reach_radius == 0:
        return None, None
    return values_of(COURSE, cfg, args)


def frozen_normaliser(sd, envs, obs_dim, dev, normalize=True):
    """obs -> what the policy was trained on: the checkpoint's VecNormalize
    statistics, frozen (the identity for a checkpoint without them)."""
    if not normalize or "vecnorm" not in sd:
        return lambda obs: obs
    from drone_rl_amd import ppo_kernels as K
    vs = sd["vecnorm"]
    vn = K.VecNormalize(envs, obs_dim, dev, gamma=vs["gamma"], clip_obs=vs["clip_obs"],
                        clip_reward=vs["clip_reward"], epsilon=vs["epsilon"])
    vn.load_state_dict(vs)      # (returns of another env count are dropped)
    vn.training = False
    buf = torch.empty(envs, obs_dim, dtype=torch.float32, device=dev)
    return lambda obs: vn.normalize_obs(obs, out=buf)


NO_SENSOR = ((0.0,) * 4, (0.0,) * 4, (0, 0))


def sensor_of(cfg, args):
    """(noise4, bias4, (lo, hi)): per setting the command line's, else the
    checkpoint's (neutral for checkpoints from before the option), checked."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.train import _floats4, _ints2
    given = (None if args.obs_noise is None else _floats4(args.obs_noise),
             None if args.obs_bias is None else _floats4(args.obs_bias),
             None if args.obs_delay is None else _ints2(args.obs_delay))
    return K.check_sensor(*(tuple(cfg.get(k, d)) if g is None else g
                            for g, k, d in zip(given, ("obs_noise", "obs_bias", "obs_delay"),
                                               NO_SENSOR)))


def sensor_front(variant, sensor, envs, obs_dim, dev, seed):
    """(reset, step): the env's clean observation -> what the policy sees of
    it (both the identity for neutral settings)."""
    from drone_rl_amd import ppo_kernels as K
    noise, bias, delay = sensor
    if K.sensor_neutral(noise, bias, delay):
        return (lambda obs: obs), (lambda obs, done: obs)
    sm = K.SensorModel(envs, obs_dim, dev, columns=K.sensor_columns(variant, noise, bias),
                       delay=delay, seed=seed, env_id_offset=1 << 40)
    buf = torch.empty(envs, obs_dim, dtype=torch.float32, device=dev)
    return (lambda obs: sm.reset(obs, out=buf)), \
        (lambda obs, done: sm.step(obs, done.contiguous(), obs_out=buf))


@torch.no_grad()
def evaluate(ckpt, eps, envs, steps, seed, deterministic, wind=(0.0, 0.0, 0.0, 0.0),
             course=(None, None), airframe=(0.0, 0.0, 0.0), fixed_airframe=None,
             normalize=True, sensor=NO_SENSOR):
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    cfg = sd["config"]
    dev = torch.device("cuda", 0)
    smooth = cfg.get("variant", "gym") == "smooth"
    # "rk4"  is the gym's task: evaluated like it, on its
    # own variant (16-d obs)
    variant = "smooth" if smooth else ("rk4" if cfg.get("variant") == "rk4" else "gym")
    alpha = float(cfg.get("motor_alpha", 1.0)) if smooth else 1.0
    lam = float(cfg.get("rate_penalty", 0.0)) if smooth else 0.0
    pol = ActorCritic(OBS_DIM[variant], 4, tuple(cfg["net_arch"]), dev, 0.0, 0)
    pol.flat.data.copy_(sd["flat"].to(dev))
    env = DroneBatch(envs, variant, device=dev, seed=seed, env_id_offset=1 << 40, monitor=True,
                     motor_alpha=alpha, rate_penalty=lam, **dict(zip(WIND.keys, wind)),
                     **dict(zip(COURSE.keys, course)), **dict(zip(AIRFRAME.keys, airframe)))
    fixed = None
    if fixed_airframe is not None:
        # one airframe for every env and episode: the option enabled, its
        # resets drawing ones, the field written again ahead of each step
        env.set_airframe(0.5, 0.5, 0.5)
        env.set_airframe(0.0, 0.0, 0.0)
        fixed = torch.tensor(fixed_airframe, dtype=torch.float32, device=dev).repeat(envs, 1)
    env.set("eps", torch.full((envs,), float(eps), dtype=torch.float64))
    obs = env.reset().clone()
    infer = PolicyInference(pol, envs)
    norm = frozen_normaliser(sd, envs, OBS_DIM[variant], dev, normalize)
    see_reset, see_step = sensor_front(variant, sensor, envs, OBS_DIM[variant], dev, seed)
    seen = see_reset(obs)
    g = torch.Generator(device=dev).manual_seed(seed)
    std = pol.log_std.exp()
    ret_sum = len_sum = n_done = n_crash = 0.0
    in_bonus = 0.0
    dev_sq = 0.0
    # the force each motor applies before the step (gym: tracked here)
    force = torch.full((envs, 4), HOVER, device=dev)
    ep_ret = torch.empty(envs, device=dev)
    ep_len = torch.empty(envs, dtype=torch.int32, device=dev)
    for _ in range(steps):
        mean, _ = infer(norm(seen))
        a = mean if deterministic else mean + std * torch.randn(mean.shape, generator=g,
                                                                 device=dev)
        env.ep_ret, env.ep_len = ep_ret, ep_len
        cmd = a.clamp(0.0, MOTOR_MAX).contiguous()
        if smooth:
            force = obs[:, 15:19]
        dev_sq += float(((cmd - force) ** 2).sum(1).mean())
        if fixed is not None:
            env.set("airframe", fixed)
        o, r, d = env.step(cmd)
        obs = o.clone()
        seen = see_step(obs, d)
        db = d.bool()
        if not smooth:
            force = torch.where(db[:, None], torch.full_like(cmd, HOVER), cmd)
        in_bonus += float((r > 0).float().mean())      # +1 - 0.01 d > 0 only within 5 cm
        n_done += float(db.sum())
        ret_sum += float(ep_ret[db].sum())
        len_sum += float(ep_len[db].float().sum())
        n_crash += float((db & (ep_len < 200)).sum())
    reaches = float(env.get("waypoint")[:, 1].sum()) if env.waypoints_enabled else None
    env.close()
    n = max(n_done, 1.0)
    out = {"deterministic": deterministic, "episodes": int(n_done),
           "ep_rew_mean": ret_sum / n, "ep_len_mean": len_sum / n,
           "crash_frac": n_crash / n, "bonus_step_frac": in_bonus / steps,
           "cmd_dev_sq_mean": dev_sq / steps}
    if reaches is not None:
        # on a course bonus_step_frac is the share of steps with a reach
        # (given a bonus above 0.01 R); per episode: all reaches counted since
        # enabling over the episodes that ended
        out["waypoints_per_episode"] = reaches / n
    return out


@torch.no_grad()
def evaluate_tag(ckpt, envs, steps, seed, deterministic, normalize=True, sensor=NO_SENSOR):
    sd = torch.load(ckpt, map_location="cpu", weights_only=True)
    cfg = sd["config"]
    dev = torch.device("cuda", 0)
    pol = ActorCritic(OBS_DIM["tag"], 4, tuple(cfg["net_arch"]), dev, 0.0, 0)
    pol.flat.data.copy_(sd["flat"].to(dev))
    env = DroneBatch(envs, "tag", device=dev, seed=seed, env_id_offset=1 << 40, monitor=True,
                     keep_terminal_obs=True, tag_radius=cfg.get("tag_radius"),
                     crash_penalty=cfg.get("crash_penalty"))
    obs = env.reset().clone()
    infer = PolicyInference(pol, envs)
    norm = frozen_normaliser(sd, envs, OBS_DIM["tag"], dev, normalize)
    see_reset, see_step = sensor_front("tag", sensor, envs, OBS_DIM["tag"], dev, seed)
    seen = see_reset(obs)
    g = torch.Generator(device=dev).manual_seed(seed)
    std = pol.log_std.exp()
    ep_ret = torch.empty(envs, device=dev)
    ep_len = torch.empty(envs, dtype=torch.int32, device=dev)
    # per role (0 pursuer, 1 evader): return sum, episodes, own crashes
    ret = [0.0, 0.0]
    eps_n = [0.0, 0.0]
    crashed = [0.0, 0.0]
    len_sum = tagged = dist = 0.0
    for _ in range(steps):
        mean, _ = infer(norm(seen))
        a = mean if deterministic else mean + std * torch.randn(mean.shape, generator=g,
                                                                 device=dev)
        env.ep_ret, env.ep_len = ep_ret, ep_len
        o, r, d = env.step(a.clamp(0.0, MOTOR_MAX).contiguous())
        obs = o.clone()
        seen = see_step(obs, d)
        db = d.bool()
        # the state the step ended in: the terminal obs where the pair was reset
        end = torch.where(db[:, None], env.term_obs, o)
        own_crash = db & ((end[:, 2] < 0) | (end[:, :3].square().sum(1) > 2500.0))
        dd = end[0::2, 12:15].norm(dim=1)
        tagged += float((dd < env.tag_radius).float().mean())
        dist += float(dd.mean())
        len_sum += float(ep_len[db].float().sum())
        for role in (0, 1):
            m = db[role::2]
            ret[role] += float(ep_ret[role::2][m].sum())
            eps_n[role] += float(m.sum())
            crashed[role] += float(own_crash[role::2].sum())
    env.close()
    n = [max(x, 1.0) for x in eps_n]
    return {"deterministic": deterministic, "episodes": int(eps_n[0]),
            "ep_len_mean": len_sum / max(eps_n[0] + eps_n[1], 1.0),
            "ep_rew_mean_pursuer": ret[0] / n[0], "ep_rew_mean_evader": ret[1] / n[1],
            "crash_frac_pursuer": crashed[0] / n[0], "crash_frac_evader": crashed[1] / n[1],
            "tag_fraction": tagged / steps, "pair_distance_mean": dist / steps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("ckpt")
    ap.add_argument("--eps", type=float, default=1.0)
    ap.add_argument("--envs", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--seed", type=int, default=123)
    for option, texts in HELP.items():
        for k, text in zip(option.keys, texts):
            ap.add_argument("--" + k.replace("_", "-"), type=float, default=None, help=text)
    ap.add_argument("--fixed-airframe", default=None,
                    help="gym checkpoints: m,s,g0,g1,g2,g3 -- fly every episode on this one "
                         "airframe (not together with the spreads)")
    ap.add_argument("--no-normalize", action="store_true",
                    help="checkpoints with VecNormalize statistics: feed the policy the raw "
                         "observations instead of the normalised ones")
    ap.add_argument("--obs-noise", default=None, metavar="P,V,A,R",
                    help="sensor model: noise std of the position, velocity, attitude and "
                         "body-rate observations (default: the checkpoint's)")
    ap.add_argument("--obs-bias", default=None, metavar="P,V,A,R",
                    help="sensor model: half-width of the per-episode bias of the same four")
    ap.add_argument("--obs-delay", default=None, metavar="LO,HI",
                    help="sensor model: per-episode observation latency drawn from LO..HI steps")
    a = ap.parse_args()
    out = {"ckpt": os.path.basename(a.ckpt), "eps": a.eps, "envs": a.envs, "steps": a.steps}
    sd = torch.load(a.ckpt, map_location="cpu", weights_only=True)
    cfg = sd["config"]
    if "vecnorm" in sd:
        out["normalized"] = not a.no_normalize
    out["variant"] = cfg.get("variant", "gym")
    sensor = sensor_of(cfg, a)
    if sensor != NO_SENSOR:
        out.update(zip(("obs_noise", "obs_bias", "obs_delay"), sensor))
    if out["variant"] == "smooth":
        out["motor_alpha"] = cfg.get("motor_alpha", 1.0)
        out["rate_penalty"] = cfg.get("rate_penalty", 0.0)
    if out["variant"] == "tag":
        out["tag_radius"], out["crash_penalty"] = check_tag("tag", cfg.get("tag_radius"),
                                                            cfg.get("crash_penalty"))
    wind = values_of(WIND, cfg, a)
    if any(wind) or out["variant"] == "gym":
        # raises for a non-gym checkpoint with a wind flag
        out.update(zip(WIND.keys, WIND.check(out["variant"], *wind)))
    course = course_of(cfg, a)
    # raises for a non-gym checkpoint with a course flag, or wind and a course
    rb = COURSE.check(out["variant"], *course, wind=wind)
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
    if any(airframe) or fixed is not None or out["variant"] == "gym":
        # raises for a non-gym checkpoint with a spread, or a spread beside
        # wind or a course
        out.update(zip(AIRFRAME.keys,
                       AIRFRAME.check(out["variant"], *(airframe if fixed is None else (0.5,) * 3),
                                      wind=wind, waypoints=rb)))
        if fixed is not None:
            out.update(zip(AIRFRAME.keys, AIRFRAME.defaults))
            out["fixed_airframe"] = fixed
    for det in (True, False):
        out["deterministic" if det else "sampled"] = (
            evaluate_tag(a.ckpt, a.envs, a.steps, a.seed, det, not a.no_normalize, sensor)
            if out["variant"] == "tag"
            else evaluate(a.ckpt, a.eps, a.envs, a.steps, a.seed, det, wind, course, airframe,
                          fixed, not a.no_normalize, sensor))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
