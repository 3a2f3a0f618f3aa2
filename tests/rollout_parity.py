"""The rollout contract, spelled once: dr_rollout / dr_rollout_random over one
or more launches equals K dr_step launches on the same actions bit for bit,
every output at every step and every state field at the end.

`compare` is the loop; CASES holds what differs between the env variants and
options that have only the one-role rollout kernel; check_rollout and
check_rollout_random run one case.  Imported by the tests/test_*_gpu.py files;
run as a script (argv: CASE DTYPE N[,N...] K) it is the body of their
subprocess tests, because the launch-form overrides are read once per process.
tests/test_rollout_parity_gpu.py shows that `compare` can fail."""
import sys
from dataclasses import dataclass
from types import SimpleNamespace
from typing import Callable

import torch

BASE = ("pos", "vel", "euler", "omega", "target", "current_step", "ep_num", "eps")


def compare(a, b, K, *, actions=None, random=None, split=None, fields, per_step=None):
    """K rollout steps on `a`, in launches of the lengths `split` (default
    K // 2 and the rest, so the state crosses a launch boundary), against K
    dr_step launches on `b`.  `actions` (K,n,4) are supplied, or `random` =
    (seed, step0) selects the in-kernel policy, whose actions_out rows must be
    random_actions'.  per_step(b, t) runs after each reference step.  Returns
    the rollout's (obs, rew, done); the handles stay open."""
    from drone_rl_amd import random_actions
    n = a.num_envs
    split = (K // 2, K - K // 2) if split is None else split
    assert sum(split) == K
    if random is not None:
        seed, step0 = random
        got = torch.empty(K, n, 4, device="cuda")
    outs, t0 = [], 0
    for k in split:
        if random is None:
            outs.append(a.rollout(k, actions[t0:t0 + k]))
        else:
            outs.append(a.rollout(k, None, seed=seed, step0=step0 + t0,
                                  actions_out=got[t0:t0 + k]))
        t0 += k
    obs, rew, done = outs[0] if len(outs) == 1 else (torch.cat(x) for x in zip(*outs))
    for t in range(K):
        if random is None:
            act = actions[t]
        else:
            act = random_actions(n, seed=seed, step=step0 + t, env_id_offset=a.env_id_offset)
            assert torch.equal(got[t], act), (t, "actions_out")
        so, sr, sd = b.step(act)
        assert torch.equal(obs[t], so), (t, "obs")
        assert torch.equal(rew[t], sr), (t, "rew")
        assert torch.equal(done[t], sd), (t, "done")
        if per_step is not None:
            per_step(b, t)
    for k in fields:
        assert torch.equal(a.get(k), b.get(k)), k
    return obs, rew, done


# ---- the cases --------------------------------------------------------------
# Each *_live(r) asserts that the case's feature did something in the run r:
# the pair r.a / r.b, r.n, r.acts, the outputs r.obs / r.rew / r.done, r.start
# (a's fields before the run) and r.seen (the case's `watch`, OR-ed over the
# reference steps).
def _smooth_live(r):
    # the lag and the penalty are live: the forces differ from the commands
    assert not torch.equal(r.obs[-1][:, 15:], r.acts[-1])


def _tag_live(r):
    # the pair coupling is live: the ends come in pairs, the rewards are not the gym's
    assert torch.equal(r.done[:, 0::2], r.done[:, 1::2])
    assert bool((r.rew[:, 1::2] > 0).any())


def _rk4_live(r):
    # the attitude moved off the identity
    assert not torch.equal(r.obs[-1][:, 6], torch.ones(r.n, device="cuda"))


def _wind_live(r):
    w = r.a.get("wind")
    assert bool((w[:, :3] != 0).all()) and bool((w[:, 3:] != 0).any())   # the wind is live


def _airframe_live(r):
    af, af0 = r.a.get("airframe"), r.start["airframe"]
    assert bool((af != 1).all(dim=1).any()) and bool((af != af0).any(dim=1).all())   # redrawn


def _waypoint_counts(r):
    """(reaches, envs that held j >= 3 at some step)."""
    return int(r.a.get("waypoint")[:, 1].sum()), int(r.seen.sum())


@dataclass(frozen=True)
class Case:
    variant: str
    kw: dict                                # the constructor's option keywords
    obs_dim: int
    fields: tuple
    env_id_offset: int = 5
    max_steps: int = 16                     # < K: every env resets in the launch
    min_done: Callable = lambda n: n + 1    # least int(done.sum()): more than n
    prepare: Callable = None                # prepare(x) before x.reset()
    split_random: bool = False              # the random form over two launches too
    watch: Callable = None                  # watch(b) -> (n,) bool after each step
    live: Callable = None                   # asserts on the supplied-actions run
    result: Callable = None                 # what both checks return


CASES = {
    "smooth": Case("smooth", dict(motor_alpha=0.25, rate_penalty=0.02), 19, BASE + ("motor",),
                   live=_smooth_live),
    # an even offset: env ids 2j pursue; every pair resets three times
    "tag": Case("tag", dict(tag_radius=0.3, crash_penalty=0.5), 19, BASE, env_id_offset=6,
                max_steps=7, min_done=lambda n: 3 * n, live=_tag_live),
    "rk4": Case("rk4", {}, 16, tuple("quat" if k == "euler" else k for k in BASE), max_steps=7,
                split_random=True, live=_rk4_live),
    "wind": Case("gym", dict(drag=0.5, wind_speed=2.0, gust_sigma=0.5, gust_rate=0.1), 15,
                 BASE + ("wind",), live=_wind_live),
    "waypoint": Case("gym", dict(reach_radius=1.0, reach_bonus=1.0), 15, BASE + ("waypoint",),
                     prepare=lambda x: x.set("eps", torch.full((x.num_envs,), 1.0,
                                                               dtype=torch.float64)),
                     watch=lambda b: b.get("waypoint")[:, 0] >= 3, result=_waypoint_counts),
    "airframe": Case("gym", dict(mass_spread=0.3, inertia_spread=0.3, motor_spread=0.1), 15,
                     BASE + ("airframe",), live=_airframe_live),
}


def pair(case, n, dtype):
    """Two identical batches of the case after reset."""
    from drone_rl_amd import DroneBatch
    out = []
    for _ in range(2):
        x = DroneBatch(n, case.variant, dtype=dtype, seed=99, env_id_offset=case.env_id_offset,
                       max_steps=case.max_steps, **case.kw)
        if case.prepare is not None:
            case.prepare(x)
        x.reset()
        ep = x.get("ep_num").cpu()
        ep[::11] = 1999                     # the curriculum bump inside the launch
        x.set("ep_num", ep)
        out.append(x)
    return out


def _check(case, n, K, dtype, *, random):
    from drone_rl_amd import random_actions
    case = CASES[case] if isinstance(case, str) else case
    a, b = pair(case, n, dtype)
    r = SimpleNamespace(a=a, b=b, n=n, acts=None,
                        start={k: a.get(k).clone() for k in case.fields},
                        seen=torch.zeros(n, dtype=torch.bool, device="cuda"))
    per_step = None
    if case.watch is not None:
        def per_step(b, t):
            r.seen |= case.watch(b)
    if random is None:
        r.acts = torch.empty(K, n, 4, device="cuda")
        for t in range(K):
            random_actions(n, seed=3, step=t, env_id_offset=case.env_id_offset, out=r.acts[t])
    r.obs, r.rew, r.done = compare(
        a, b, K, actions=r.acts, random=random, fields=case.fields, per_step=per_step,
        split=None if random is None or case.split_random else (K,))
    if random is None:
        assert r.obs.shape == (K, n, case.obs_dim)
        assert int(r.done.sum()) >= case.min_done(n)
        if case.live is not None:
            case.live(r)
    out = case.result(r) if case.result is not None else None
    a.close()
    b.close()
    return out


def check_rollout(case, n, K, dtype):
    """Supplied actions, over two launches so the case's state crosses a
    launch boundary; then the reset count and the case's liveness asserts."""
    return _check(case, n, K, dtype, random=None)


def check_rollout_random(case, n, K, dtype):
    """The in-kernel random policy: actions_out holds the commands."""
    return _check(case, n, K, dtype, random=(77, 1000))


if __name__ == "__main__":
    if len(sys.argv) != 5 or sys.argv[1] not in CASES or sys.argv[2] not in ("f64", "f32"):
        sys.exit(f"usage: rollout_parity.py {{{','.join(CASES)}}} {{f64,f32}} N[,N...] K")
    dt = {"f64": torch.float64, "f32": torch.float32}[sys.argv[2]]
    for n in sys.argv[3].split(","):
        res = [f(sys.argv[1], int(n), int(sys.argv[4]), dt)
               for f in (check_rollout, check_rollout_random)]
        print("ok", sys.argv[1], sys.argv[2], n, sys.argv[4],
              *(("(reaches, deep):", *res) if res[0] is not None else ()))
