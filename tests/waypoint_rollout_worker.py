"""dr_rollout on a gym batch flying waypoint courses against K dr_step
launches, bitwise: every output and every state field, `waypoint` included,
with reaches, resets and the curriculum bump inside the launch.  Imported by
tests/test_waypoint_gpu.py; run as a script (argv: dtype n K) it is that
test's subprocess body, because DRONERL_ROLLOUT_WS is read once per process."""
import sys

import torch

from drone_rl_amd import DroneBatch, random_actions

COURSE = dict(reach_radius=1.0, reach_bonus=1.0)
FIELDS = ("pos", "vel", "euler", "omega", "target", "current_step", "ep_num", "eps", "waypoint")


def _pair(n, dtype):
    out = []
    for _ in range(2):
        x = DroneBatch(n, "gym", dtype=dtype, seed=99, env_id_offset=5, max_steps=16, **COURSE)
        x.set("eps", torch.full((n,), 1.0, dtype=torch.float64))
        x.reset()
        ep = x.get("ep_num").cpu()
        ep[::11] = 1999                     # the curriculum bump inside the launch
        x.set("ep_num", ep)
        out.append(x)
    return out


def _same_state(a, b):
    for k in FIELDS:
        assert torch.equal(a.get(k), b.get(k)), k


def check_rollout(n, K, dtype):
    """Supplied actions, over two launches so a course crosses a launch
    boundary.  Returns (reaches, envs that held j >= 3 at some step)."""
    a, b = _pair(n, dtype)
    acts = torch.empty(K, n, 4, device="cuda")
    for t in range(K):
        random_actions(n, seed=3, step=t, env_id_offset=5, out=acts[t])
    k1 = K // 2
    o1, r1, d1 = a.rollout(k1, acts[:k1])
    o2, r2, d2 = a.rollout(K - k1, acts[k1:])
    obs, rew, done = torch.cat([o1, o2]), torch.cat([r1, r2]), torch.cat([d1, d2])
    assert obs.shape == (K, n, 15)
    deep = torch.zeros(n, dtype=torch.bool, device="cuda")
    for t in range(K):
        so, sr, sd = b.step(acts[t])
        assert torch.equal(obs[t], so), (t, "obs")
        assert torch.equal(rew[t], sr), (t, "rew")
        assert torch.equal(done[t], sd), (t, "done")
        deep |= b.get("waypoint")[:, 0] >= 3
    _same_state(a, b)
    assert int(done.sum()) > n        # max_steps 16 < K: every env reset in the launch
    reaches = int(a.get("waypoint")[:, 1].sum())
    a.close()
    b.close()
    return reaches, int(deep.sum())


def check_rollout_random(n, K, dtype):
    """The in-kernel random policy: actions_out holds the commands."""
    a, b = _pair(n, dtype)
    got = torch.empty(K, n, 4, device="cuda")
    obs, rew, done = a.rollout(K, None, seed=77, step0=1000, actions_out=got)
    for t in range(K):
        act = random_actions(n, seed=77, step=1000 + t, env_id_offset=5)
        assert torch.equal(got[t], act), (t, "actions_out")
        so, sr, sd = b.step(act)
        assert torch.equal(obs[t], so) and torch.equal(rew[t], sr) and torch.equal(done[t], sd), t
    _same_state(a, b)
    reaches = int(a.get("waypoint")[:, 1].sum())
    a.close()
    b.close()
    return reaches


if __name__ == "__main__":
    dt = {"f64": torch.float64, "f32": torch.float32}[sys.argv[1]]
    r, deep = check_rollout(int(sys.argv[2]), int(sys.argv[3]), dt)
    r2 = check_rollout_random(int(sys.argv[2]), int(sys.argv[3]), dt)
    print("ok", *sys.argv[1:], "reaches", r, r2, "deep", deep)
