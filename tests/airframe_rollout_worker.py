"""dr_rollout on a gym batch with airframe randomisation enabled against K
dr_step launches, bitwise: every output and every state field, `airframe`
included, with resets (and their airframe draws) inside the launch.  Imported
by tests/test_airframe_gpu.py; run as a script (argv: dtype n K) it is that
test's subprocess body, because DRONERL_ROLLOUT_WS is read once per process."""
import sys

import torch

from drone_rl_amd import DroneBatch, random_actions

AIRFRAME = dict(mass_spread=0.3, inertia_spread=0.3, motor_spread=0.1)
FIELDS = ("pos", "vel", "euler", "omega", "target", "current_step", "ep_num", "eps", "airframe")


def _pair(n, dtype):
    out = []
    for _ in range(2):
        x = DroneBatch(n, "gym", dtype=dtype, seed=99, env_id_offset=5, max_steps=16, **AIRFRAME)
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
    """Supplied actions, over two launches so an episode (and its airframe)
    crosses a launch boundary."""
    a, b = _pair(n, dtype)
    af0 = a.get("airframe").clone()
    acts = torch.empty(K, n, 4, device="cuda")
    for t in range(K):
        random_actions(n, seed=3, step=t, env_id_offset=5, out=acts[t])
    k1 = K // 2
    o1, r1, d1 = a.rollout(k1, acts[:k1])
    o2, r2, d2 = a.rollout(K - k1, acts[k1:])
    obs, rew, done = torch.cat([o1, o2]), torch.cat([r1, r2]), torch.cat([d1, d2])
    assert obs.shape == (K, n, 15)
    for t in range(K):
        so, sr, sd = b.step(acts[t])
        assert torch.equal(obs[t], so), (t, "obs")
        assert torch.equal(rew[t], sr), (t, "rew")
        assert torch.equal(done[t], sd), (t, "done")
    _same_state(a, b)
    assert int(done.sum()) > n        # max_steps 16 < K: every env reset in the launch
    af = a.get("airframe")
    assert bool((af != 1).all(dim=1).any()) and bool((af != af0).any(dim=1).all())   # redrawn
    a.close()
    b.close()


def check_rollout_random(n, K, dtype):
    """The in-kernel random policy: actions_out holds the commands, not the
    gained ones."""
    a, b = _pair(n, dtype)
    got = torch.empty(K, n, 4, device="cuda")
    obs, rew, done = a.rollout(K, None, seed=77, step0=1000, actions_out=got)
    for t in range(K):
        act = random_actions(n, seed=77, step=1000 + t, env_id_offset=5)
        assert torch.equal(got[t], act), (t, "actions_out")
        so, sr, sd = b.step(act)
        assert torch.equal(obs[t], so) and torch.equal(rew[t], sr) and torch.equal(done[t], sd), t
    _same_state(a, b)
    a.close()
    b.close()


if __name__ == "__main__":
    dt = {"f64": torch.float64, "f32": torch.float32}[sys.argv[1]]
    check_rollout(int(sys.argv[2]), int(sys.argv[3]), dt)
    check_rollout_random(int(sys.argv[2]), int(sys.argv[3]), dt)
    print("ok", *sys.argv[1:])
