"""Subprocess body of tests/test_rollout_gpu.py's forced-form tests:
dr_rollout's kernel form is chosen once per process (DRONERL_ROLLOUT_WS, read
at the first launch), so each forced form runs in its own process.  K steps
of dr_rollout against K dr_step launches, bitwise, every output and the final
state.  argv: variant n K [max_steps], the actions read from HBM; with
max_steps given, the in-kernel random policy instead, its actions checked
against random_actions and at least 3 n resets required."""
import sys

import torch

from drone_rl_amd import DroneBatch, random_actions
from rollout_parity import BASE, compare


def main():
    variant, n, K = sys.argv[1], int(sys.argv[2]), int(sys.argv[3])
    max_steps = int(sys.argv[4]) if len(sys.argv) > 4 else None
    kw = dict(dtype=torch.float64, seed=99, env_id_offset=5, max_steps=max_steps)
    a = DroneBatch(n, variant, **kw)
    b = DroneBatch(n, variant, **kw)
    for x in (a, b):
        x.reset()
        ep = x.get("ep_num").cpu()
        ep[::11] = 1999                     # the curriculum bump inside the launch
        x.set("ep_num", ep)
        if max_steps:
            # a third of the envs reset twice within one draw-ahead group
            s = x.get("current_step").cpu()
            s[::3] = max_steps - 2
            x.set("current_step", s)
    fields = BASE + (("motion",) if variant == "moving" else ())
    if max_steps:
        obs, rew, done = compare(a, b, K, random=(3, 500), split=(K,), fields=fields)
    else:
        acts = torch.empty(K, n, 4, device="cuda")
        for t in range(K):
            random_actions(n, seed=3, step=t, env_id_offset=5, out=acts[t])
        obs, rew, done = compare(a, b, K, actions=acts, split=(K,), fields=fields)
    assert int(done.sum()) >= (3 * n if max_steps else n // 8 + 1)
    print("ok", variant, n, K)


if __name__ == "__main__":
    main()
