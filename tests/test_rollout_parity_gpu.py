"""rollout_parity.compare, the one spelling of "dr_rollout equals K dr_step
launches bitwise", can fail: it raises on a pair that differs in an output,
and on a pair that differs only in a state field no output shows.  The
"smooth" case at f32, n = 65 (one full wave plus a wave with a single live
lane), K = 3."""
import pytest
import torch

from rollout_parity import CASES, compare, pair

pytestmark = pytest.mark.gpu
N, K, ROW = 65, 3, 64
CASE = CASES["smooth"]


def _run(change=None):
    """compare on a fresh pair, after change(b)."""
    from drone_rl_amd import random_actions
    a, b = pair(CASE, N, torch.float32)
    if change is not None:
        change(b)
    acts = torch.stack([random_actions(N, seed=3, step=t, env_id_offset=CASE.env_id_offset)
                        for t in range(K)])
    try:
        return compare(a, b, K, actions=acts, fields=CASE.fields)
    finally:
        a.close()
        b.close()


def _bump(field, value):
    def change(b):
        x = b.get(field).cpu()
        x[ROW] += value
        b.set(field, x)
    return change


def test_output_mismatch_is_caught():
    """vel of env 64 off by 2^-10 in the stepped batch: the first step's obs
    (which holds vel) differs."""
    with pytest.raises(AssertionError) as e:
        _run(_bump("vel", 2.0 ** -10))
    assert str(e.value).splitlines()[0] == "(0, 'obs')"


def test_state_only_mismatch_is_caught():
    """eps of env 64 differs in the stepped batch.  eps is read only by a
    reset, and env 64 ends no episode in the K steps (asserted on an unchanged
    pair: the runs are deterministic, and compare passes the changed pair's
    outputs before it reaches the fields), so every output is equal and the
    final field comparison alone must raise."""
    obs, rew, done = _run()
    assert not done[:, ROW].any()
    with pytest.raises(AssertionError) as e:
        _run(_bump("eps", 0.5))
    assert str(e.value).splitlines()[0] == "eps"
