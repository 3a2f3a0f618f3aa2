"""The "tag" env variant on the GPU: envs 2j / 2j+1 are
a pursuer / evader pair coupled through in-register lane exchanges.

The variant is this build's specification (the reference has none).  It is
pinned (a) to the gym variant, whose dynamics, step limit and resets it keeps
bit for bit; (b) to its own antisymmetry (one distance, two signs); (c) to the
NumPy restatement tests/tag_ref.py, built around the oracle's gym step, on
random states with pairs on both sides of the tag radius and drones that
crash.  Bars as for the gym and moving envs: done exact (f64), obs within
1e-5 * max(|ref|, 1), reward atol 2e-5, the role column exact.  Then every
layer above the step kernel: the pair's common reset, dr_reset_masked,
dr_rollout, the trainer with checkpoints, and the VecEnv facade.  The batch
sizes leave the last wave partly filled: 1030 = 16 * 64 + 6."""
import ctypes

import numpy as np
import pytest
import torch

from rollout_parity import check_rollout, check_rollout_random
from subproc import run_worker
from tag_ref import tag_random_state, tag_step

pytestmark = pytest.mark.gpu
VEC = ("pos", "vel", "euler", "omega", "target")
N = 1030


def _batch(n, variant="tag", **kw):
    from drone_rl_amd import DroneBatch
    return DroneBatch(n, variant, **kw)


def _hover_actions(n, t, seed=3):
    from drone_rl_amd import random_actions
    return random_actions(n, seed=seed, step=t, lo=2.2, hi=2.7)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_dynamics_are_the_gym_env(dtype):
    """Same seed, same near-hover actions (nobody crashes), max_steps 8, 40
    steps: each drone's own 12 obs floats, done, ep_num and current_step equal
    the gym variant's bitwise across five resets, and so do the carried target
    and the reset positions."""
    g = _batch(N, "gym", dtype=dtype, seed=11, max_steps=8)
    m = _batch(N, "tag", dtype=dtype, seed=11, max_steps=8)
    assert m.obs_dim == 19 and (m.tag_radius, m.crash_penalty) == (0.25, 0.0)
    og, om = g.reset(), m.reset()
    assert om.shape == (N, 19) and torch.equal(om[:, :12], og[:, :12])
    for t in range(40):
        a = _hover_actions(N, t)
        og, rg, dg = g.step(a)
        om, rm, dm = m.step(a)
        assert torch.equal(om[:, :12], og[:, :12]), t
        assert torch.equal(dm, dg), t
        # no crash occurred: the gym's done is the step limit alone
        assert bool(dg.all()) if t % 8 == 7 else not bool(dg.any()), t
        for k in ("ep_num", "current_step", "pos", "target", "eps"):
            assert torch.equal(m.get(k), g.get(k)), (t, k)
    # the constructor's reset, reset(), then five step-limit resets
    assert int(g.get("ep_num").min()) == 7
    g.close()
    m.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_antisymmetry(dtype):
    """Random actions, 210 steps (crashes, the step limit, resets): a pair
    ends together, the rewards are exact negatives at c = 0, so are the
    relative position / velocity obs, and the role is +-1 by parity."""
    from drone_rl_amd import random_actions
    b = _batch(N, dtype=dtype, seed=5)
    role = torch.ones(N, device="cuda")
    role[1::2] = -1.0
    obs = b.reset()
    assert torch.equal(obs[0::2, 12:18], -obs[1::2, 12:18]) and torch.equal(obs[:, 18], role)
    ends = torch.zeros(N, dtype=torch.int64, device="cuda")
    tagged = 0
    for t in range(210):
        obs, rew, done = b.step(random_actions(N, seed=9, step=t))
        assert torch.equal(done[0::2], done[1::2]), t
        assert torch.equal(rew[1::2], -rew[0::2]), t
        assert torch.equal(obs[0::2, 12:18], -obs[1::2, 12:18]), t
        assert torch.equal(obs[:, 18], role), t
        ends += done
        tagged += int((rew[0::2] > 0).sum())
    assert int(ends.min()) >= 1 and tagged > 0
    b.close()


def test_step_law_vs_restatement():
    """30 steps from random tumbling states at R = 0.25, c = 0.5, no
    auto-reset; the GPU state is re-synced to the restatement's after every
    step (the dynamics are chaotic, as in test_moving_gpu)."""
    from drone_rl_amd import random_actions
    n, R, C = 4098, 0.25, 0.5
    rng = np.random.default_rng(0)
    s = tag_random_state(n, rng, R)
    b = _batch(n, dtype=torch.float64, auto_reset=False, tag_radius=R, crash_penalty=C)
    for k in VEC:
        b.set(k, s[k])
    b.set("current_step", s["step"])
    inside = outside = crashes = 0
    for t in range(30):
        a = random_actions(n, seed=5, step=t)
        obs, rew, done = b.step(a)
        ro, rr, rd, rc = tag_step(s, a.cpu().numpy(), R, C)
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), rd)
        err = np.abs(obs[:, :18].astype(np.float64) - ro[:, :18]) / \
            np.maximum(np.abs(ro[:, :18].astype(np.float64)), 1.0)
        assert err.max() <= 1e-5, (t, err.max())
        np.testing.assert_allclose(rew, rr, rtol=0, atol=2e-5)
        np.testing.assert_array_equal(obs[:, 18], ro[:, 18])
        # the pursuer's reward before the penalty is positive exactly inside R
        g = rr[0::2] + np.where(rc[0::2], np.float32(C), np.float32(0))
        inside += int((g > 0).sum())
        outside += int((g <= 0).sum())
        crashes += int(rc.sum())
        for k in VEC[:4]:
            b.set(k, s[k])
    # the restatement's own output exercised both sides of the radius and the penalty
    assert inside >= 0.1 * 30 * n / 2 and outside >= 0.1 * 30 * n / 2, (inside, outside)
    assert crashes >= 0.01 * 30 * n, crashes
    np.testing.assert_array_equal(b.get("current_step").cpu().numpy(), s["step"])
    b.close()


def test_one_member_crashes_and_masked_reset():
    """Every third pair's pursuer starts 1 mm above the ground, descending: it
    crashes, both rows end and reset, neither is truncated, the crasher alone
    pays c; the survivor's terminal obs shows its own pre-reset state and the
    crasher's terminal position, the reset obs the partner's reset position.
    Then dr_reset_masked with one member's byte set resets the pair."""
    C = 0.5
    kw = dict(dtype=torch.float64, seed=7)
    b = _batch(N, keep_terminal_obs=True, monitor=True, crash_penalty=C, **kw)
    ref = _batch(N, auto_reset=False, **kw)          # c = 0, keeps the terminal state
    b.reset()
    ref.reset()
    pos, vel = b.get("pos").cpu().numpy(), b.get("vel").cpu().numpy()
    assert np.array_equal(pos, ref.get("pos").cpu().numpy())
    low = np.zeros(N, bool)
    low[0::6] = True                                 # the pursuers of pairs 0, 3, 6, ...
    pos[low, 2], vel[low, 2] = 0.001, -1.0
    for x in (b, ref):
        x.set("pos", pos)
        x.set("vel", vel)
    # and one pursuer (row 2) is a step from the limit: its pair is truncated
    cs = np.zeros(N, np.int32)
    cs[2] = 199
    for x in (b, ref):
        x.set("current_step", cs)
    limit = np.zeros(N, bool)
    limit[2:4] = True
    ep0 = b.get("ep_num").cpu().numpy()
    a = _hover_actions(N, 0)
    trunc = torch.full((N,), 7, dtype=torch.uint8, device="cuda")
    obs, rew, done = b.step(a, trunc_out=trunc)
    _, rew0, done0 = ref.step(a)
    obs, rew, done, rew0 = (x.cpu().numpy() for x in (obs, rew, done, rew0))
    crashed = low | np.roll(low, 1)                  # the crashers and their evaders
    pair_low = crashed | limit                       # every row whose pair ended
    np.testing.assert_array_equal(done.astype(bool), pair_low)
    np.testing.assert_array_equal(done0.cpu().numpy().astype(bool), pair_low)
    # truncated: ended with no crash on either side
    np.testing.assert_array_equal(trunc.cpu().numpy(), limit.astype(np.uint8))
    assert (trunc.cpu().numpy()[crashed] == 0).all()
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), ep0 + pair_low)
    step = b.get("current_step").cpu().numpy()
    assert (step[pair_low] == 0).all() and (step[~pair_low] == 1).all()
    # the penalty: one f32 subtract, on the crasher only
    np.testing.assert_array_equal(rew[~low], rew0[~low])
    np.testing.assert_array_equal(rew[low], rew0[low] - np.float32(C))
    np.testing.assert_array_equal(rew0[1::2], -rew0[0::2])
    # terminal obs of the pairs that ended, from the state ref kept
    tp, tv = ref.get("pos").cpu().numpy(), ref.get("vel").cpu().numpy()
    assert (tp[low, 2] < 0).all() and (tp[~low, 2] > 0.9).all()
    swap = np.arange(N) ^ 1
    term = b.term_obs.cpu().numpy()
    rows = np.flatnonzero(pair_low)
    np.testing.assert_array_equal(term[rows, 0:3], tp[rows].astype(np.float32))
    np.testing.assert_array_equal(term[rows, 3:6], tv[rows].astype(np.float32))
    np.testing.assert_array_equal(term[rows, 12:15], (tp[swap] - tp)[rows].astype(np.float32))
    np.testing.assert_array_equal(term[rows, 15:18], (tv[swap] - tv)[rows].astype(np.float32))
    np.testing.assert_array_equal(term[rows, 18], np.where(rows % 2 == 0, 1, -1))
    assert (term[~pair_low] == 0).all()
    # the obs after the step: every row sees its partner's current (reset) state
    np_, nv = b.get("pos").cpu().numpy(), b.get("vel").cpu().numpy()
    assert (np_[pair_low, 2] == 1.0).all() and (nv[pair_low] == 0).all()
    np.testing.assert_array_equal(obs[:, 0:3], np_.astype(np.float32))
    np.testing.assert_array_equal(obs[:, 12:15], (np_[swap] - np_).astype(np.float32))
    np.testing.assert_array_equal(obs[:, 15:18], (nv[swap] - nv).astype(np.float32))

    # masked reset: a byte on one member resets both
    ep1 = b.get("ep_num").cpu().numpy()
    mask = np.zeros(N, bool)
    mask[[5, 8, N - 1]] = True                       # an evader, a pursuer, the last row
    want = mask | mask[swap]
    assert want.sum() == 6
    b.set("current_step", np.full(N, 3, np.int32))
    obs = b.reset_masked(torch.from_numpy(mask)).cpu().numpy()
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), ep1 + want)
    np.testing.assert_array_equal(b.get("current_step").cpu().numpy(), np.where(want, 0, 3))
    p2 = b.get("pos").cpu().numpy()
    np.testing.assert_array_equal(p2[~want], np_[~want])
    assert (p2[want] != np_[want]).any()
    np.testing.assert_array_equal(obs[:, 0:3], p2.astype(np.float32))
    np.testing.assert_array_equal(obs[:, 12:15], (p2[swap] - p2).astype(np.float32))
    np.testing.assert_array_equal(obs[:, 18], np.where(np.arange(N) % 2 == 0, 1, -1))
    b.close()
    ref.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [N, 2])
def test_rollout_is_bitwise_k_steps(dtype, n):
    """dr_rollout / dr_rollout_random (the one-role kernel, the exchanges in
    registers) against K = 24 dr_step launches: outputs and every state
    field, with the pairs' resets inside the launch (max_steps 7)."""
    check_rollout("tag", n, 24, dtype)
    check_rollout_random("tag", n, 24, dtype)


def test_rollout_vs_half_populated_step_waves(monkeypatch):
    """DRONERL_ROWS_PER_WAVE=32 (read by dr_create) puts 32 envs on a wave of
    the step kernel; the rollout keeps 64.  Same bits."""
    monkeypatch.setenv("DRONERL_ROWS_PER_WAVE", "32")
    check_rollout("tag", N, 24, torch.float64)
    check_rollout("tag", 2, 24, torch.float32)


def test_rollout_ignores_the_warp_specialised_override():
    """DRONERL_ROLLOUT_WS=1 forces the warp-specialised rollout forms for the
    other variants; this one has only the one-role kernel and must keep it
    (the override is read once per process, hence the subprocess)."""
    run_worker("rollout_parity.py", "tag", "f64", f"{N},2", "24", DRONERL_ROLLOUT_WS="1")


def test_set_tag_abi():
    from drone_rl_amd import _lib
    b = _batch(4, auto_reset=False)
    L = _lib.lib()
    r, c = ctypes.c_float(), ctypes.c_float()
    assert L.dr_get_tag(b.handle, ctypes.byref(r), ctypes.byref(c)) == _lib.DR_OK
    assert (r.value, c.value) == (0.25, 0.0)
    assert L.dr_get_tag(b.handle, None, None) == _lib.DR_OK
    for bad in ((0.0, 0.0), (-1.0, 0.0), (float("nan"), 0.0), (float("inf"), 0.0),
                (0.25, -1.0), (0.25, float("inf")), (0.25, float("nan"))):
        assert L.dr_set_tag(b.handle, *bad) == _lib.DR_ERR_INVALID, bad
    assert L.dr_obs_dim(b.handle) == 19
    # a new radius acts on the next step: two hovering drones 0.28 m apart
    b.reset()
    pos = np.array([[0, 0, 1.0], [0.28, 0, 1.0], [0, 0, 1.0], [0.5, 0, 1.0]])
    b.set("pos", pos)
    a = torch.full((4, 4), 2.45, device="cuda")
    _, rew, _ = b.step(a)
    assert rew[0] < 0 and rew[1] == -rew[0]
    b.set_tag(0.3, 0.5)
    assert L.dr_get_tag(b.handle, ctypes.byref(r), ctypes.byref(c)) == _lib.DR_OK
    assert (r.value, c.value) == (float(np.float32(0.3)), 0.5)
    assert (b.tag_radius, b.crash_penalty) == (float(np.float32(0.3)), 0.5)
    _, rew, _ = b.step(a)
    rew = rew.cpu().numpy()
    assert rew[0] > 0.99 and rew[1] == -rew[0] and rew[2] < 0 and rew[3] == -rew[2]
    g = _batch(4, "gym")
    assert L.dr_set_tag(g.handle, 0.25, 0.0) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_get_tag(g.handle, ctypes.byref(r), ctypes.byref(c)) == _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        g.set_tag(0.25, 0.0)
    b.close()
    g.close()


# ---- trainer, checkpoints, VecEnv ------------------------------------------
def _trainer():
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    return PPOTrainer(PPOConfig(num_envs=256, n_steps=8, batch_size=1024, n_epochs=2,
                                net_arch=(256, 256), seed=5, variant="tag", tag_radius=0.3,
                                crash_penalty=0.1))


def test_trainer_fused_graph_and_checkpoint(tmp_path):
    """Self-play with one shared net: the trainer stays on the fused path at
    obs width 19; the captured rollout graph is bitwise the eager rollout; a
    checkpoint carries the two parameters in its config and resumes bit for
    bit; episode_stats reports the roles apart."""
    a, b = _trainer(), _trainer()
    b.rollout_graph = False
    assert a.use_fused and a.obs.shape[-1] == 19
    assert (a.env.tag_radius, a.env.crash_penalty) == (float(np.float32(0.3)),
                                                       float(np.float32(0.1)))
    assert a._graph_key("rollout")[-4:-2] == (a.env.tag_radius, a.env.crash_penalty)
    path = tmp_path / "ck.pt"
    for it in range(2):
        if it == 1:
            a.save(path)
        sa, sb = a.learn_step(), b.learn_step()
        assert torch.isfinite(sa).all() and torch.equal(sa, sb)
        for name in ("obs", "actions", "rewards", "dones", "adv"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
    assert a._rgraph is not None and b._rgraph is None
    assert torch.isfinite(a.policy.flat).all()
    role = a.obs[..., 18]
    assert bool((role[..., 0::2] == 1).all()) and bool((role[..., 1::2] == -1).all())
    es = a.episode_stats()
    assert {"ep_rew_mean", "ep_len_mean", "episodes", "ep_rew_mean_pursuer",
            "ep_rew_mean_evader"} <= set(es)
    assert all(np.isfinite(v) for v in es.values())
    cfg = torch.load(path, weights_only=True)["config"]
    assert (cfg["variant"], cfg["tag_radius"], cfg["crash_penalty"]) == ("tag", 0.3, 0.1)
    c = _trainer()
    c.load(path)
    c.learn_step()
    assert torch.equal(a.policy.flat.detach(), c.policy.flat.detach())
    for k in ("pos", "vel", "ep_num", "current_step"):
        assert torch.equal(a.env.get(k), c.env.get(k)), k
    assert a.num_timesteps == c.num_timesteps
    k0 = a._graph_key("rollout")
    a.env.set_tag(0.2, 0.1)
    assert a._graph_key("rollout") != k0
    for t in (a, b, c):
        t.close()


def test_vec_env_facade():
    from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv
    v = BatchedDroneVecEnv(4, variant="tag", seed=3, tag_radius=0.3)
    assert v.num_envs == 4 and v.observation_space.shape == (19,)
    assert v.batch.obs_dim == 19 and v.batch.tag_radius == float(np.float32(0.3))
    obs = v.reset()
    assert obs.shape == (4, 19) and (obs[:, 18] == [1, -1, 1, -1]).all()
    obs, rew, done, infos = v.step(np.full((4, 4), 2.45, np.float32))
    assert obs.shape == (4, 19) and not done.any()
    assert (rew[1::2] == -rew[0::2]).all() and (obs[0::2, 12:18] == -obs[1::2, 12:18]).all()
    v.close()
    with pytest.raises(ValueError):
        DroneVectorEnv(4, seed=3, variant="tag")
