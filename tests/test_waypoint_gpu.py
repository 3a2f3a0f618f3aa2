"""The gym env's waypoint courses on the GPU (DESIGN.md section 18;
dr_set_waypoints): the target moves on to a fresh draw when the drone reaches
it.

The option is this build's specification (the reference has none).  It is
pinned (a) to the gym variant, which it reproduces bit for bit at eps 0 with
the gym's radius and bonus, and whose physics, done and resets it keeps at any
values; (b) to the NumPy restatement tests/waypoint_ref.py, built around the
oracle's gym step, on random states.  Bars as for the gym env: done exact
(f64), obs within 1e-5 * max(|ref|, 1), reward atol 2e-5; targets and counters
are compared exactly.  Then every layer above the step kernel: resets,
dr_rollout, the trainer with checkpoints, and the VecEnv facades.  Every test
asserts a minimum number of reaches, so none passes with the feature idle."""
import numpy as np
import pytest
import torch

import waypoint_ref
from rollout_parity import check_rollout, check_rollout_random
from shared import gym_batch as _batch
from subproc import run_worker
from trainer_checks import (graph_equals_eager_and_resumes, graph_key_changes, plain_trainer,
                            small_trainer)

pytestmark = pytest.mark.gpu
VEC = ("pos", "vel", "euler", "omega", "target")
STATE = VEC + ("current_step", "ep_num", "eps")


def _bits(t):
    a = np.ascontiguousarray(t.cpu().numpy() if torch.is_tensor(t) else t)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _eps(b, value):
    b.set("eps", torch.full((b.num_envs,), float(value), dtype=torch.float64))


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_eps0_with_the_gym_radius_is_the_gym_env(dtype):
    """eps 0, (R, B) = (0.05, 1): obs, reward, done, terminal obs, ep_num and
    every state field equal a gym batch's bitwise over 210 steps (every env
    passes the 200-step limit; many crash earlier).  Every waypoint is (0, 0,
    1) again, and the reach counters hold the number of gym bonuses paid."""
    from drone_rl_amd import random_actions
    n = 1031
    g = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True)
    w = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True, reach_radius=0.05,
               reach_bonus=1.0)
    assert w.waypoints_enabled and not g.waypoints_enabled
    assert (w.reach_radius, w.reach_bonus) == (float(np.float32(0.05)), 1.0)
    with pytest.raises(Exception):
        g.get("waypoint")
    assert torch.equal(w.reset(), g.reset())
    assert w.get("waypoint").dtype == torch.int32 and not w.get("waypoint").any()
    bonuses = 0
    for t in range(210):
        a = random_actions(n, seed=3, step=t)
        og, rg, dg = g.step(a)
        ow, rw, dw = w.step(a)
        assert torch.equal(ow, og), t
        assert torch.equal(rw, rg) and torch.equal(dw, dg), t
        assert torch.equal(w.term_obs, g.term_obs), t
        bonuses += int((rg > 0).sum())
    for k in STATE:
        assert torch.equal(w.get(k), g.get(k)), k
    q = int(w.get("waypoint")[:, 1].sum())
    print(f"eps 0 ({dtype}): reaches {q}, gym bonuses {bonuses}")
    assert q == bonuses
    assert q >= 100
    g.close()
    w.close()


def test_physics_done_and_resets_do_not_depend_on_the_course():
    """eps 1, (R, B) = (1, 1), 210 steps: obs[:, :12] and done are the gym's
    bitwise throughout (the physics never reads the target); a row that stood
    at its episode's first waypoint before the step and did not reach it has
    the gym's whole obs row and reward."""
    from drone_rl_amd import random_actions
    n = 1031
    g = _batch(n, seed=11)
    w = _batch(n, seed=11, reach_radius=1.0, reach_bonus=1.0)
    for x in (g, w):
        _eps(x, 1.0)
    assert torch.equal(w.reset(), g.reset())
    wp0 = w.get("waypoint")
    same_rows = 0
    for t in range(210):
        a = random_actions(n, seed=3, step=t)
        og, rg, dg = g.step(a)
        ow, rw, dw = w.step(a)
        assert torch.equal(ow[:, :12], og[:, :12]) and torch.equal(dw, dg), t
        wp1 = w.get("waypoint")
        first = (wp0[:, 0] == 0) & (wp1[:, 1] == wp0[:, 1])
        assert torch.equal(ow[first], og[first]) and torch.equal(rw[first], rg[first]), t
        same_rows += int(first.sum())
        wp0 = wp1
    for k in ("pos", "vel", "euler", "omega", "current_step", "ep_num", "eps"):
        assert torch.equal(w.get(k), g.get(k)), k
    q = int(wp0[:, 1].sum())
    print(f"physics independence: reaches {q}, first-waypoint rows compared {same_rows}")
    assert q >= 8000
    assert same_rows >= n
    assert not torch.equal(w.get("target"), g.get("target"))
    g.close()
    w.close()


def test_step_law_vs_restatement():
    """30 steps from random tumbling states, f64, no auto-reset, R = 0.25, B =
    2.5, per-env eps from {0, 0.5, 1.3}, random ep_num, a few rows at j =
    70000; before each step the even rows' target is put at the drone, so they
    reach.  The GPU state is re-synced to the restatement's after every step
    (the dynamics are chaotic, as in test_moving_gpu); target and counters are
    never re-synced: they are exact.  A row whose distance is within 1e-9 of R
    may fall either way in the last ulp and is skipped (and then re-synced):
    at most 2 in the whole test (on the CPU none came within 1e-6)."""
    from test_moving_gpu import _random_state

    from drone_rl_amd import random_actions
    n, seed, off = 4099, 21, 3
    p = dict(reach_radius=0.25, reach_bonus=2.5)
    rng = np.random.default_rng(0)
    s = _random_state(n, rng, eps=0.0)
    del s["motion"]
    s["eps"] = rng.choice([0.0, 0.5, 1.3], n)
    s["ep_num"] = rng.integers(1, 5000, n).astype(np.int32)
    s["waypoint"] = np.zeros((n, 2), np.int32)
    s["waypoint"][::98, 0] = 70000         # even rows: they reach at every step
    b = _batch(n, dtype=torch.float64, auto_reset=False, seed=seed, env_id_offset=off, **p)
    for k in VEC:
        b.set(k, s[k])
    b.set("current_step", s["step"])
    b.set("eps", s["eps"])
    b.set("ep_num", s["ep_num"])
    b.set("waypoint", s["waypoint"])
    np.testing.assert_array_equal(b.get("waypoint").cpu().numpy(), s["waypoint"])
    ids = torch.tensor([98, 4098, 0], dtype=torch.int32, device="cuda")
    got = b.gather("waypoint", ids)
    assert got.shape == (3, 2) and got.dtype == torch.int32
    np.testing.assert_array_equal(got.cpu().numpy(), s["waypoint"][[98, 4098, 0]])
    gids = np.arange(n, dtype=np.uint64) + off
    worst_obs = worst_rew = 0.0
    skipped = 0
    R = float(np.float32(p["reach_radius"]))
    for t in range(30):
        s["target"][::2] = s["pos"][::2]
        b.set("target", s["target"])
        a = random_actions(n, seed=5, step=t)
        obs, rew, done = b.step(a)
        ro, rr, rd, reached, d = waypoint_ref.waypoint_step(s, a.cpu().numpy(), p, seed, gids)
        ok = ~(np.abs(d - R) < 1e-9)
        skipped += int((~ok).sum())
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), rd)
        err = np.abs(obs.astype(np.float64) - ro) / np.maximum(np.abs(ro.astype(np.float64)), 1.0)
        worst_obs = max(worst_obs, float(err[ok].max()))
        worst_rew = max(worst_rew, float(np.abs(rew - rr)[ok].max()))
        assert err[ok].max() <= 1e-5, (t, err[ok].max())
        np.testing.assert_allclose(rew[ok], rr[ok], rtol=0, atol=2e-5)
        np.testing.assert_array_equal(_bits(b.get("target"))[ok], _bits(s["target"])[ok])
        np.testing.assert_array_equal(b.get("waypoint").cpu().numpy()[ok], s["waypoint"][ok])
        assert reached.mean() >= 0.45, (t, reached.mean())
        assert reached[::2].all()
        for k in VEC[:4]:
            b.set(k, s[k])
        if not ok.all():
            b.set("target", s["target"])
            b.set("waypoint", s["waypoint"])
    print(f"waypoint step law: worst obs error {worst_obs:.3e}, worst reward error "
          f"{worst_rew:.3e}, rows skipped {skipped}, reaches {int(s['waypoint'][:, 1].sum())}")
    assert skipped <= 2
    # the three curriculum levels and the preset indices were all live
    assert (s["waypoint"][::98, 0] == 70030).all() and (s["waypoint"][::2, 1] == 30).all()
    z = s["eps"][::2] == 0.0
    np.testing.assert_array_equal(s["target"][::2][z], np.broadcast_to([0.0, 0.0, 1.0],
                                                                       (int(z.sum()), 3)))
    assert (s["target"][::2][~z, 0] > 0).all()
    np.testing.assert_array_equal(b.get("current_step").cpu().numpy(), s["step"])
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), s["ep_num"])
    b.close()


def test_draws_belong_to_the_env_not_the_batch():
    """A batch of 512 at env_id_offset 1024 is, over 20 steps with resets
    (max_steps 8), rows 1024..1535 of a 2,048-env batch with the same seed:
    waypoints are keyed by the global env id; and every current waypoint past
    an episode's first is waypoint_ref's draw for (env, episode, index)."""
    from drone_rl_amd import random_actions
    kw = dict(seed=31, max_steps=8, reach_radius=1.0, reach_bonus=1.0)
    small = _batch(512, env_id_offset=1024, **kw)
    big = _batch(2048, **kw)
    for x in (small, big):
        _eps(x, 1.0)
    assert torch.equal(small.reset(), big.reset()[1024:1536])
    for t in range(20):
        ab = random_actions(2048, seed=4, step=t)
        a_s = random_actions(512, seed=4, step=t, env_id_offset=1024)
        assert torch.equal(a_s, ab[1024:1536])
        o1, r1, d1 = small.step(a_s)
        o2, r2, d2 = big.step(ab)
        assert torch.equal(o1, o2[1024:1536]) and torch.equal(d1, d2[1024:1536]), t
        assert torch.equal(r1, r2[1024:1536]), t
    for k in STATE + ("waypoint",):
        assert torch.equal(small.get(k), big.get(k)[1024:1536]), k
    assert int(small.get("ep_num").min()) >= 3
    wp = big.get("waypoint").cpu().numpy()
    ep = big.get("ep_num").cpu().numpy()
    tgt = big.get("target").cpu().numpy()
    on = wp[:, 0] >= 1
    print(f"draws: reaches {int(wp[:, 1].sum())} (rows 1024..1535: "
          f"{int(wp[1024:1536, 1].sum())}), rows past their first waypoint {int(on.sum())}")
    assert on.sum() >= 200
    np.testing.assert_array_equal(
        _bits(tgt[on]), _bits(waypoint_ref.waypoint(31, np.arange(2048)[on], ep[on], wp[on, 0],
                                                    1.0)))
    assert wp[:, 1].sum() >= 4000
    small.close()
    big.close()


def test_auto_reset_reset_masked_reset_and_enabling():
    """j is zeroed where a reset happened and only there (auto-reset, dr_reset,
    reset_masked); q is kept, a reach in the terminal step included; enabling
    the option mid-episode leaves every other field as it was.  All at
    env_id_offset 2^33."""
    from drone_rl_amd import _lib, random_actions
    n, seed, off = 1031, 7, 1 << 33
    rng = np.random.default_rng(1)
    b = _batch(n, seed=seed, env_id_offset=off, reach_radius=1.0, reach_bonus=1.0)
    _eps(b, 1.0)
    b.reset()
    wp0 = np.stack([rng.integers(0, 9, n), rng.integers(0, 1000, n)], 1).astype(np.int32)
    b.set("waypoint", wp0)
    step0 = np.where(np.arange(n) % 2 == 0, 199, 3).astype(np.int32)
    b.set("current_step", step0)
    tgt = b.get("target").cpu().numpy()
    tgt[::3] = b.get("pos").cpu().numpy()[::3]      # every third row reaches
    b.set("target", tgt)
    ep0 = b.get("ep_num").cpu().numpy()
    obs, rew, done = b.step(random_actions(n, seed=2, step=0))
    done = done.cpu().numpy().astype(bool)
    assert done[::2].all() and not done[1::2].all()
    wp1 = b.get("waypoint").cpu().numpy()
    dq = wp1[:, 1] - wp0[:, 1]
    assert set(np.unique(dq)) <= {0, 1} and dq[::3].all()
    assert (done & (dq == 1)).sum() >= n // 8       # reaches in the terminal step: counted
    assert (rew.cpu().numpy()[dq == 1] > 0.9).all() and (rew.cpu().numpy()[dq == 0] < 0).all()
    np.testing.assert_array_equal(wp1[:, 0], np.where(done, 0, wp0[:, 0] + dq))
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), ep0 + done)
    # the masked reset
    b.set("waypoint", wp0)
    mask = torch.from_numpy(rng.uniform(size=n) < 0.5)
    assert 0 < int(mask.sum()) < n
    b.reset_masked(mask)
    mk = mask.numpy()
    np.testing.assert_array_equal(b.get("waypoint").cpu().numpy(),
                                  np.stack([np.where(mk, 0, wp0[:, 0]), wp0[:, 1]], 1))
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), ep0 + done + mk)
    # dr_reset
    b.set("waypoint", wp0)
    b.reset()
    np.testing.assert_array_equal(b.get("waypoint").cpu().numpy(),
                                  np.stack([np.zeros(n, np.int32), wp0[:, 1]], 1))
    b.close()
    # enabling mid-episode
    g = _batch(n, seed=seed, env_id_offset=off, max_steps=5)
    _eps(g, 1.0)
    g.reset()
    for t in range(7):
        g.step(random_actions(n, seed=2, step=t))
    assert int(g.get("ep_num").min()) >= 2
    before = {k: g.get(k) for k in STATE}
    g.set_waypoints(0.25, 1.0)
    assert g.waypoints_enabled
    for k in STATE:
        assert torch.equal(g.get(k), before[k]), k
    assert not g.get("waypoint").any()
    # and a later call changes the two values only
    g.set("waypoint", wp0)
    g.set_waypoints(0.5, 0.0)
    assert (g.reach_radius, g.reach_bonus) == (0.5, 0.0)
    np.testing.assert_array_equal(g.get("waypoint").cpu().numpy(), wp0)
    assert _lib.lib().dr_obs_dim(g.handle) == 15
    g.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rollout_is_bitwise_k_steps(dtype):
    """dr_rollout / dr_rollout_random (the one-role kernel; waypoint, index
    and counter in registers) against K dr_step launches: outputs and every
    state field, `waypoint` included, with reaches and resets inside the
    launch (max_steps 16 < K)."""
    reaches, deep = check_rollout("waypoint", 777, 37, dtype)
    reaches_random, _ = check_rollout_random("waypoint", 777, 37, dtype)
    print(f"rollout ({dtype}): reaches {reaches} / {reaches_random} (in-kernel actions), "
          f"envs that held j >= 3: {deep}")
    assert reaches >= 2000 and reaches_random >= 2000
    assert deep >= 200


def test_rollout_ignores_the_warp_specialised_override():
    """DRONERL_ROLLOUT_WS=1 forces the warp-specialised rollout forms for a
    plain gym handle; a waypoint handle has only the one-role kernel and must
    keep it (the override is read once per process, hence the subprocess)."""
    run_worker("rollout_parity.py", "waypoint", "f64", "777", "37", DRONERL_ROLLOUT_WS="1")


# ---- trainer, checkpoints, VecEnv ------------------------------------------
def _trainer():
    return small_trainer(reach_radius=0.25, reach_bonus=1.0)


def test_trainer_fused_graph_and_checkpoint(tmp_path):
    """The trainer stays on the fused path (the obs is the gym's 15 floats);
    the captured rollout graph is bitwise the eager rollout; a checkpoint
    carries the course parameters and field and resumes bit for bit, also into
    a trainer built without the option; episode_stats reports the waypoints
    per episode."""
    def make():
        t = _trainer()
        assert t.use_fused and t.obs.shape[-1] == 15 and t.env.waypoints_enabled
        assert (t.env.reach_radius, t.env.reach_bonus) == (0.25, 1.0)
        return t

    def plain():
        t = small_trainer()
        assert not t.env.waypoints_enabled
        return t

    def at_save(sd):
        assert sd["env"]["waypoint"].dtype == torch.int32
        assert sd["config"]["reach_radius"] == 0.25 and sd["config"]["reach_bonus"] == 1.0

    def per_iter(a, x):
        # x: the eager twin, or a trainer that loaded the checkpoint and stepped once
        assert x.env.waypoints_enabled
        assert (x.env.reach_radius, x.env.reach_bonus) == (0.25, 1.0)
        ea, ex = a.episode_stats(), x.episode_stats()
        assert ea == ex and np.isfinite(ea["ep_waypoints_mean"]) and ea["ep_waypoints_mean"] >= 0

    def after(a, b):
        # the reaches of the last rollout are what the counters gained in it
        assert torch.equal(a.env.get("waypoint"), b.env.get("waypoint"))
        assert int(a.env.get("waypoint")[:, 1].sum()) >= 16     # eps 0: starts within 0.25 m reach

    graph_equals_eager_and_resumes(make, tmp_path, field="waypoint", field_shape=(2048, 2),
                                   resume_fields=("pos", "target", "waypoint", "ep_num"),
                                   at_save=at_save, per_iter=per_iter, after=after,
                                   resume_into=(plain,))


def test_graph_key_follows_set_waypoints():
    """A changed parameter drops the captured rollout graph's key; its last
    two entries stay the smoothing pair."""
    a = _trainer()
    k0, k1 = graph_key_changes(a, lambda env: env.set_waypoints(0.5, 1.0))
    assert k1[-2:] == k0[-2:] == (a.env.motor_alpha, a.env.rate_penalty)
    graph_key_changes(a, lambda env: env.set_waypoints(0.5, 2.0))
    a.close()
    g = plain_trainer()
    assert "ep_waypoints_mean" not in g.episode_stats()
    # enabling changes the kernels a graph would hold
    graph_key_changes(g, lambda env: env.set_waypoints())
    assert (g.env.reach_radius, g.env.reach_bonus) == (0.25, 1.0)
    g.close()


def test_set_waypoints_abi():
    import ctypes

    from drone_rl_amd import DroneBatch, _lib
    L = _lib.lib()
    v = [ctypes.c_float(7.0) for _ in range(2)]
    g = _batch(8)
    assert L.dr_get_waypoints(g.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == [0.0, 0.0]               # before enabling
    buf = torch.zeros(8, 2, dtype=torch.int32, device="cuda")
    for fn in (L.dr_get_state, L.dr_set_state):
        assert fn(g.handle, _lib.FIELDS["waypoint"], buf.data_ptr(), None) == \
            _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(_lib.DroneRLError):
        g.get("waypoint")
    with pytest.raises(_lib.DroneRLError):
        g.set("waypoint", np.zeros((8, 2), np.int32))
    for bad in ((0.0, 1.0), (-0.25, 1.0), (float("nan"), 1.0), (float("inf"), 1.0),
                (0.25, -1.0), (0.25, float("nan")), (0.25, float("inf"))):
        assert L.dr_set_waypoints(g.handle, *bad) == _lib.DR_ERR_INVALID, bad
    assert L.dr_get_state(g.handle, _lib.FIELDS["waypoint"], buf.data_ptr(), None) == \
        _lib.DR_ERR_UNSUPPORTED                             # the refusals enabled nothing
    b = _batch(8, reach_radius=0.25, reach_bonus=2.5)
    assert L.dr_get_waypoints(b.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == [0.25, 2.5]
    assert L.dr_get_waypoints(b.handle, None, None) == _lib.DR_OK
    assert L.dr_set_waypoints(b.handle, 0.0, 1.0) == _lib.DR_ERR_INVALID     # no way back
    assert L.dr_set_waypoints(b.handle, 0.25, 0.0) == _lib.DR_OK             # B = 0 is allowed
    assert L.dr_obs_dim(b.handle) == 15
    # wind and waypoints exclude each other; the neutral wind call stays legal
    assert L.dr_set_wind(b.handle, 0.5, 0.0, 0.0, 0.0) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_set_wind(b.handle, 0.0, 0.0, 0.0, 0.0) == _lib.DR_OK
    with pytest.raises(ValueError):
        b.set_wind(0.5, 0, 0, 0)
    w = _batch(8, drag=0.5)
    assert L.dr_set_waypoints(w.handle, 0.25, 1.0) == _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        w.set_waypoints(0.25, 1.0)
    z = _batch(8)
    z.set_wind(0, 0, 0, 0)                                  # enabled nothing
    z.set_waypoints(0.25, 1.0)
    sm = DroneBatch(8, "smooth")
    assert L.dr_set_waypoints(sm.handle, 0.25, 1.0) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_get_waypoints(sm.handle, None, None) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_get_state(sm.handle, _lib.FIELDS["waypoint"], buf.data_ptr(), None) == \
        _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sm.set_waypoints(0.25, 1.0)
    long = _batch(8, max_steps=1 << 24)
    assert L.dr_set_waypoints(long.handle, 0.25, 1.0) == _lib.DR_ERR_UNSUPPORTED
    for x in (g, b, w, z, sm, long):
        x.close()


def test_vec_env_facades():
    from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv
    hover = np.full((4, 4), 9.81 / 4, np.float32)
    v = BatchedDroneVecEnv(4, seed=3, reach_radius=2.0, reach_bonus=3.0)
    assert v.observation_space.shape == (15,)
    obs = v.reset()
    assert obs.shape == (4, 15)
    # eps 0: the start is within 0.71 m of (0, 0, 1), so every env reaches
    obs, rew, done, infos = v.step(hover)
    assert obs.shape == (4, 15) and not done.any()
    assert (rew > 2.9).all()
    wp = np.stack(v.get_attr("waypoint"))
    assert wp.dtype == np.int32
    np.testing.assert_array_equal(wp, np.ones((4, 2), np.int32))
    np.testing.assert_array_equal(v.get_attr("waypoint", [2])[0], [1, 1])
    np.testing.assert_array_equal(np.stack(v.get_attr("target")),
                                  np.broadcast_to([0.0, 0.0, 1.0], (4, 3)))
    v.close()
    plain = BatchedDroneVecEnv(4, seed=3)
    with pytest.raises(AttributeError):
        plain.get_attr("waypoint")
    plain.close()
    e = DroneVectorEnv(4, seed=3, reach_bonus=3.0)          # the radius takes its default
    assert e.single_observation_space.shape == (15,)
    assert e.observation_space.shape == (4, 15)
    o, _ = e.reset()
    assert o.shape == (4, 15) and e.batch.waypoints_enabled
    assert (e.batch.reach_radius, e.batch.reach_bonus) == (0.25, 3.0)
    e.step(hover)
    wp = e.get_attr("waypoint")
    assert wp.shape == (4, 2) and wp.dtype == np.int32 and (wp[:, 0] == wp[:, 1]).all()
    e.close()
    with pytest.raises(AttributeError):
        e2 = DroneVectorEnv(4, seed=3)
        try:
            e2.get_attr("waypoint")
        finally:
            e2.close()
