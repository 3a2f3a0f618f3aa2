"""The gym env's wind option on the GPU (dr_set_wind):
linear drag, a per-episode mean wind and AR(1) gusts in front of the gym step.

The option is this build's specification (the reference has none).  It is
pinned (a) to the gym variant, which it reproduces bit for bit at the neutral
parameters, and through it to the reference's golden vectors; (b) to the
NumPy restatement tests/wind_ref.py, built around the oracle's gym step, on
random states.  Bars as for the gym env: done exact (f64), obs within 1e-5 *
max(|ref|, 1), reward atol 2e-5; the wind state is exact f32 and compared
bitwise.  Then every layer above the step kernel: resets, dr_rollout, the
trainer with checkpoints, and the VecEnv facades."""
import numpy as np
import pytest
import torch

import wind_ref
from rollout_parity import check_rollout, check_rollout_random
from shared import f32_bits as _bits, gym_batch as _batch
from subproc import run_worker
from trainer_checks import (graph_equals_eager_and_resumes, graph_key_changes, plain_trainer,
                            small_trainer)

pytestmark = pytest.mark.gpu
VEC = ("pos", "vel", "euler", "omega", "target")
WIND = dict(drag=0.5, wind_speed=2.0, gust_sigma=0.5, gust_rate=0.1)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_neutral_is_the_gym_env(dtype):
    """A gym batch, a batch after set_wind(0, 0, 0, 0) (which enables nothing)
    and a batch whose wind was enabled and then set to all zeros (the wind
    kernels at the neutral parameters): obs, reward, done, terminal obs and
    ep_num equal bitwise over 210 steps (every env passes the 200-step limit;
    many crash earlier)."""
    from drone_rl_amd import random_actions
    n = 1031
    g = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True)
    z = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True)
    z.set_wind(0, 0, 0, 0)
    w = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True, **WIND)
    w.set_wind(0, 0, 0, 0)
    assert not z.wind_enabled and w.wind_enabled
    with pytest.raises(Exception):
        z.get("wind")
    assert (w.drag, w.wind_speed, w.gust_sigma, w.gust_rate) == (0.0, 0.0, 0.0, 0.0)
    og = g.reset()
    for x in (z, w):
        assert torch.equal(x.reset(), og)
    assert not w.get("wind").any()          # drawn at W = 0: zeros
    done_count = torch.zeros(n, dtype=torch.int64, device="cuda")
    early = 0
    for t in range(210):
        a = random_actions(n, seed=3, step=t)
        og, rg, dg = g.step(a)
        for x in (z, w):
            ox, rx, dx = x.step(a)
            assert torch.equal(ox, og), t
            assert torch.equal(rx, rg) and torch.equal(dx, dg), t
            assert torch.equal(x.term_obs, g.term_obs), t
        done_count += dg
        if t < 199:
            early += int(dg.sum())
    assert int(done_count.min()) >= 1 and early > n // 2
    for x in (z, w):
        assert torch.equal(x.get("ep_num"), g.get("ep_num"))
        for k in VEC:
            assert torch.equal(x.get(k), g.get(k)), k
    assert not w.get("wind").any()
    for x in (g, z, w):
        x.close()


def test_step_law_vs_restatement():
    """30 steps from random tumbling states with random mean wind and gust
    written through set("wind"), k = 0.5, sigma = 0.5, beta = 0.1, no
    auto-reset; the GPU state is re-synced to the restatement's after every
    step (the dynamics are chaotic, as in test_moving_gpu).  The wind field is
    never re-synced: it is bitwise."""
    from test_moving_gpu import _random_state

    from drone_rl_amd import random_actions
    n, seed, off = 4099, 21, 3
    rng = np.random.default_rng(0)
    s = _random_state(n, rng, eps=0.0)
    del s["motion"]
    s["wind"] = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.normal(0, 0.5, (n, 3))],
                               1).astype(np.float32)
    p = dict(drag=0.5, wind_speed=2.0, gust_sigma=0.5, gust_rate=0.1)
    b = _batch(n, dtype=torch.float64, auto_reset=False, seed=seed, env_id_offset=off, **p)
    for k in VEC:
        b.set(k, s[k])
    b.set("current_step", s["step"])
    b.set("wind", s["wind"])
    s["ep_num"] = b.get("ep_num").cpu().numpy()
    assert (s["ep_num"] == 1).all()
    gids = np.arange(n, dtype=np.uint64) + off
    np.testing.assert_array_equal(b.get("wind").cpu().numpy(), s["wind"])
    ids = torch.tensor([5, 4098, 0], dtype=torch.int32, device="cuda")
    np.testing.assert_array_equal(b.gather("wind", ids).cpu().numpy(), s["wind"][[5, 4098, 0]])
    worst_obs = worst_rew = 0.0
    for t in range(30):
        a = random_actions(n, seed=5, step=t)
        v0 = s["vel"].copy()
        obs, rew, done = b.step(a)
        ro, rr, rd = wind_ref.wind_step(s, a.cpu().numpy(), p, seed, gids)
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), rd)
        err = np.abs(obs.astype(np.float64) - ro) / np.maximum(np.abs(ro.astype(np.float64)), 1.0)
        worst_obs = max(worst_obs, float(err.max()))
        worst_rew = max(worst_rew, float(np.abs(rew - rr).max()))
        assert err.max() <= 1e-5, (t, err.max())
        np.testing.assert_allclose(rew, rr, rtol=0, atol=2e-5)
        np.testing.assert_array_equal(_bits(b.get("wind")), s["wind"].view(np.uint32))
        for k in VEC[:4]:
            b.set(k, s[k])
    print(f"wind step law: worst obs error {worst_obs:.3e}, worst reward error {worst_rew:.3e}")
    # the disturbance was live: the gusts moved and the drag changed the velocity
    assert 0.4 < s["wind"][:, 3:].std() < 0.6          # sigma = 0.5
    assert np.abs(s["vel"] - v0).max() > 0.01
    np.testing.assert_array_equal(b.get("current_step").cpu().numpy(), s["step"])
    b.close()


def test_draws_belong_to_the_env_not_the_batch():
    """A batch of 512 at env_id_offset 1024 holds, after 20 steps with resets
    (max_steps 8), the wind of rows 1024..1535 of a 2,048-env batch with the
    same seed: mean wind and gusts are keyed by the global env id."""
    from drone_rl_amd import random_actions
    small = _batch(512, seed=31, env_id_offset=1024, max_steps=8, **WIND)
    big = _batch(2048, seed=31, max_steps=8, **WIND)
    os_, ob = small.reset(), big.reset()
    assert torch.equal(os_, ob[1024:1536])
    for t in range(20):
        ab = random_actions(2048, seed=4, step=t)
        a_s = random_actions(512, seed=4, step=t, env_id_offset=1024)
        assert torch.equal(a_s, ab[1024:1536])
        o1, r1, d1 = small.step(a_s)
        o2, r2, d2 = big.step(ab)
        assert torch.equal(o1, o2[1024:1536]) and torch.equal(d1, d2[1024:1536]), t
    ws, wb = small.get("wind"), big.get("wind")
    np.testing.assert_array_equal(_bits(ws), _bits(wb[1024:1536]))
    assert int(small.get("ep_num").min()) >= 3
    ep = big.get("ep_num").cpu().numpy()
    np.testing.assert_array_equal(
        wb[:, :3].cpu().numpy(), wind_ref.mean_wind(31, np.arange(2048), ep, WIND["wind_speed"]))
    small.close()
    big.close()


def test_auto_reset_masked_reset_and_enabling():
    """At the step limit every env auto-resets: the new episode's mean wind is
    wind_ref.mean_wind for the new ep_num and the gust is 0; dr_reset does
    the same; reset_masked changes only masked rows; enabling wind on a handle
    mid-episode fills the mean wind of each env's current episode."""
    from drone_rl_amd import random_actions
    n, seed, off, W = 1031, 7, 1 << 33, WIND["wind_speed"]
    gids = np.arange(n, dtype=np.uint64) + np.uint64(off)
    rng = np.random.default_rng(1)
    b = _batch(n, seed=seed, env_id_offset=off, **WIND)
    np.testing.assert_array_equal(b.get("wind")[:, :3].cpu().numpy(),
                                  wind_ref.mean_wind(seed, gids, 1, W))
    b.reset()
    np.testing.assert_array_equal(b.get("wind")[:, :3].cpu().numpy(),
                                  wind_ref.mean_wind(seed, gids, 2, W))
    w0 = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.normal(0, 0.5, (n, 3))],
                        1).astype(np.float32)
    b.set("wind", w0)
    ep = rng.integers(1, 5000, n).astype(np.int32)
    b.set("ep_num", ep)
    b.set("current_step", np.full(n, 199, np.int32))
    obs, rew, done = b.step(random_actions(n, seed=2, step=0))
    assert bool(done.all())
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), ep + 1)
    w1 = b.get("wind").cpu().numpy()
    np.testing.assert_array_equal(w1[:, :3], wind_ref.mean_wind(seed, gids, ep + 1, W))
    assert not w1[:, 3:].any() and not np.signbit(w1[:, 3:]).any()
    assert (b.get("current_step").cpu().numpy() == 0).all()
    # a later wind_speed applies from the next reset; the masked reset
    b.set_wind(0.5, 3.0, 0.5, 0.1)
    np.testing.assert_array_equal(b.get("wind").cpu().numpy(), w1)
    b.set("wind", w0)
    mask = torch.from_numpy(rng.uniform(size=n) < 0.5)
    assert 0 < int(mask.sum()) < n
    b.reset_masked(mask)
    mk = mask.numpy()
    ep2 = b.get("ep_num").cpu().numpy()
    np.testing.assert_array_equal(ep2, ep + 1 + mk)
    want = np.where(mk[:, None],
                    np.concatenate([wind_ref.mean_wind(seed, gids, ep2, 3.0),
                                    np.zeros((n, 3), np.float32)], 1), w0)
    np.testing.assert_array_equal(b.get("wind").cpu().numpy(), want)
    b.close()
    # enabling mid-episode
    g = _batch(n, seed=seed, env_id_offset=off, max_steps=5)
    g.reset()
    for t in range(7):
        g.step(random_actions(n, seed=2, step=t))
    assert int(g.get("ep_num").min()) >= 3
    epg = rng.integers(1, 5000, n).astype(np.int32)
    g.set("ep_num", epg)
    step_before = g.get("current_step").cpu().numpy()
    g.set_wind(**WIND)
    wg = g.get("wind").cpu().numpy()
    np.testing.assert_array_equal(wg[:, :3], wind_ref.mean_wind(seed, gids, epg, W))
    assert not wg[:, 3:].any()
    np.testing.assert_array_equal(g.get("current_step").cpu().numpy(), step_before)
    np.testing.assert_array_equal(g.get("ep_num").cpu().numpy(), epg)
    g.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rollout_is_bitwise_k_steps(dtype):
    """dr_rollout / dr_rollout_random (the one-role kernel, mean wind and gust
    in registers) against K dr_step launches: outputs and every state field,
    `wind` included, with resets inside the launch (max_steps 16 < K)."""
    check_rollout("wind", 777, 37, dtype)
    check_rollout_random("wind", 777, 37, dtype)


def test_rollout_ignores_the_warp_specialised_override():
    """DRONERL_ROLLOUT_WS=1 forces the warp-specialised rollout forms for a
    plain gym handle; a wind handle has only the one-role kernel and must keep
    it (the override is read once per process, hence the subprocess)."""
    run_worker("rollout_parity.py", "wind", "f64", "777", "37", DRONERL_ROLLOUT_WS="1")


# ---- trainer, checkpoints, VecEnv ------------------------------------------
def test_trainer_fused_graph_and_checkpoint(tmp_path):
    """The trainer stays on the fused path (the obs is the gym's 15 floats);
    the captured rollout graph is bitwise the eager rollout; a checkpoint
    carries the wind parameters and field and resumes bit for bit."""
    def make():
        t = small_trainer(**WIND)
        assert t.use_fused and t.obs.shape[-1] == 15 and t.env.wind_enabled
        assert (t.env.drag, t.env.wind_speed, t.env.gust_sigma) == (0.5, 2.0, 0.5)
        assert t.env.gust_rate == float(np.float32(0.1))
        return t

    def at_save(sd):
        assert sd["config"]["drag"] == 0.5 and sd["config"]["gust_rate"] == 0.1

    def after(a, b):
        assert bool((a.env.get("wind")[:, 3:] != 0).any())

    graph_equals_eager_and_resumes(make, tmp_path, field="wind", field_shape=(2048, 6),
                                   resume_fields=("pos", "wind", "ep_num"), at_save=at_save,
                                   after=after)


def test_graph_key_follows_set_wind():
    """A changed parameter drops the captured rollout graph's key."""
    a = small_trainer(**WIND)
    graph_key_changes(a, lambda env: env.set_wind(0.25, 2.0, 0.5, 0.1))
    a.close()
    g = plain_trainer()
    # enabling changes the kernels a graph would hold
    graph_key_changes(g, lambda env: env.set_wind(**WIND))
    g.close()


def test_set_wind_abi():
    import ctypes

    from drone_rl_amd import DroneBatch, _lib
    b = _batch(8, **WIND)
    L = _lib.lib()
    v = [ctypes.c_float() for _ in range(4)]
    assert L.dr_get_wind(b.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == [0.5, 2.0, 0.5, float(np.float32(0.1))]
    assert L.dr_get_wind(b.handle, None, None, None, None) == _lib.DR_OK
    for bad in ((-0.1, 0, 0, 0), (float("nan"), 0, 0, 0), (float("inf"), 0, 0, 0),
                (50.5, 0, 0, 0), (0, -1.0, 0, 0), (0, float("inf"), 0, 0), (0, 0, -0.5, 0),
                (0, 0, float("nan"), 0), (0, 0, 0, -0.01), (0, 0, 0, 1.5),
                (0, 0, 0, float("nan"))):
        assert L.dr_set_wind(b.handle, *bad) == _lib.DR_ERR_INVALID, bad
    assert L.dr_get_wind(b.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == [0.5, 2.0, 0.5, float(np.float32(0.1))]   # refusals changed nothing
    assert L.dr_set_wind(b.handle, 50.0, 0.0, 0.0, 1.0) == _lib.DR_OK        # k dt = 1, beta = 1
    assert L.dr_obs_dim(b.handle) == 15
    sm = DroneBatch(8, "smooth")
    assert L.dr_set_wind(sm.handle, 0.5, 0.0, 0.0, 0.0) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_get_wind(sm.handle, None, None, None, None) == _lib.DR_ERR_UNSUPPORTED
    buf = torch.zeros(8, 6, device="cuda")
    assert L.dr_get_state(sm.handle, _lib.FIELDS["wind"], buf.data_ptr(), None) == \
        _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(ValueError):
        sm.set_wind(0.5, 0, 0, 0)
    g = _batch(8)
    for fn in (L.dr_get_state, L.dr_set_state):
        assert fn(g.handle, _lib.FIELDS["wind"], buf.data_ptr(), None) == _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(_lib.DroneRLError):
        g.get("wind")
    with pytest.raises(_lib.DroneRLError):
        g.set("wind", np.zeros((8, 6), np.float32))
    long = _batch(8, max_steps=1 << 24)
    assert L.dr_set_wind(long.handle, 0.5, 0.0, 0.0, 0.0) == _lib.DR_ERR_UNSUPPORTED
    for x in (b, sm, g, long):
        x.close()


def test_vec_env_facades():
    from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv
    v = BatchedDroneVecEnv(4, seed=3, **WIND)
    assert v.observation_space.shape == (15,)
    obs = v.reset()
    assert obs.shape == (4, 15)
    obs, rew, done, infos = v.step(np.full((4, 4), 9.81 / 4, np.float32))
    assert obs.shape == (4, 15) and not done.any()
    wind = np.stack(v.get_attr("wind"))
    assert wind.shape == (4, 6)
    np.testing.assert_array_equal(wind[:, :3], wind_ref.mean_wind(3, np.arange(4), 2, 2.0))
    assert (wind[:, 3:] != 0).all()
    # level hover from rest: the first step's velocity is the drag impulse's
    np.testing.assert_allclose(obs[:, 3:5], (0.5 * wind[:, :2].astype(np.float64)
                                             + 0.5 * wind[:, 3:5]) * 0.02, rtol=1e-6, atol=1e-9)
    v.close()
    plain = BatchedDroneVecEnv(4, seed=3)
    with pytest.raises(AttributeError):
        plain.get_attr("wind")
    plain.close()
    e = DroneVectorEnv(4, seed=3, **WIND)
    assert e.single_observation_space.shape == (15,)
    assert e.observation_space.shape == (4, 15)
    o, _ = e.reset()
    assert o.shape == (4, 15) and e.batch.wind_enabled
    e.close()
