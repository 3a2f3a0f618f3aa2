"""The gym env's airframe option on the GPU (DESIGN.md section 19;
dr_set_airframe): a per-episode mass scale, inertia scale and four motor gains
inside the gym step.

The option is this build's specification (the reference has none).  It is
pinned (a) to the gym variant, which it reproduces bit for bit at the neutral
airframe, and through it to the reference's golden vectors; (b) to the NumPy
restatement tests/airframe_ref.py, the oracle's batched gym step with the
option's three changes, on random states.  Bars as for the gym env: done exact
(f64), obs within 1e-5 * max(|ref|, 1), reward atol 2e-5; the airframe is
exact f32 and compared bitwise.  Then every layer above the step kernel:
resets, dr_rollout, the trainer with checkpoints, and the VecEnv facades."""
import numpy as np
import pytest
import torch

import airframe_ref
from rollout_parity import check_rollout, check_rollout_random
from shared import f32_bits as _bits, gym_batch as _batch
from subproc import run_worker
from trainer_checks import (graph_equals_eager_and_resumes, graph_key_changes, plain_trainer,
                            small_trainer)

pytestmark = pytest.mark.gpu
VEC = ("pos", "vel", "euler", "omega", "target")
AIRFRAME = dict(mass_spread=0.3, inertia_spread=0.3, motor_spread=0.1)
SPREADS = (0.3, 0.3, 0.1)
F = lambda x: float(np.float32(x))   # noqa: E731


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_neutral_is_the_gym_env(dtype):
    """A gym batch, a batch after set_airframe(0, 0, 0) (which enables
    nothing) and a batch whose airframes were enabled, set back to all zeros
    and reset (the airframe kernels on m = s = g = 1): obs, reward, done,
    terminal obs, ep_num and the five vector fields equal bitwise over 210
    steps (every env passes the 200-step limit; many crash earlier)."""
    from drone_rl_amd import random_actions
    n = 1031
    g = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True)
    z = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True)
    z.set_airframe(0, 0, 0)
    w = _batch(n, dtype=dtype, seed=11, keep_terminal_obs=True, **AIRFRAME)
    assert bool((w.get("airframe") != 1).any())
    w.set_airframe(0, 0, 0)
    assert not z.airframe_enabled and w.airframe_enabled
    with pytest.raises(Exception):
        z.get("airframe")
    assert (w.mass_spread, w.inertia_spread, w.motor_spread) == (0.0, 0.0, 0.0)
    og = g.reset()
    for x in (z, w):
        assert torch.equal(x.reset(), og)
    assert bool((w.get("airframe") == 1).all())     # redrawn at zero spreads: ones
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
    assert bool((w.get("airframe") == 1).all())
    for x in (g, z, w):
        x.close()


def test_step_law_vs_restatement():
    """30 steps from random tumbling states with random airframes written
    through set("airframe") (m, s in [0.5, 1.5), g in [0.8, 1.2)), no
    auto-reset; the GPU state is re-synced to the restatement's after every
    step (the dynamics are chaotic, as in test_moving_gpu).  The airframe is
    never re-synced: no step writes it."""
    from test_moving_gpu import _random_state

    from drone_rl_amd import random_actions
    n, seed, off = 4099, 21, 3
    rng = np.random.default_rng(0)
    s = _random_state(n, rng, eps=0.0)
    del s["motion"]
    s["airframe"] = np.concatenate([rng.uniform(0.5, 1.5, (n, 2)), rng.uniform(0.8, 1.2, (n, 4))],
                                   1).astype(np.float32)
    b = _batch(n, dtype=torch.float64, auto_reset=False, seed=seed, env_id_offset=off, **AIRFRAME)
    plain = _batch(n, dtype=torch.float64, auto_reset=False, seed=seed, env_id_offset=off)
    for x in (b, plain):
        for k in VEC:
            x.set(k, s[k])
        x.set("current_step", s["step"])
    b.set("airframe", s["airframe"])
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(), s["airframe"])
    ids = torch.tensor([5, 4098, 0], dtype=torch.int32, device="cuda")
    np.testing.assert_array_equal(b.gather("airframe", ids).cpu().numpy(),
                                  s["airframe"][[5, 4098, 0]])
    a = random_actions(n, seed=5, step=0)
    plain.step(a)
    v_gym = plain.get("vel").cpu().numpy()
    plain.close()
    worst_obs = worst_rew = 0.0
    for t in range(30):
        a = random_actions(n, seed=5, step=t)
        obs, rew, done = b.step(a)
        ro, rr, rd = airframe_ref.airframe_step(s, a.cpu().numpy())
        if t == 0:
            # the option was live: a plain gym step from the same state differs
            assert np.abs(s["vel"] - v_gym).max() > 0.01
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), rd)
        err = np.abs(obs.astype(np.float64) - ro) / np.maximum(np.abs(ro.astype(np.float64)), 1.0)
        worst_obs = max(worst_obs, float(err.max()))
        worst_rew = max(worst_rew, float(np.abs(rew - rr).max()))
        assert err.max() <= 1e-5, (t, err.max())
        np.testing.assert_allclose(rew, rr, rtol=0, atol=2e-5)
        np.testing.assert_array_equal(_bits(b.get("airframe")), s["airframe"].view(np.uint32))
        for k in VEC[:4]:
            b.set(k, s[k])
    print(f"airframe step law: worst obs error {worst_obs:.3e}, "
          f"worst reward error {worst_rew:.3e}")
    np.testing.assert_array_equal(b.get("current_step").cpu().numpy(), s["step"])
    b.close()


def test_draws_belong_to_the_env_not_the_batch():
    """A batch of 512 at env_id_offset 1024 holds, after 20 steps with resets
    (max_steps 8), the airframes of rows 1024..1535 of a 2,048-env batch with
    the same seed: the draw is keyed by the global env id."""
    from drone_rl_amd import random_actions
    small = _batch(512, seed=31, env_id_offset=1024, max_steps=8, **AIRFRAME)
    big = _batch(2048, seed=31, max_steps=8, **AIRFRAME)
    os_, ob = small.reset(), big.reset()
    assert torch.equal(os_, ob[1024:1536])
    for t in range(20):
        ab = random_actions(2048, seed=4, step=t)
        a_s = random_actions(512, seed=4, step=t, env_id_offset=1024)
        assert torch.equal(a_s, ab[1024:1536])
        o1, r1, d1 = small.step(a_s)
        o2, r2, d2 = big.step(ab)
        assert torch.equal(o1, o2[1024:1536]) and torch.equal(d1, d2[1024:1536]), t
    ws, wb = small.get("airframe"), big.get("airframe")
    np.testing.assert_array_equal(_bits(ws), _bits(wb[1024:1536]))
    assert int(small.get("ep_num").min()) >= 3
    ep = big.get("ep_num").cpu().numpy()
    np.testing.assert_array_equal(_bits(wb),
                                  airframe_ref.airframe(31, np.arange(2048), ep,
                                                        SPREADS).view(np.uint32))
    small.close()
    big.close()


def test_auto_reset_masked_reset_enabling_and_late_spreads():
    """At the step limit every env auto-resets: the new episode's airframe is
    airframe_ref.airframe for the new ep_num; dr_reset does the same;
    reset_masked changes only masked rows; changed spreads apply from the next
    reset only; enabling the option mid-episode fills the airframe of each
    env's current episode."""
    from drone_rl_amd import random_actions
    n, seed, off = 1031, 7, 1 << 33
    gids = np.arange(n, dtype=np.uint64) + np.uint64(off)
    rng = np.random.default_rng(1)
    b = _batch(n, seed=seed, env_id_offset=off, **AIRFRAME)
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(),
                                  airframe_ref.airframe(seed, gids, 1, SPREADS))
    b.reset()
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(),
                                  airframe_ref.airframe(seed, gids, 2, SPREADS))
    w0 = np.concatenate([rng.uniform(0.5, 1.5, (n, 2)), rng.uniform(0.8, 1.2, (n, 4))],
                        1).astype(np.float32)
    b.set("airframe", w0)
    ep = rng.integers(1, 5000, n).astype(np.int32)
    b.set("ep_num", ep)
    b.set("current_step", np.full(n, 199, np.int32))
    obs, rew, done = b.step(random_actions(n, seed=2, step=0))
    assert bool(done.all())
    np.testing.assert_array_equal(b.get("ep_num").cpu().numpy(), ep + 1)
    w1 = b.get("airframe").cpu().numpy()
    np.testing.assert_array_equal(w1, airframe_ref.airframe(seed, gids, ep + 1, SPREADS))
    assert (b.get("current_step").cpu().numpy() == 0).all()
    # a step without a reset leaves the field as written
    b.set("airframe", w0)
    b.step(random_actions(n, seed=2, step=1))
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(), w0)
    # later spreads apply from the next reset; the masked reset
    late = (0.5, 0.0, 0.2)
    b.set_airframe(*late)
    assert (b.mass_spread, b.inertia_spread, b.motor_spread) == (0.5, 0.0, F(0.2))
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(), w0)
    mask = torch.from_numpy(rng.uniform(size=n) < 0.5)
    assert 0 < int(mask.sum()) < n
    b.reset_masked(mask)
    mk = mask.numpy()
    ep2 = b.get("ep_num").cpu().numpy()
    np.testing.assert_array_equal(ep2, ep + 1 + mk)
    drawn = airframe_ref.airframe(seed, gids, ep2, late)
    assert (drawn[:, 1] == 1).all() and (drawn[:, 0] != 1).mean() > 0.99
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(),
                                  np.where(mk[:, None], drawn, w0))
    # ... and reach the in-kernel auto-reset
    b.set("current_step", np.full(n, 199, np.int32))
    b.step(random_actions(n, seed=2, step=2))
    np.testing.assert_array_equal(b.get("airframe").cpu().numpy(),
                                  airframe_ref.airframe(seed, gids, ep2 + 1, late))
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
    g.set_airframe(**AIRFRAME)
    np.testing.assert_array_equal(g.get("airframe").cpu().numpy(),
                                  airframe_ref.airframe(seed, gids, epg, SPREADS))
    np.testing.assert_array_equal(g.get("current_step").cpu().numpy(), step_before)
    np.testing.assert_array_equal(g.get("ep_num").cpu().numpy(), epg)
    g.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rollout_is_bitwise_k_steps(dtype):
    """dr_rollout / dr_rollout_random (the one-role kernel, the six words and
    two reciprocals in registers) against K dr_step launches: outputs and
    every state field, `airframe` included, with resets inside the launch
    (max_steps 16 < K)."""
    check_rollout("airframe", 777, 37, dtype)
    check_rollout_random("airframe", 777, 37, dtype)


def test_rollout_ignores_the_warp_specialised_override():
    """DRONERL_ROLLOUT_WS=1 forces the warp-specialised rollout forms for a
    plain gym handle; an airframe handle has only the one-role kernel and must
    keep it (the override is read once per process, hence the subprocess)."""
    run_worker("rollout_parity.py", "airframe", "f64", "777", "37", DRONERL_ROLLOUT_WS="1")


# ---- trainer, checkpoints, VecEnv ------------------------------------------
def test_trainer_fused_graph_and_checkpoint(tmp_path):
    """The trainer stays on the fused path (the obs is the gym's 15 floats);
    the captured rollout graph is bitwise the eager rollout; a checkpoint
    carries the spreads and the field and resumes bit for bit."""
    def make():
        t = small_trainer(**AIRFRAME)
        assert t.use_fused and t.obs.shape[-1] == 15 and t.env.airframe_enabled
        assert (t.env.mass_spread, t.env.inertia_spread, t.env.motor_spread) == \
            (F(0.3), F(0.3), F(0.1))
        return t

    def at_save(sd):
        assert sd["config"]["mass_spread"] == 0.3 and sd["config"]["motor_spread"] == 0.1

    def after(a, b):
        assert bool((a.env.get("airframe") != 1).all(dim=1).any())

    graph_equals_eager_and_resumes(make, tmp_path, field="airframe", field_shape=(2048, 6),
                                   resume_fields=("pos", "airframe", "ep_num"), at_save=at_save,
                                   after=after)


def test_graph_key_follows_set_airframe():
    """A changed spread drops the captured rollout graph's key; so does
    enabling."""
    a = small_trainer(**AIRFRAME)
    graph_key_changes(a, lambda env: env.set_airframe(0.3, 0.3, 0.2))
    a.close()
    g = plain_trainer()
    # enabling changes the kernels a graph would hold
    graph_key_changes(g, lambda env: env.set_airframe(**AIRFRAME))
    g.close()


def test_set_airframe_abi():
    import ctypes

    from drone_rl_amd import DroneBatch, _lib
    b = _batch(8, **AIRFRAME)
    L = _lib.lib()
    v = [ctypes.c_float() for _ in range(3)]
    want = [F(0.3), F(0.3), F(0.1)]
    assert L.dr_get_airframe(b.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == want
    assert L.dr_get_airframe(b.handle, None, None, None) == _lib.DR_OK
    field = b.get("airframe").clone()
    for bad in (-0.1, 0.91, float("nan"), float("inf"), 1e39):
        for j in range(3):
            args = [0.2, 0.2, 0.2]
            args[j] = bad
            assert L.dr_set_airframe(b.handle, *args) == _lib.DR_ERR_INVALID, args
    assert L.dr_get_airframe(b.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == want             # refusals changed nothing
    assert torch.equal(b.get("airframe"), field)
    assert L.dr_set_airframe(b.handle, 0.9, 0.0, 0.9) == _lib.DR_OK     # the bound itself
    assert L.dr_obs_dim(b.handle) == 15
    # the other options are refused on an airframe handle
    assert L.dr_set_wind(b.handle, 0.5, 0.0, 0.0, 0.0) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_set_wind(b.handle, 0.0, 0.0, 0.0, 0.0) == _lib.DR_OK    # neutral: nothing to refuse
    assert L.dr_set_waypoints(b.handle, 0.25, 1.0) == _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(ValueError, match="not both"):
        b.set_wind(0.5, 0, 0, 0)
    with pytest.raises(ValueError, match="not both"):
        b.set_waypoints(0.25, 1.0)
    assert not b.wind_enabled and not b.waypoints_enabled
    buf = torch.zeros(8, 6, device="cuda")
    for fld in ("wind", "waypoint"):
        assert L.dr_get_state(b.handle, _lib.FIELDS[fld], buf.data_ptr(), None) == \
            _lib.DR_ERR_UNSUPPORTED
    # and the option on theirs, and on another variant
    sm = DroneBatch(8, "smooth")
    wd = _batch(8, drag=0.5)
    wp = _batch(8, reach_radius=0.25)
    for x in (sm, wd, wp):
        assert L.dr_set_airframe(x.handle, 0.3, 0.0, 0.0) == _lib.DR_ERR_UNSUPPORTED
        assert L.dr_get_state(x.handle, _lib.FIELDS["airframe"], buf.data_ptr(), None) == \
            _lib.DR_ERR_UNSUPPORTED
        with pytest.raises(ValueError):
            x.set_airframe(0.3, 0, 0)
        assert not x.airframe_enabled
    assert L.dr_get_airframe(sm.handle, None, None, None) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_get_airframe(wd.handle, *[ctypes.byref(x) for x in v]) == _lib.DR_OK
    assert [x.value for x in v] == [0.0, 0.0, 0.0]
    # invalid comes before unsupported
    assert L.dr_set_airframe(sm.handle, -1.0, 0.0, 0.0) == _lib.DR_ERR_INVALID
    g = _batch(8)
    for fn in (L.dr_get_state, L.dr_set_state):
        assert fn(g.handle, _lib.FIELDS["airframe"], buf.data_ptr(), None) == \
            _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(_lib.DroneRLError):
        g.get("airframe")
    with pytest.raises(_lib.DroneRLError):
        g.set("airframe", np.ones((8, 6), np.float32))
    assert L.dr_set_airframe(g.handle, 0.0, 0.0, 0.0) == _lib.DR_OK     # enables nothing
    assert L.dr_get_state(g.handle, _lib.FIELDS["airframe"], buf.data_ptr(), None) == \
        _lib.DR_ERR_UNSUPPORTED
    for x in (b, sm, wd, wp, g):
        x.close()


def test_vec_env_facades():
    from drone_rl_amd.env import INERTIA, MASS
    from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv
    v = BatchedDroneVecEnv(4, seed=3, **AIRFRAME)
    assert v.observation_space.shape == (15,)
    obs = v.reset()
    assert obs.shape == (4, 15)
    h = np.float32(9.81 / 4)
    obs, rew, done, infos = v.step(np.full((4, 4), h, np.float32))
    assert obs.shape == (4, 15) and not done.any()
    af = np.stack(v.get_attr("airframe"))
    assert af.shape == (4, 6) and af.dtype == np.float32
    np.testing.assert_array_equal(af, airframe_ref.airframe(3, np.arange(4), 2, SPREADS))
    mass = v.get_attr("mass")
    assert mass == [MASS * float(m) for m in af[:, 0]] and len(set(mass)) == 4
    inertia = v.get_attr("I", indices=[2])
    np.testing.assert_array_equal(inertia[0], np.array(INERTIA) * float(af[2, 1]))
    # level at rest: the first step's climb is the gained thrust over the mass
    a = af[:, 2:] * h
    T = (((a[:, 0] + a[:, 1]) + a[:, 2]) + a[:, 3]).astype(np.float64)
    np.testing.assert_allclose(obs[:, 5], (-9.81 + T / af[:, 0]) * 0.02, rtol=1e-5, atol=1e-7)
    v.close()
    plain = BatchedDroneVecEnv(4, seed=3)
    with pytest.raises(AttributeError):
        plain.get_attr("airframe")
    assert plain.get_attr("mass") == [1.0] * 4
    plain.close()
    e = DroneVectorEnv(4, seed=3, **AIRFRAME)
    assert e.single_observation_space.shape == (15,)
    assert e.observation_space.shape == (4, 15)
    o, _ = e.reset()
    assert o.shape == (4, 15) and e.batch.airframe_enabled
    assert e.get_attr("airframe").shape == (4, 6)
    np.testing.assert_array_equal(e.get_attr("mass"), MASS * e.get_attr("airframe")[:, 0])
    assert e.get_attr("I").shape == (4, 3)
    e.close()
