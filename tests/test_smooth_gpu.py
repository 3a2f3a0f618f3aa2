"""The "smooth" env variant on the GPU: the gym env
behind a first-order motor lag with an action-rate penalty.

The variant is this build's specification (the reference has none).  It is
pinned (a) to the gym variant, which it reproduces bit for bit at the neutral
parameters alpha = 1, rate_penalty = 0, and through it to the reference's
golden vectors; (b) to the NumPy restatement tests/smooth_ref.py, built
around the oracle's gym step, on random states.  Bars as for the gym and
moving envs: done exact (f64), obs within 1e-5 * max(|ref|, 1), reward atol
2e-5; the motor forces are exact f32 and compared bitwise.  Then every layer
above the step kernel: auto-reset, dr_rollout, the K = 19 first-layer PPO
kernels, the trainer with checkpoints, and the VecEnv facade."""
import numpy as np
import pytest
import torch

from rollout_parity import check_rollout, check_rollout_random
from smooth_ref import HOVER, smooth_step
from subproc import run_worker
from trainer_checks import graph_equals_eager_and_resumes, graph_key_changes, small_trainer

pytestmark = pytest.mark.gpu
VEC = ("pos", "vel", "euler", "omega", "target")
ALPHA, LAM = 0.25, 0.02


def _batch(n, variant="smooth", **kw):
    from drone_rl_amd import DroneBatch
    return DroneBatch(n, variant, **kw)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_neutral_is_the_gym_env(dtype):
    """alpha = 1, rate_penalty = 0 (the defaults): obs[:, :15], reward, done,
    terminal obs and resets equal the gym variant's bitwise over 210 steps
    (every env passes the 200-step limit; many crash earlier), and
    obs[:, 15:19] is the previous command, HOVER in rows that reset."""
    from drone_rl_amd import random_actions
    n = 1031
    g = _batch(n, "gym", dtype=dtype, seed=11, keep_terminal_obs=True)
    m = _batch(n, "smooth", dtype=dtype, seed=11, keep_terminal_obs=True)
    assert m.obs_dim == 19 and (m.motor_alpha, m.rate_penalty) == (1.0, 0.0)
    og, om = g.reset(), m.reset()
    assert om.shape == (n, 19)
    hover = torch.full((n, 4), float(HOVER), device="cuda")
    assert torch.equal(om[:, :15], og) and torch.equal(om[:, 15:], hover)
    done_count = torch.zeros(n, dtype=torch.int64, device="cuda")
    early = 0
    for t in range(210):
        a = random_actions(n, seed=3, step=t)
        og, rg, dg = g.step(a)
        om, rm, dm = m.step(a)
        assert torch.equal(om[:, :15], og), t
        assert torch.equal(rm, rg) and torch.equal(dm, dg), t
        assert torch.equal(m.term_obs[:, :15], g.term_obs), t
        assert torch.equal(om[:, 15:], torch.where(dm.bool()[:, None], hover, a)), t
        done_count += dm
        if t < 199:
            early += int(dm.sum())
    assert int(done_count.min()) >= 1 and early > n // 2
    assert torch.equal(m.get("ep_num"), g.get("ep_num"))
    assert torch.equal(m.get("motor"), om[:, 15:])
    g.close()
    m.close()


def test_step_law_vs_restatement():
    """30 steps from random tumbling states with random motor forces at
    alpha = 0.25, rate_penalty = 0.02, no auto-reset; the GPU state is
    re-synced to the restatement's after every step (the dynamics are chaotic,
    as in test_moving_gpu)."""
    from test_moving_gpu import _random_state

    from drone_rl_amd import random_actions
    n = 4099
    rng = np.random.default_rng(0)
    s = _random_state(n, rng, eps=0.0)
    del s["motion"]
    s["motor"] = rng.uniform(0, 7.36, (n, 4)).astype(np.float32)
    b = _batch(n, dtype=torch.float64, auto_reset=False, motor_alpha=ALPHA, rate_penalty=LAM)
    for k in VEC:
        b.set(k, s[k])
    b.set("current_step", s["step"])
    b.set("motor", s["motor"])
    np.testing.assert_array_equal(b.get("motor").cpu().numpy(), s["motor"])
    ids = torch.tensor([5, 4098, 0], dtype=torch.int32, device="cuda")
    np.testing.assert_array_equal(b.gather("motor", ids).cpu().numpy(), s["motor"][[5, 4098, 0]])
    for t in range(30):
        a = random_actions(n, seed=5, step=t)
        obs, rew, done = b.step(a)
        ro, rr, rd = smooth_step(s, a.cpu().numpy(), ALPHA, LAM)
        obs, rew = obs.cpu().numpy(), rew.cpu().numpy()
        np.testing.assert_array_equal(done.cpu().numpy().astype(bool), rd)
        err = np.abs(obs[:, :15].astype(np.float64) - ro[:, :15]) / \
            np.maximum(np.abs(ro[:, :15].astype(np.float64)), 1.0)
        assert err.max() <= 1e-5, (t, err.max())
        np.testing.assert_allclose(rew, rr, rtol=0, atol=2e-5)
        np.testing.assert_array_equal(obs[:, 15:], ro[:, 15:])
        np.testing.assert_array_equal(b.get("motor").cpu().numpy(), s["motor"])
        for k in VEC[:4]:
            b.set(k, s[k])
    # the penalty was live: it is most of the reward under a random policy
    assert float(np.mean(rr)) < -0.1
    np.testing.assert_array_equal(b.get("current_step").cpu().numpy(), s["step"])
    b.close()


def test_auto_reset_and_masked_reset():
    """At the step limit every env auto-resets: the terminal obs carries that
    step's lagged forces, the reset obs and the stored forces are HOVER;
    reset_masked resets the forces only where the mask is set."""
    from drone_rl_amd import random_actions
    n = 1031
    rng = np.random.default_rng(1)
    b = _batch(n, seed=7, keep_terminal_obs=True, motor_alpha=ALPHA, rate_penalty=LAM)
    b.reset()
    f0 = rng.uniform(0, 7.36, (n, 4)).astype(np.float32)
    b.set("motor", f0)
    b.set("current_step", np.full(n, 199, np.int32))
    a = random_actions(n, seed=2, step=0)
    obs, rew, done = b.step(a)
    assert bool(done.all())
    a_np = a.cpu().numpy()
    f1 = (np.float32(1.0) - np.float32(ALPHA)) * f0 + np.float32(ALPHA) * a_np
    np.testing.assert_array_equal(b.term_obs[:, 15:].cpu().numpy(), f1)
    hover = np.full((n, 4), HOVER, np.float32)
    np.testing.assert_array_equal(obs[:, 15:].cpu().numpy(), hover)
    np.testing.assert_array_equal(b.get("motor").cpu().numpy(), hover)
    assert (b.get("current_step").cpu().numpy() == 0).all()
    # masked reset
    f2 = rng.uniform(0, 7.36, (n, 4)).astype(np.float32)
    b.set("motor", f2)
    mask = torch.from_numpy(rng.uniform(size=n) < 0.5)
    assert 0 < int(mask.sum()) < n
    obs = b.reset_masked(mask)
    want = np.where(mask.numpy()[:, None], hover, f2)
    np.testing.assert_array_equal(b.get("motor").cpu().numpy(), want)
    np.testing.assert_array_equal(obs[:, 15:].cpu().numpy(), want)
    b.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_rollout_is_bitwise_k_steps(dtype):
    """dr_rollout / dr_rollout_random (the one-role kernel, the lag state in
    registers) against K dr_step launches: outputs and every state field,
    `motor` included, with resets inside the launch (max_steps 16 < K)."""
    check_rollout("smooth", 777, 37, dtype)
    check_rollout_random("smooth", 777, 37, dtype)


def test_rollout_ignores_the_warp_specialised_override():
    """DRONERL_ROLLOUT_WS=1 forces the warp-specialised rollout forms for the
    other variants; this one has only the one-role kernel and must keep it
    (the override is read once per process, hence the subprocess)."""
    run_worker("rollout_parity.py", "smooth", "f64", "777", "37", DRONERL_ROLLOUT_WS="1")


# ---- the first-layer PPO kernels at the 19-d observation -------------------
K19 = [(19, 64, 77), (19, 256, 5001)]


@pytest.mark.parametrize("k,n,m", K19)
def test_linear_tanh_k19_matches_torch(k, n, m):
    from drone_rl_amd import ppo_kernels as K
    x = torch.randn(m, k, device="cuda")
    w = torch.randn(n, k, device="cuda") * 0.4
    b = torch.randn(n, device="cuda") * 0.1
    h = torch.empty(m, n, device="cuda")
    K.linear_tanh(x, w, b, h)
    ref = torch.tanh(torch.addmm(b, x, w.t()))
    assert (h - ref).abs().max().item() <= 2e-6


@pytest.mark.parametrize("k,n,m", K19)
def test_first_layer_backward_k19_matches_f64(k, n, m):
    """The check and bound of test_first_layer_backward_matches_torch."""
    import test_ppo_kernels_gpu as PK
    PK.test_first_layer_backward_matches_torch(k, n, m)


@pytest.mark.parametrize("k,n,m", K19)
def test_paired_first_layer_kernels_k19_equal_single(k, n, m):
    """Bitwise, with and without rows= (test_paired_first_layer_kernels_equal_single)."""
    import test_ppo_kernels_gpu as PK
    PK.test_paired_first_layer_kernels_equal_single(k, n, m)


def test_gather_records_at_width_19():
    import test_ppo_kernels_gpu as PK
    PK.test_gather_records_is_gather_minibatch(1025, 19)


def test_fused_step_matches_unfused_path_at_width_19():
    """test_fused_step_matches_unfused_path's comparison and bound at obs
    width 19, arch (64, 64), m = 1000."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep, fusable
    arch, m, od = (64, 64), 1000, 19
    torch.manual_seed(1)
    pol = ActorCritic(od, 4, arch, device="cuda", seed=4)
    assert fusable(pol)
    with torch.no_grad():
        pol.flat.mul_(3.0)
    obs = torch.randn(m, od, device="cuda")
    fs = FusedTrainStep(pol, m)
    with torch.no_grad():
        mean, value, cache = fs.forward(obs)
        d = torch.distributions.Normal(mean, pol.log_std.exp())
        act = d.sample()
        aux = torch.stack([d.log_prob(act).sum(1) + 0.1 * torch.randn(m, device="cuda"),
                           torch.randn(m, device="cuda"), torch.randn(m, device="cuda")], 1)
    L = K.PPOLoss(m, "cuda", 0.2, 0.01, 0.5, True)
    g_mean, g_ls, g_v, st = L(mean, pol.log_std.detach(), value, act, aux=aux)
    ref = fs.backward(obs, cache, g_mean, g_v, g_ls).clone()
    st_ref = st.clone()
    head = K.HeadLossBackward(m, arch[-1], "cuda", 0.2, 0.01, 0.5, True)
    grad, st2 = fs.step(obs, act, aux, head)
    grad = grad.clone()
    for name, _, _ in pol.layout:
        lo, hi, _ = pol.offsets[name]
        scale = ref[lo:hi].abs().max().item() + 1e-12
        assert (grad[lo:hi] - ref[lo:hi]).abs().max().item() <= 2e-4 * scale + 1e-7, name
    assert torch.allclose(st2, st_ref, rtol=1e-4, atol=1e-6)
    grad2, _ = fs.step(obs, act, aux, head)
    assert torch.equal(grad, grad2)


# ---- trainer, checkpoints, VecEnv ------------------------------------------
def _trainer():
    return small_trainer(variant="smooth", motor_alpha=0.5, rate_penalty=0.01)


def test_trainer_fused_graph_and_checkpoint(tmp_path):
    """The trainer stays on the fused path at obs width 19; the captured
    rollout graph is bitwise the eager rollout (rollout_graph = False, what
    DRONERL_ROLLOUT_GRAPH=0 sets); a checkpoint carries the motor forces and
    resumes bit for bit."""
    def make():
        t = _trainer()
        assert t.use_fused and t.obs.shape[-1] == 19
        assert (t.env.motor_alpha, t.env.rate_penalty) == (0.5, 0.01)
        assert t._graph_key("rollout")[-2:] == (0.5, 0.01)
        return t

    graph_equals_eager_and_resumes(make, tmp_path, field="motor", field_shape=(2048, 4),
                                   resume_fields=("pos", "motor", "ep_num"))


def test_graph_key_follows_set_smoothing():
    """A changed parameter drops the captured rollout graph's key."""
    a = _trainer()
    graph_key_changes(a, lambda env: env.set_smoothing(0.25, 0.01))
    a.close()


def test_set_smoothing_abi():
    import ctypes

    from drone_rl_amd import _lib
    b = _batch(8, motor_alpha=0.5, rate_penalty=0.01)
    L = _lib.lib()
    al, lam = ctypes.c_float(), ctypes.c_float()
    assert L.dr_get_smoothing(b.handle, ctypes.byref(al), ctypes.byref(lam)) == _lib.DR_OK
    assert (al.value, lam.value) == (0.5, float(np.float32(0.01)))
    for bad in ((0.0, 0.0), (1.5, 0.0), (float("nan"), 0.0), (0.5, -1.0), (0.5, float("inf"))):
        assert L.dr_set_smoothing(b.handle, *bad) == _lib.DR_ERR_INVALID, bad
    assert L.dr_obs_dim(b.handle) == 19
    g = _batch(8, "gym")
    assert L.dr_set_smoothing(g.handle, 0.5, 0.0) == _lib.DR_ERR_UNSUPPORTED
    with pytest.raises(_lib.DroneRLError):
        g.get("motor")
    with pytest.raises(ValueError):
        g.set_smoothing(0.5, 0.0)
    b.close()
    g.close()


def test_vec_env_facade():
    from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv
    v = BatchedDroneVecEnv(4, variant="smooth", seed=3, motor_alpha=0.5, rate_penalty=0.01)
    assert v.observation_space.shape == (19,)
    obs = v.reset()
    assert obs.shape == (4, 19) and (obs[:, 15:] == HOVER).all()
    act = np.full((4, 4), 3.0, np.float32)
    obs, rew, done, infos = v.step(act)
    want = np.float32(0.5) * HOVER + np.float32(0.5) * np.float32(3.0)
    assert obs.shape == (4, 19) and (obs[:, 15:] == want).all() and not done.any()
    motor = v.get_attr("motor")
    assert len(motor) == 4 and (np.stack(motor) == want).all()
    v.close()
    e = DroneVectorEnv(4, seed=3, variant="smooth", motor_alpha=0.5, rate_penalty=0.01)
    assert e.single_observation_space.shape == (19,)
    assert e.observation_space.shape == (4, 19)
    o, _ = e.reset()
    assert o.shape == (4, 19)
    e.close()
