"""The "smooth" variant's step law without a GPU: the
NumPy restatement tests/smooth_ref.py is pinned to the oracle's gym step (and
through it to the reference's golden vectors) at the neutral parameters and
to hand-computed values at alpha = 0.25, rate_penalty = 0.02; the argument
checks of the C ABI, DroneBatch and PPOConfig that run before any device
work."""
import numpy as np
import pytest

from oracle import cref
from smooth_ref import HOVER, smooth_step

VEC = ("pos", "vel", "euler", "omega", "target")


def _state(g, idx=slice(None)):
    # copies: the oracle steps its state in place
    s = {k: np.array(g[k][idx], np.float64, order="C") for k in VEC}
    s["step"] = np.array(g["step"][idx], np.int32)
    return s


def test_neutral_restatement_is_the_gym_step(golden):
    """alpha = 1, rate_penalty = 0: b = 0 and f' = a, so obs[:, :15], reward,
    done and the state after the step are the oracle's gym step bitwise, and
    obs[:, 15:] is the command."""
    g = golden("gym_step.npz")
    a = np.ascontiguousarray(g["action"], np.float32)
    n = len(a)
    ref = _state(g)
    ro, rr, rd = cref.gym_step(ref, a)
    s = _state(g)
    s["motor"] = np.random.default_rng(0).uniform(0, 7.36, (n, 4)).astype(np.float32)
    obs, rew, done = smooth_step(s, a, 1.0, 0.0)
    assert obs.shape == (n, 19) and obs.dtype == np.float32 and rew.dtype == np.float32
    np.testing.assert_array_equal(obs[:, :15], ro)
    np.testing.assert_array_equal(rew, rr.astype(np.float32))
    np.testing.assert_array_equal(done, rd)
    fin = np.isfinite(a).all(1)
    assert fin.sum() > n // 2
    np.testing.assert_array_equal(obs[fin, 15:], a[fin])
    np.testing.assert_array_equal(s["motor"], obs[:, 15:])
    for k in VEC[:4] + ("step",):
        np.testing.assert_array_equal(s[k], ref[k])


def test_restatement_hand_computed():
    """Two envs at alpha = 0.25, rate_penalty = 0.02, every value exactly
    representable: env 0 force 2 N on each motor, command (4, 0, 2, 6):
    d = (2, -2, 0, 4), s = 24, f' = 0.75 * 2 + 0.25 * a = (2.5, 1.5, 2, 3);
    env 1 force = command = 1: s = 0, f' = 1."""
    def state():
        s = {"pos": np.array([[0.1, -0.2, 1.0], [0.0, 0.0, 1.0]]),
             "vel": np.zeros((2, 3)), "euler": np.array([[0.05, -0.02, 0.3], [0.0, 0.0, 0.0]]),
             "omega": np.zeros((2, 3)), "target": np.array([[0.0, 0.0, 1.0], [0.0, 0.0, 1.0]]),
             "step": np.array([3, 7], np.int32)}
        return s
    s = state()
    s["motor"] = np.array([[2, 2, 2, 2], [1, 1, 1, 1]], np.float32)
    cmd = np.array([[4, 0, 2, 6], [1, 1, 1, 1]], np.float32)
    obs, rew, done = smooth_step(s, cmd, 0.25, 0.02)
    want_f = np.array([[2.5, 1.5, 2.0, 3.0], [1, 1, 1, 1]], np.float32)
    np.testing.assert_array_equal(obs[:, 15:], want_f)
    np.testing.assert_array_equal(s["motor"], want_f)
    ref = state()
    ro, rr, rd = cref.gym_step(ref, want_f)
    np.testing.assert_array_equal(obs[:, :15], ro)
    np.testing.assert_array_equal(done, rd)
    pen = np.float32(0.02) * np.float32(24.0)
    assert rew[0] == np.float32(rr[0]) - pen and abs(float(pen) - 0.48) < 1e-7
    assert rew[1] == np.float32(rr[1])
    np.testing.assert_array_equal(s["step"], [4, 8])
    assert float(HOVER) == float(np.float32(2.4525))


def test_set_smoothing_validates_without_gpu():
    import ctypes

    from drone_rl_amd import _lib
    L = _lib.lib()
    assert L.dr_set_smoothing(None, 0.5, 0.01) == _lib.DR_ERR_INVALID
    assert "null handle" in _lib.last_error()
    a, lam = ctypes.c_float(), ctypes.c_float()
    assert L.dr_get_smoothing(None, ctypes.byref(a), ctypes.byref(lam)) == _lib.DR_ERR_INVALID
    assert _lib.DR_VARIANT_SMOOTH == 3 and _lib.FIELDS["motor"] == 11


@pytest.mark.parametrize("kw", [dict(motor_alpha=0.0), dict(motor_alpha=1.5),
                                dict(motor_alpha=float("nan")), dict(rate_penalty=-0.1),
                                dict(rate_penalty=float("inf"))])
def test_argument_checks_need_no_device(kw):
    """Out-of-range values are refused for the smooth variant, and any
    non-neutral value on another variant, before a device is touched."""
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.ppo import PPOConfig
    with pytest.raises(ValueError):
        DroneBatch(4, "smooth", **kw)
    with pytest.raises(ValueError):
        PPOConfig(variant="smooth", **kw)


def test_smoothing_needs_the_smooth_variant():
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import OBS_DIM, RESET_UNIFORMS
    from drone_rl_amd.ppo import PPOConfig
    from drone_rl_amd.ppo_kernels import LINEAR_TANH_K
    for variant in ("gym", "moving", "vectorized"):
        with pytest.raises(ValueError):
            DroneBatch(4, variant, motor_alpha=0.5)
        with pytest.raises(ValueError):
            DroneBatch(4, variant, rate_penalty=0.01)
    with pytest.raises(ValueError):
        PPOConfig(variant="gym", motor_alpha=0.5)
    with pytest.raises(ValueError):
        PPOConfig(variant="moving", rate_penalty=0.01)
    c = PPOConfig(variant="smooth", motor_alpha=0.5, rate_penalty=0.01)
    assert (c.motor_alpha, c.rate_penalty) == (0.5, 0.01)
    assert PPOConfig().motor_alpha == 1.0 and PPOConfig().rate_penalty == 0.0
    assert OBS_DIM["smooth"] == 19 and RESET_UNIFORMS["smooth"] == 5
    assert 19 in LINEAR_TANH_K
