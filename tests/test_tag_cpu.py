"""The "tag" variant's step law without a GPU: the
NumPy restatement tests/tag_ref.py on a pair inside the tag radius and a pair
outside it with one crashing member, every expected value formed here by
scalar arithmetic; its antisymmetry on random states; and the argument
checks of the C ABI, DroneBatch and PPOConfig that run before any device
work."""
import ctypes
import math

import numpy as np
import pytest

from tag_ref import tag_step

R, C = 0.25, 0.5


def _falling_pairs():
    """Four drones at rest, level, motors off: a step is free fall, x and y
    stay, vz = -9.81 * 0.02, z += vz * 0.02 (about -3.9 mm).  Pair 0 is
    0.125 m apart at one height; pair 1's pursuer starts 1 mm above the
    ground (it crashes), its evader 5 m away and higher."""
    pos = np.array([[0.0, 0.0, 1.0], [0.125, 0.0, 1.0], [0.0, 0.0, 0.001], [3.0, 4.0, 1.0]])
    z = np.zeros((4, 3))
    return {"pos": pos, "vel": z.copy(), "euler": z.copy(), "omega": z.copy(),
            "target": np.full((4, 3), 7.0), "step": np.array([3, 3, 198, 198], np.int32)}


def test_restatement_hand_computed():
    s = _falling_pairs()
    obs, rew, done, crash = tag_step(s, np.zeros((4, 4), np.float32), R, C)
    vz = 0.0 + (-9.81 + 0.0) * 0.02
    znew = [z0 + vz * 0.02 for z0 in (1.0, 1.0, 0.001, 1.0)]
    assert znew[2] < 0 < znew[3]
    np.testing.assert_array_equal(s["pos"][:, 2], znew)
    np.testing.assert_array_equal(crash, [False, False, True, False])
    # pair 0 goes on (step 4 of 200); pair 1 ends for both: one crashed
    np.testing.assert_array_equal(done, [False, False, True, True])
    np.testing.assert_array_equal(s["step"], [4, 4, 199, 199])
    # pair 0: d = 0.125 < R, the bonus is on
    g0 = 0.01 * -0.125 + 1.0
    assert rew.dtype == np.float32
    assert rew[0] == np.float32(g0) and rew[1] == np.float32(-g0)
    assert abs(float(rew[0]) - 0.99875) < 1e-7
    # pair 1: d = sqrt(9 + 16 + dz^2) > R; the crasher alone pays c
    dz = znew[2] - znew[3]
    d1 = math.sqrt((9.0 + 16.0) + dz * dz)
    g1 = 0.01 * -d1
    assert rew[2] == np.float32(g1) - np.float32(C) and rew[3] == np.float32(-g1)
    assert 5.0 < d1 < 5.2 and rew[2] < -0.5 and 0.05 < rew[3] < 0.052
    # obs: own 12, partner - own position and velocity, the role
    assert obs.shape == (4, 19) and obs.dtype == np.float32
    np.testing.assert_array_equal(obs[:, 2], np.array(znew).astype(np.float32))
    np.testing.assert_array_equal(obs[:, 5], np.full(4, vz, np.float32))
    np.testing.assert_array_equal(obs[0, 12:18], np.array([0.125, 0, 0, 0, 0, 0], np.float32))
    np.testing.assert_array_equal(obs[1, 12:18], np.array([-0.125, 0, 0, 0, 0, 0], np.float32))
    np.testing.assert_array_equal(obs[2, 12:15], np.array([3, 4, znew[3] - znew[2]], np.float32))
    np.testing.assert_array_equal(obs[:, 18], [1, -1, 1, -1])
    # the carried target is not part of the law
    t = _falling_pairs()
    t["target"][:] = -3.0
    obs2, rew2, done2, _ = tag_step(t, np.zeros((4, 4), np.float32), R, C)
    np.testing.assert_array_equal(obs2, obs)
    np.testing.assert_array_equal(rew2, rew)
    # at c = 0 the crasher pays nothing
    u = _falling_pairs()
    _, rew3, _, _ = tag_step(u, np.zeros((4, 4), np.float32), R, 0.0)
    assert rew3[2] == np.float32(g1) and rew3[3] == -rew3[2]


def test_restatement_step_limit_ends_the_pair():
    s = _falling_pairs()
    s["step"][:] = [199, 10, 10, 10]       # only the first pursuer is at the limit
    _, _, done, crash = tag_step(s, np.zeros((4, 4), np.float32), R, C)
    np.testing.assert_array_equal(done, [True, True, True, True])
    np.testing.assert_array_equal(crash, [False, False, True, False])
    s = _falling_pairs()
    _, _, done, _ = tag_step(s, np.zeros((4, 4), np.float32), R, C, max_steps=4)
    np.testing.assert_array_equal(done, [True, True, True, True])


def test_restatement_antisymmetry():
    rng = np.random.default_rng(3)
    n = 512
    s = {"pos": rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 1.5], "vel": rng.normal(0, 0.5, (n, 3)),
         "euler": rng.normal(0, 0.2, (n, 3)), "omega": rng.normal(0, 0.5, (n, 3)),
         "target": np.zeros((n, 3)), "step": rng.integers(0, 190, n).astype(np.int32)}
    s["pos"][1::2] = s["pos"][0::2] + rng.normal(0, 0.15, (n // 2, 3))
    a = rng.uniform(0, 7.36, (n, 4)).astype(np.float32)
    obs, rew, done, _ = tag_step(s, a, R, 0.0)
    np.testing.assert_array_equal(done[0::2], done[1::2])
    np.testing.assert_array_equal(rew[1::2], -rew[0::2])
    np.testing.assert_array_equal(obs[0::2, 12:18], -obs[1::2, 12:18])
    inside = rew[0::2] > 0
    assert 0.1 < inside.mean() < 0.9


def test_create_needs_even_counts_before_any_device_call():
    from drone_rl_amd import _lib
    L = _lib.lib()
    assert _lib.DR_VARIANT_TAG == 4
    for n, off in ((3, 0), (4, 1), (1, 1)):
        cfg = _lib.dr_config(num_envs=n, variant=_lib.DR_VARIANT_TAG, state_dtype=0, rng_mode=0,
                             auto_reset=1, device=0, max_steps=0, seed=1, env_id_offset=off,
                             dt=0.02)
        h = ctypes.c_void_p()
        assert L.dr_create(ctypes.byref(cfg), ctypes.byref(h)) == _lib.DR_ERR_INVALID, (n, off)
        assert "even" in _lib.last_error() and not h.value


def test_set_tag_validates_without_gpu():
    from drone_rl_amd import _lib
    L = _lib.lib()
    assert L.dr_set_tag(None, 0.25, 0.0) == _lib.DR_ERR_INVALID
    assert "null handle" in _lib.last_error()
    r, c = ctypes.c_float(), ctypes.c_float()
    assert L.dr_get_tag(None, ctypes.byref(r), ctypes.byref(c)) == _lib.DR_ERR_INVALID
    assert "null handle" in _lib.last_error()


@pytest.mark.parametrize("kw", [dict(tag_radius=0.0), dict(tag_radius=-1.0),
                                dict(tag_radius=float("nan")), dict(tag_radius=float("inf")),
                                dict(crash_penalty=-0.1), dict(crash_penalty=float("nan")),
                                dict(crash_penalty=float("inf"))])
def test_argument_checks_need_no_device(kw):
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.ppo import PPOConfig
    with pytest.raises(ValueError):
        DroneBatch(4, "tag", **kw)
    with pytest.raises(ValueError):
        PPOConfig(variant="tag", **kw)


def test_tag_parameters_need_the_tag_variant_and_even_counts():
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import OBS_DIM, RESET_UNIFORMS
    from drone_rl_amd.ppo import PPOConfig
    from drone_rl_amd.vec_env import BatchedDroneVecEnv
    for variant in ("gym", "moving", "vectorized", "smooth"):
        with pytest.raises(ValueError):
            DroneBatch(4, variant, tag_radius=0.25)
        with pytest.raises(ValueError):
            DroneBatch(4, variant, crash_penalty=0.0)
    with pytest.raises(ValueError):
        PPOConfig(variant="gym", tag_radius=0.3)
    with pytest.raises(ValueError):
        PPOConfig(variant="smooth", crash_penalty=0.1)
    with pytest.raises(ValueError, match="even"):
        DroneBatch(5, "tag")
    with pytest.raises(ValueError, match="even"):
        DroneBatch(4, "tag", env_id_offset=3)
    with pytest.raises(ValueError, match="even"):
        PPOConfig(variant="tag", num_envs=1023)
    with pytest.raises(ValueError, match="even"):
        BatchedDroneVecEnv(3, variant="tag", seed=1)
    c = PPOConfig(variant="tag", num_envs=1024, tag_radius=0.3, crash_penalty=0.1)
    assert (c.tag_radius, c.crash_penalty) == (0.3, 0.1)
    assert PPOConfig().tag_radius is None and PPOConfig().crash_penalty is None
    assert OBS_DIM["tag"] == 19 and RESET_UNIFORMS["tag"] == 5
