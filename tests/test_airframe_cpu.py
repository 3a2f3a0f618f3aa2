"""The gym env's airframe option (dr_set_airframe)
without a GPU: the NumPy restatement tests/airframe_ref.py is the gym step bit
for bit at the neutral airframe, follows the law by hand on a level hover, its
per-episode draw is a function of (seed, env, episode, block) inside the
promised ranges, and the argument rules of the C ABI, DroneBatch and PPOConfig
run before any device work."""
import math
import os

import numpy as np
import pytest

import airframe_ref
from oracle import cref, drone_np
from shared import bits as _bits, gym_state as _state


# ---- ids and tables ---------------------------------------------------------
def test_ids_tables_and_header():
    from drone_rl_amd import _lib
    assert _lib.FIELDS["airframe"] == 15 and _lib.ABI_VERSION == 16
    assert _lib.SIGNATURES["dr_set_airframe"][1][1:] == [_lib.c_float] * 3
    assert len(_lib.SIGNATURES["dr_get_airframe"][1]) == 4
    here = os.path.dirname(__file__)
    hdr = open(os.path.join(here, "..", "include", "dronerl.h")).read()
    assert ("int dr_set_airframe(dr_handle *h, float mass_spread, float inertia_spread, "
            "float motor_spread);") in hdr
    assert ("int dr_get_airframe(const dr_handle *h, float *mass_spread, "
            "float *inertia_spread,") in hdr
    assert "DR_FIELD_AIRFRAME = 15" in hdr
    assert "#define DR_ABI_VERSION 16" in hdr
    common = open(os.path.join(here, "..", "drone_rl_amd", "csrc", "common.h")).read()
    assert "TAG_AIRFRAME = 0x46000000u" in common and airframe_ref.TAG_AIRFRAME == 0x46000000


def test_null_handle_is_refused_before_any_device_call():
    import ctypes

    from drone_rl_amd import _lib
    L = _lib.lib()
    assert L.dr_set_airframe(None, 0.3, 0.3, 0.1) == _lib.DR_ERR_INVALID
    assert "dr_set_airframe: null handle" in _lib.last_error()
    x = ctypes.c_float()
    assert L.dr_get_airframe(None, ctypes.byref(x), None, None) == _lib.DR_ERR_INVALID
    assert "dr_get_airframe: null handle" in _lib.last_error()
    buf = (ctypes.c_float * 6)()
    assert L.dr_get_state(None, _lib.FIELDS["airframe"], buf, None) == _lib.DR_ERR_INVALID
    assert L.dr_set_state(None, _lib.FIELDS["airframe"], buf, None) == _lib.DR_ERR_INVALID


# ---- argument rules (no device work) ----------------------------------------
NAMES = ("mass_spread", "inertia_spread", "motor_spread")
BAD = [{k: v} for k in NAMES for v in (-0.1, 0.91, float("nan"), float("inf"), 1e39)]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_values_raise_without_a_device(bad):
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import check_airframe
    from drone_rl_amd.ppo import PPOConfig
    with pytest.raises(ValueError):
        check_airframe("gym", **bad)
    with pytest.raises(ValueError):
        DroneBatch(4, "gym", **bad)
    with pytest.raises(ValueError):
        PPOConfig(**bad)


def test_variant_and_exclusion_rules_need_no_device():
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import check_airframe, check_waypoints, check_wind
    from drone_rl_amd.ppo import PPOConfig
    f = lambda x: float(np.float32(x))   # noqa: E731
    assert check_airframe("gym", 0.3, 0.3, 0.1) == (f(0.3), f(0.3), f(0.1))
    assert check_airframe("gym", 0.9, 0, 0.9) == (f(0.9), 0.0, f(0.9))    # the bound itself
    cfg = PPOConfig(mass_spread=0.3, inertia_spread=0.3, motor_spread=0.1)
    assert (cfg.mass_spread, cfg.inertia_spread, cfg.motor_spread) == (0.3, 0.3, 0.1)
    for variant in ("vectorized", "moving", "smooth", "tag", "rk4"):
        assert check_airframe(variant) == (0.0, 0.0, 0.0)       # neutral is fine anywhere
        for k in NAMES:
            with pytest.raises(ValueError, match="variant='gym'"):
                check_airframe(variant, **{k: 0.2})
            with pytest.raises(ValueError):
                DroneBatch(4, variant, **{k: 0.2})
            with pytest.raises(ValueError):
                PPOConfig(variant=variant, num_envs=4, **{k: 0.2})
    # one option per handle
    wind = check_wind("gym", drag=0.5)
    course = check_waypoints("gym", 0.25, 1.0)
    for k in NAMES:
        with pytest.raises(ValueError, match="not both"):
            check_airframe("gym", wind=wind, **{k: 0.2})
        with pytest.raises(ValueError, match="not both"):
            check_airframe("gym", waypoints=course, **{k: 0.2})
        with pytest.raises(ValueError, match="not both"):
            DroneBatch(4, "gym", drag=0.5, **{k: 0.2})
        with pytest.raises(ValueError, match="not both"):
            DroneBatch(4, "gym", reach_radius=0.25, **{k: 0.2})
        with pytest.raises(ValueError, match="not both"):
            PPOConfig(wind_speed=1.0, **{k: 0.2})
        with pytest.raises(ValueError, match="not both"):
            PPOConfig(reach_bonus=1.0, **{k: 0.2})
    # all-zero beside another option is accepted
    assert check_airframe("gym", wind=wind, waypoints=course) == (0.0, 0.0, 0.0)
    assert check_airframe("gym", 0.2, wind=check_wind("gym"), waypoints=None)[0] == f(0.2)
    PPOConfig(drag=0.5)
    PPOConfig(reach_radius=0.25)


# ---- the restatement --------------------------------------------------------
def test_neutral_restatement_is_the_batched_gym_step_bitwise(golden):
    """On the reference's golden step vectors (crashes, the step limit, huge
    angles, near gimbal lock) at m = s = g = 1: every output and state word
    equals drone_np.gym_step_batched's as bits; against the C oracle the gym's
    own bars hold (the NumPy port and the C oracle differ by 1 ulp in a few
    f64 state words of this file, so no bitwise claim there)."""
    g = golden("gym_step.npz")
    n = len(g["action"])
    assert n == 10000
    a, b, c = _state(g), _state(g), _state(g)
    b["airframe"] = np.ones((n, 6), np.float32)
    og, rg, dg = drone_np.gym_step_batched(a, g["action"])
    ow, rw, dw = airframe_ref.airframe_step(b, g["action"])
    np.testing.assert_array_equal(_bits(ow), _bits(og))
    np.testing.assert_array_equal(_bits(rw), _bits(rg))
    np.testing.assert_array_equal(dw, dg)
    for k in ("pos", "vel", "euler", "omega", "target", "step"):
        np.testing.assert_array_equal(_bits(b[k]), _bits(a[k]), err_msg=k)
    np.testing.assert_array_equal(b["airframe"], np.ones((n, 6), np.float32))
    oc, rc, dc = cref.gym_step(c, g["action"])
    np.testing.assert_array_equal(dw, dc)
    ok = np.isfinite(oc)
    np.testing.assert_array_equal(np.isfinite(ow), ok)
    err = np.abs(ow.astype(np.float64) - oc)[ok]
    assert (err <= 1e-5 * np.maximum(np.abs(oc[ok]), 1.0)).all()
    fin = np.isfinite(rc)
    np.testing.assert_allclose(rw[fin], rc[fin], rtol=0, atol=2e-5)


def _rest(af):
    return {"pos": np.array([[0.0, 0.0, 1.0]]), "vel": np.zeros((1, 3)),
            "euler": np.zeros((1, 3)), "omega": np.zeros((1, 3)),
            "target": np.array([[0.0, 0.0, 1.0]]), "step": np.zeros(1, np.int32),
            "airframe": np.array([af], np.float32)}


def test_heavy_weak_and_stiff_airframes_by_hand():
    """One env at rest, level, every motor at the hover command
    h = f32(9.81 / 4), dt = 0.02."""
    h = np.float32(9.81 / 4)
    hover = np.full((1, 4), h, np.float32)
    T = float(((h + h) + h) + h)
    # 25 % heavier: the thrust that held 1 kg no longer holds it
    s = _rest([1.25, 1, 1, 1, 1, 1])
    obs, rew, done = airframe_ref.airframe_step(s, hover)
    vz = (-9.81 + T * 0.8) * 0.02
    np.testing.assert_allclose(s["vel"][0, 2], vz, rtol=1e-6)
    assert s["vel"][0, 2] < -0.03 and s["pos"][0, 2] < 1.0 and not done[0]
    assert (s["vel"][0, :2] == 0).all() and (s["omega"] == 0).all()
    # motor 0 ten percent strong: a roll and a yaw torque of 0.1 h
    s = _rest([1, 1, 1.1, 1, 1, 1])
    airframe_ref.airframe_step(s, hover)
    w0 = ((0.5 / math.sqrt(2.0)) * (0.1 * float(h))) / 0.005 * 0.02
    w2 = (0.01 * 0.1 * float(h)) / 0.01 * 0.02
    np.testing.assert_allclose(s["omega"][0, 0], w0, rtol=1e-5)
    np.testing.assert_allclose(s["omega"][0, 1], -w0, rtol=1e-5)
    np.testing.assert_allclose(s["omega"][0, 2], w2, rtol=1e-5)
    assert s["vel"][0, 2] > 0            # and more thrust than weight
    # twice the inertia: half the rates, the same climb
    s2 = _rest([1, 2, 1.1, 1, 1, 1])
    airframe_ref.airframe_step(s2, hover)
    np.testing.assert_allclose(s2["omega"][0, 0], w0 / 2, rtol=1e-5)
    np.testing.assert_allclose(s2["omega"][0, 2], w2 / 2, rtol=1e-5)
    assert s2["vel"][0, 2] == s["vel"][0, 2]


def test_the_draw_is_a_function_of_seed_env_episode_and_block():
    n, sp = 4096, (0.3, 0.3, 0.1)
    gids = np.arange(n, dtype=np.uint64) + (1 << 40)
    a = airframe_ref.airframe(11, gids, 3, sp)
    assert a.dtype == np.float32 and a.shape == (n, 6)
    lo, hi = np.float32(1) - np.float32(0.3), np.float32(1) + np.float32(0.3)
    assert (a[:, :2] >= lo).all() and (a[:, :2] < hi).all()
    lo, hi = np.float32(1) - np.float32(0.1), np.float32(1) + np.float32(0.1)
    assert (a[:, 2:] >= lo).all() and (a[:, 2:] < hi).all()
    # uniform on +-0.3: std 0.173, standard error of a column mean 0.0027
    mean = a.astype(np.float64).mean(0)
    print("airframe column means", mean)
    assert (np.abs(mean - 1.0) < 0.02).all()
    np.testing.assert_array_equal(a[100:200], airframe_ref.airframe(11, gids[100:200], 3, sp))
    for other in (airframe_ref.airframe(12, gids, 3, sp),        # seed
                  airframe_ref.airframe(11, gids + np.uint64(n), 3, sp),   # env
                  airframe_ref.airframe(11, gids, 4, sp)):       # episode
        assert (other != a).any(axis=1).mean() > 0.99
        assert (other[:, :2] != a[:, :2]).any(axis=1).mean() > 0.99
        assert (other[:, 2:] != a[:, 2:]).any(axis=1).mean() > 0.99
    # the two blocks differ: (m, s) are not the first two gains' deviates
    same_sigma = airframe_ref.airframe(11, gids, 3, (0.1, 0.1, 0.1))
    assert (same_sigma[:, :2] != same_sigma[:, 2:4]).any(axis=1).mean() > 0.99
    # neutral: exactly 1.0f everywhere, and per spread
    np.testing.assert_array_equal(airframe_ref.airframe(11, gids, 3, (0, 0, 0)),
                                  np.ones((n, 6), np.float32))
    part = airframe_ref.airframe(11, gids, 3, (0.3, 0, 0))
    np.testing.assert_array_equal(part[:, 0], a[:, 0])
    np.testing.assert_array_equal(part[:, 1:], np.ones((n, 5), np.float32))
    # one Philox call by hand for one env, both blocks
    gid = int(gids[5])
    pm1 = lambda r: (2.0 * (r.astype(np.float64) / 2.0 ** 32) - 1.0).astype(np.float32)  # noqa: E731
    r0 = cref.philox([3, gid & 0xffffffff, gid >> 32, 0x46000000], [11, 0])
    r1 = cref.philox([3, gid & 0xffffffff, gid >> 32, 0x46000001], [11, 0])
    want = np.concatenate([np.float32(1) + np.float32(0.3) * pm1(r0[:2]),
                           np.float32(1) + np.float32(0.1) * pm1(r1)])
    np.testing.assert_array_equal(a[5], want)
