"""The gym env's wind option (dr_set_wind) without a
GPU: the NumPy restatement tests/wind_ref.py is the gym step bit for bit at
the neutral parameters, follows the law by hand on a level hover, its gusts
have the stationary statistics the law promises, and the argument rules of
the C ABI, DroneBatch and PPOConfig run before any device work."""
import math
import os

import numpy as np
import pytest

import wind_ref
from oracle import cref
from shared import bits as _bits, gym_state as _state

NEUTRAL = dict(drag=0.0, wind_speed=0.0, gust_sigma=0.0, gust_rate=0.0)


def test_neutral_restatement_is_the_gym_step_bitwise(golden):
    """On the reference's golden step vectors (crashes, the step limit, huge
    angles, near gimbal lock): every output and state word, compared as
    bits.  The mean wind is drawn at W = 0 (zeros of either sign)."""
    g = golden("gym_step.npz")
    n = len(g["action"])
    a, b = _state(g), _state(g)
    # a velocity of -0 would come back as +0 (v + 0 * (w - v) * dt); none of
    # the golden states holds one, as no state reached from a reset does
    assert not (np.signbit(a["vel"]) & (a["vel"] == 0)).any()
    gids = np.arange(n, dtype=np.uint64) + (1 << 33)
    b["ep_num"] = np.arange(n, dtype=np.int32) % 4001 + 1
    b["wind"] = np.concatenate([wind_ref.mean_wind(5, gids, b["ep_num"], 0.0),
                                np.zeros((n, 3), np.float32)], 1)
    assert np.signbit(b["wind"][:, :3]).any() and not b["wind"].any()
    og, rg, dg = cref.gym_step(a, g["action"])
    ow, rw, dw = wind_ref.wind_step(b, g["action"], NEUTRAL, 5, gids)
    np.testing.assert_array_equal(_bits(ow), _bits(og))
    np.testing.assert_array_equal(_bits(rw), _bits(rg))
    np.testing.assert_array_equal(dw, dg)
    for k in ("pos", "vel", "euler", "omega", "step"):
        np.testing.assert_array_equal(_bits(b[k]), _bits(a[k]), err_msg=k)
    assert not b["wind"].any()


def test_constant_wind_on_a_level_hover_by_hand():
    """k = 0.5 /s, a constant wind of 2 m/s along x (written as the mean
    wind; sigma = 0 keeps the gust at 0), level at rest, hover thrust: after
    one step v_x = k w dt exactly, after two the recurrence
    v <- v + (k (w - v)) dt; the level thrust adds nothing along x."""
    k, w, dt = 0.5, 2.0, 0.02
    s = {"pos": np.array([[0.0, 0.0, 1.0]]), "vel": np.zeros((1, 3)), "euler": np.zeros((1, 3)),
         "omega": np.zeros((1, 3)), "target": np.array([[0.0, 0.0, 1.0]]),
         "step": np.zeros(1, np.int32), "ep_num": np.ones(1, np.int32),
         "wind": np.array([[w, 0, 0, 0, 0, 0]], np.float32)}
    p = dict(drag=k, wind_speed=0.0, gust_sigma=0.0, gust_rate=0.1)
    hover = np.full((1, 4), 9.81 / 4, np.float32)
    obs, rew, done = wind_ref.wind_step(s, hover, p, 3, [7])
    v1 = (k * w) * dt
    assert s["vel"][0, 0] == v1 == 0.02
    assert s["vel"][0, 1] == 0.0
    assert s["pos"][0, 0] == v1 * dt
    assert obs[0, 3] == np.float32(v1) and not done[0]
    np.testing.assert_array_equal(s["wind"], np.array([[w, 0, 0, 0, 0, 0]], np.float32))
    wind_ref.wind_step(s, hover, p, 3, [7])
    v2 = v1 + (k * (w - v1)) * dt
    assert s["vel"][0, 0] == v2
    assert s["pos"][0, 0] == v1 * dt + v2 * dt
    assert s["step"][0] == 2
    # and the velocity approaches the wind's: k dt = 0.01 per step
    for _ in range(2000):
        s["pos"][:] = [0.0, 0.0, 1.0]
        s["step"][:] = 0
        wind_ref.wind_step(s, hover, p, 3, [7])
    assert abs(s["vel"][0, 0] - w) < 1e-6


def test_gust_law_statistics():
    """beta = 0.1, sigma = 0.5, 1,024 envs, 1,100 steps, the first 100
    discarded: the sample std within 2 % of sigma, |mean| <= 0.03 sigma, the
    lag-1 autocorrelation within 0.02 of b, and every |g| within the law's
    hard bound sigma sqrt(3 (1 + b) / (1 - b)) (|xi| <= 1, so |g| <= c /
    (1 - b)) plus f32 slack.  A NumPy simulation of this law over 5 seeds gave
    std error <= 0.11 %, mean <= 0.003 sigma, autocorrelation error <=
    2.4e-4, max |g| about 4.5 sigma: the bars are >= 8 standard errors wide."""
    sigma, beta, n, steps, burn = 0.5, 0.1, 1024, 1100, 100
    b, c = wind_ref.gust_coefficients(sigma, beta)
    assert b == np.float32(0.9)
    assert c == np.float32(sigma * math.sqrt(3.0 * (1.0 - float(b) ** 2)))
    gids = np.arange(n, dtype=np.uint64) + 77
    g = np.zeros((n, 3), np.float32)
    hist = np.zeros((steps - burn, n, 3), np.float32)
    for t in range(steps):
        # one long episode: the step counter runs on (below 2^24)
        g = wind_ref.gust_update(g, wind_ref.gust_noise(9, gids, 1, t), b, c)
        assert g.dtype == np.float32
        if t >= burn:
            hist[t - burn] = g
    h = hist.astype(np.float64)
    std, mean = h.std(), h.mean()
    x, y = h[:-1].ravel(), h[1:].ravel()
    rho = np.mean((x - x.mean()) * (y - y.mean())) / (x.std() * y.std())
    bound = sigma * math.sqrt(3.0 * (1.0 + float(b)) / (1.0 - float(b)))
    print(f"gust: std {std:.5f} (sigma {sigma}), mean {mean:.2e}, lag-1 {rho:.5f} (b {float(b):.5f}), "
          f"max |g| {np.abs(h).max():.4f} (bound {bound:.4f})")
    assert abs(std - sigma) <= 0.02 * sigma
    assert abs(mean) <= 0.03 * sigma
    assert abs(rho - float(b)) <= 0.02
    assert np.abs(h).max() <= bound * (1.0 + 1e-5)
    # the three axes and the envs draw different noise
    assert len(np.unique(hist[-1])) > 3 * n - 8


def test_mean_wind_is_a_function_of_key_env_and_episode():
    gids = np.arange(4096, dtype=np.uint64) + (1 << 40)
    m = wind_ref.mean_wind(11, gids, 3, 2.0)
    assert m.dtype == np.float32 and m.shape == (4096, 3)
    assert np.abs(m).max() <= 2.0 and np.abs(m).max() > 1.99
    assert abs(float(m.mean())) < 0.05 and abs(float(m.std()) - 2.0 / math.sqrt(3.0)) < 0.03
    np.testing.assert_array_equal(m[100:200], wind_ref.mean_wind(11, gids[100:200], 3, 2.0))
    assert (wind_ref.mean_wind(11, gids, 4, 2.0) != m).all(axis=1).mean() > 0.99
    assert (wind_ref.mean_wind(12, gids, 3, 2.0) != m).all(axis=1).mean() > 0.99
    # the reset stream's block 2: one Philox call by hand for one env
    r = cref.philox([3, int(gids[5]) & 0xffffffff, int(gids[5]) >> 32, 0x52000002], [11, 0])
    want = np.float32(2.0) * (2.0 * (r[:3].astype(np.float64) / 2.0 ** 32) - 1.0).astype(np.float32)
    np.testing.assert_array_equal(m[5], want)


# ---- argument rules (no device work) ---------------------------------------
def test_ids_tables_and_header():
    from drone_rl_amd import _lib
    assert _lib.FIELDS["wind"] == 13 and _lib.ABI_VERSION == 16
    assert "dr_set_wind" in _lib.SIGNATURES and "dr_get_wind" in _lib.SIGNATURES
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dronerl.h")).read()
    assert "int dr_set_wind(dr_handle *h, float drag, float wind_speed, float gust_sigma," in hdr
    assert "int dr_get_wind(const dr_handle *h, float *drag, float *wind_speed" in hdr
    assert "DR_FIELD_WIND = 13" in hdr
    assert "#define DR_ABI_VERSION 16" in hdr
    common = open(os.path.join(os.path.dirname(__file__), "..", "drone_rl_amd", "csrc",
                               "common.h")).read()
    assert "TAG_GUST = 0x47000000u" in common and wind_ref.TAG_GUST == 0x47000000


def test_null_handle_is_refused_before_any_device_call():
    import ctypes

    from drone_rl_amd import _lib
    L = _lib.lib()
    assert L.dr_set_wind(None, 0.5, 2.0, 0.5, 0.1) == _lib.DR_ERR_INVALID
    assert "dr_set_wind: null handle" in _lib.last_error()
    x = ctypes.c_float()
    assert L.dr_get_wind(None, ctypes.byref(x), None, None, None) == _lib.DR_ERR_INVALID
    buf = (ctypes.c_float * 6)()
    assert L.dr_get_state(None, _lib.FIELDS["wind"], buf, None) == _lib.DR_ERR_INVALID


BAD = [dict(drag=-0.1), dict(drag=float("nan")), dict(drag=float("inf")), dict(drag=50.5),
       dict(drag=1e39), dict(wind_speed=-1.0), dict(wind_speed=float("nan")),
       dict(wind_speed=float("inf")), dict(gust_sigma=-0.5), dict(gust_sigma=float("nan")),
       dict(gust_sigma=float("inf")), dict(gust_rate=-0.01), dict(gust_rate=1.5),
       dict(gust_rate=float("nan"))]


@pytest.mark.parametrize("bad", BAD, ids=lambda d: "-".join(f"{k}={v}" for k, v in d.items()))
def test_bad_values_raise_without_a_device(bad):
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import check_wind
    from drone_rl_amd.ppo import PPOConfig
    with pytest.raises(ValueError):
        check_wind("gym", **bad)
    with pytest.raises(ValueError):
        DroneBatch(4, "gym", **bad)
    with pytest.raises(ValueError):
        PPOConfig(**bad)


def test_variant_rules_need_no_device():
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import check_wind
    from drone_rl_amd.ppo import PPOConfig
    assert check_wind("gym", 0.5, 2, 0.5, 0.1) == (0.5, 2.0, 0.5, float(np.float32(0.1)))
    assert check_wind("gym", 50.0, 0, 0, 1.0)[0] == 50.0        # k dt = 1 exactly
    cfg = PPOConfig(drag=0.5, wind_speed=2.0, gust_sigma=0.5, gust_rate=0.1)
    assert (cfg.drag, cfg.wind_speed, cfg.gust_sigma, cfg.gust_rate) == (0.5, 2.0, 0.5, 0.1)
    for variant in ("vectorized", "moving", "smooth", "tag", "rk4"):
        assert check_wind(variant) == (0.0, 0.0, 0.0, 0.0)      # neutral is fine anywhere
        for kw in (dict(drag=0.5), dict(wind_speed=1.0), dict(gust_sigma=0.5),
                   dict(gust_rate=0.1)):
            with pytest.raises(ValueError, match="variant='gym'"):
                check_wind(variant, **kw)
            with pytest.raises(ValueError):
                DroneBatch(4, variant, **kw)
            with pytest.raises(ValueError):
                PPOConfig(variant=variant, num_envs=4, **kw)
    with pytest.raises(ValueError, match="2\\^24"):
        check_wind("gym", drag=0.5, max_steps=1 << 24)
    with pytest.raises(ValueError, match="2\\^24"):
        DroneBatch(4, "gym", drag=0.5, max_steps=1 << 24)
    check_wind("gym", drag=0.5, max_steps=(1 << 24) - 1)
