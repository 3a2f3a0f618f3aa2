"""The sensor model without a GPU: properties of the
NumPy restatement, its fault modes on the device comparison's own inputs, and
every host-side check of the new ABI, config fields and command-line flags."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from sensor_ref import (CASES, DONE_PATTERNS, STEPS, SensorRef, bits, case_inputs, done_pattern,
                        make_ref)

SENSOR_FUNCS = ("dr_sensor_reset", "dr_sensor_step")


# ------------------------------------------------------------- restatement
def _coded_run(fault=None):
    """Observations that carry (ep, s) of the test's own episode count: the
    delivered value says which episode and step it came from."""
    n, od, steps = 64, 5, 60
    rng = np.random.default_rng(1)
    ref = SensorRef(n, od, np.zeros(od), np.zeros(od), np.full(od, -1), delay=(0, 4), seed=3,
                    fault=fault)
    ep, s = np.zeros(n, np.int64), np.zeros(n, np.int64)
    code = lambda: np.repeat((1000.0 * ep + s)[:, None], od, 1).astype(np.float32)
    out = ref.reset(code())
    assert np.array_equal(out, code())
    bad = 0
    for _ in range(steps):
        done = rng.random(n) < 0.1
        ep, s = np.where(done, ep + 1, ep), np.where(done, 0, s + 1)
        out = ref.step(code(), done)
        want = 1000.0 * ep + np.maximum(s - ref.d, 0)
        bad += int((out != want[:, None].astype(np.float32)).sum())
    assert set(ref.d) == {0, 1, 2, 3, 4}
    return bad


def test_delayed_rows_come_from_the_same_episode():
    assert _coded_run() == 0


def test_a_leak_shows_in_the_coded_observations():
    assert _coded_run("leak") > 0


@pytest.mark.parametrize("fault", ["leak", "mirror_plus", "stale_ep"])
def test_fault_modes_differ_on_the_device_comparisons_inputs(fault):
    """On a case of the device comparison with delays, mirrors, terminal
    rows and dones each wrong law gives other outputs than the law: the
    bitwise comparison on the device can fail."""
    inp = case_inputs(CASES[1])
    assert inp["delay"][1] > 0 and (inp["mirror"] >= 0).any() and inp["dones"].any()
    a, b = make_ref(inp), make_ref(inp, fault=fault)
    differ = not np.array_equal(a.reset(inp["obs0"]), b.reset(inp["obs0"]))
    for t in range(STEPS):
        oa, ta = a.step(inp["obs"][t], inp["dones"][t], inp["term"][t])
        ob, tb = b.step(inp["obs"][t], inp["dones"][t], inp["term"][t])
        differ |= not np.array_equal(oa, ob)
    assert differ


def test_every_done_pattern_and_setting_is_among_the_cases():
    assert {c[0] for c in CASES} == {1, 63, 257, 4099}
    assert {c[1] for c in CASES} == {12, 15, 16, 19}
    assert {c[2] for c in CASES} == {(0, 0), (3, 3), (0, 4), (15, 15)}
    assert {c[3] for c in CASES} == {c[4] for c in CASES} == {False, True}
    assert {c[5] for c in CASES} == set(DONE_PATTERNS)
    d = done_pattern("consecutive", STEPS, 4, np.random.default_rng(0))
    assert d[5:8, 0].all() and d.sum() == 6


def test_delay_draw_covers_exactly_lo_to_hi():
    n, od = 4096, 3
    ref = SensorRef(n, od, np.zeros(od), np.zeros(od), np.full(od, -1), delay=(2, 6), seed=11)
    ref.reset(np.zeros((n, od), np.float32))
    assert set(ref.d) == {2, 3, 4, 5, 6}
    ref.step(np.zeros((n, od), np.float32), np.ones(n, np.uint8))
    assert set(ref.d) == {2, 3, 4, 5, 6} and (ref.ep == 1).all()


def test_neutral_configuration_is_the_identity_bitwise():
    n, od = 33, 15
    rng = np.random.default_rng(5)
    ref = SensorRef(n, od, np.zeros(od), np.zeros(od), np.where(np.arange(od) >= 12,
                                                                np.arange(od) - 12, -1))
    x = rng.standard_normal((n, od)).astype(np.float32)
    x[0, :4] = (-0.0, 0.0, np.inf, np.nan)
    assert np.array_equal(bits(ref.reset(x)), bits(x))
    for t in range(5):
        x = rng.standard_normal((n, od)).astype(np.float32)
        x[1, 12:] = -0.0
        out, to = ref.step(x, rng.random(n) < 0.3, term_obs=-x)
        assert np.array_equal(bits(out), bits(x))


def test_env_id_offset_slices_the_draws():
    od = 15
    rng = np.random.default_rng(6)
    sigma, beta = np.full(od, 0.05, np.float32), np.full(od, 0.02, np.float32)
    mk = lambda n, off: SensorRef(n, od, sigma, beta, np.full(od, -1), delay=(0, 4), seed=9,
                                  env_id_offset=off)
    whole, part = mk(128, 0), mk(64, 64)
    x = rng.standard_normal((128, od)).astype(np.float32)
    assert np.array_equal(whole.reset(x)[64:], part.reset(x[64:]))
    for t in range(6):
        x = rng.standard_normal((128, od)).astype(np.float32)
        done = rng.random(128) < 0.2
        assert np.array_equal(whole.step(x, done)[64:], part.step(x[64:], done[64:]))
    assert np.array_equal(whole.state()[:, 64:], part.state())
    assert np.array_equal(whole.bias[64:], part.bias)


def test_noise_has_the_stated_std():
    """The noise is sigma' u with u uniform on [-1, 1): std sigma, kurtosis
    1.8, so over m independent samples the sample variance has the relative
    standard error sqrt((1.8 - 1) / m) = sqrt(0.8 / m); 5 of them are allowed.
    The roundings are far below that: sigma' and pm1 carry 2^-24 relative, and
    out - x differs from e by at most half an ulp of out (6e-8 |out| against
    e of order sigma = 0.05), about 1e-6 of the variance."""
    n, od, steps = 4096, 4, 50
    m = n * (steps + 1)
    assert m >= 2e5
    sigma = np.array([0.05, 0.02, 0.1, 0.0], np.float32)
    ref = SensorRef(n, od, sigma, np.zeros(od), np.full(od, -1), seed=2)
    rng = np.random.default_rng(8)
    err = []
    x = rng.standard_normal((n, od)).astype(np.float32)
    err.append(ref.reset(x).astype(np.float64) - x)
    for t in range(steps):
        x = rng.standard_normal((n, od)).astype(np.float32)
        err.append(ref.step(x, rng.random(n) < 0.05).astype(np.float64) - x)
    err = np.concatenate(err)
    assert err.shape == (m, od)
    tol = 5.0 * math.sqrt(0.8 / m)
    for c in range(3):
        var = float(np.mean(err[:, c] ** 2))
        rel = var / float(sigma[c]) ** 2 - 1.0
        print(f"column {c}: sample var / sigma^2 - 1 = {rel:+.3e} (allowed {tol:.3e})")
        assert abs(rel) <= tol
        assert abs(float(err[:, c].mean())) <= 5.0 * float(sigma[c]) / math.sqrt(m)
    assert not err[:, 3].any()


def test_column_table():
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.env import OBS_DIM
    assert set(K.SENSOR_COLUMNS) == set(OBS_DIM)
    noise, bias = (1, 2, 3, 4), (5, 6, 7, 8)
    for variant, od in OBS_DIM.items():
        s, b, m = K.sensor_columns(variant, noise, bias)
        assert len(s) == len(b) == len(m) == od
        assert all(-1 <= m[c] < c for c in range(od))
        assert s[:6] == [1, 1, 1, 2, 2, 2] and b[:6] == [5, 5, 5, 6, 6, 6]
    s, b, m = K.sensor_columns("gym", noise, bias)
    assert s == [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3 + [0] * 3
    assert m == [-1] * 12 + [0, 1, 2]
    s, b, m = K.sensor_columns("rk4", noise, bias)
    assert s == [1] * 3 + [2] * 3 + [3] * 4 + [4] * 3 + [0] * 3 and m[13:] == [0, 1, 2]
    s, b, m = K.sensor_columns("tag", noise, bias)
    assert s == [1] * 3 + [2] * 3 + [3] * 3 + [4] * 3 + [1] * 3 + [2] * 3 + [0]
    assert m == [-1] * 19
    for variant in ("moving", "smooth"):
        s, b, m = K.sensor_columns(variant, noise, bias)
        assert m[12:15] == [0, 1, 2] and not any(s[15:]) and not any(b[12:])
        assert m[15:] == [-1] * (OBS_DIM[variant] - 15)
    assert K.sensor_columns("vectorized", noise, bias)[2] == [-1] * 12


# -------------------------------------------------------------- validation
def test_header_declares_the_functions_and_abi_16():
    src = open(os.path.join(ROOT, "include", "dronerl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in SENSOR_FUNCS:
        assert re.search(r"\b%s\s*\(" % f, src), f
    assert re.search(r"#define\s+DR_ABI_VERSION\s+16\b", src)
    assert re.search(r"#define\s+DR_SENSOR_MAX_DIM\s+24\b", src)
    assert re.search(r"#define\s+DR_SENSOR_MAX_DELAY\s+15\b", src)
    assert re.search(r"\bdr_sensor_config\b", src)
    from drone_rl_amd import _lib
    assert set(SENSOR_FUNCS) <= set(_lib.SIGNATURES)
    assert (_lib.DR_SENSOR_MAX_DIM, _lib.DR_SENSOR_MAX_DELAY) == (24, 15)
    assert ctypes.sizeof(_lib.dr_sensor_config) == 8 + 8 + 8 + 3 * 4 * 24
    assert _lib.lib().dr_abi_version() == 16


def _host_buffers(n, d, hi):
    """Host memory standing in for device buffers: every call below must be
    refused before any HIP call, so nothing ever reads it."""
    from drone_rl_amd import _lib
    mk = lambda k, t=ctypes.c_float: ctypes.cast((t * k)(), ctypes.c_void_p)
    return _lib.lib(), dict(obs=mk(n * d), done=mk(n, ctypes.c_uint8), term=None,
                            state=mk(3 * n, ctypes.c_int32), bias=mk(n * d),
                            ring=mk((hi + 1) * n * d), out=mk(n * d), term_out=None,
                            spare=mk(n * d))


def _config(d=15, lo=0, hi=4, sigma=None, beta=None, mirror=None):
    from drone_rl_amd import _lib
    c = _lib.dr_sensor_config(delay_lo=lo, delay_hi=hi, seed=1, env_id_offset=0)
    for k in range(24):
        c.sigma[k], c.beta[k], c.mirror[k] = 0.01, 0.01, -1
    for arr, given in ((c.sigma, sigma), (c.beta, beta), (c.mirror, mirror)):
        for k, v in (given or {}).items():
            arr[k] = v
    return c


REFUSALS = [
    (dict(n=0), {}, "n must"), (dict(n=-3), {}, "n must"),
    (dict(d=0), {}, "obs_dim"), (dict(d=25), {}, "obs_dim"),
    ({}, dict(sigma={3: -0.1}), "sigma[3]"), ({}, dict(sigma={0: float("nan")}), "sigma[0]"),
    ({}, dict(sigma={14: float("inf")}), "sigma[14]"),
    ({}, dict(beta={2: -1.0}), "beta[2]"), ({}, dict(beta={5: float("inf")}), "beta[5]"),
    ({}, dict(beta={5: float("nan")}), "beta[5]"),
    ({}, dict(mirror={0: 0}), "mirror[0]"), ({}, dict(mirror={12: 12}), "mirror[12]"),
    ({}, dict(mirror={12: 13}), "mirror[12]"), ({}, dict(mirror={3: -2}), "mirror[3]"),
    ({}, dict(lo=-1), "delay"), ({}, dict(lo=3, hi=2), "delay"), ({}, dict(hi=16), "delay"),
    (dict(obs=None), {}, "obs"), (dict(out=None), {}, "obs_out"),
    (dict(state=None), {}, "state"), (dict(bias=None), {}, "bias"), (dict(ring=None), {}, "ring"),
]


@pytest.mark.parametrize("kw,ckw,word", REFUSALS)
def test_argument_checks_need_no_gpu(kw, ckw, word):
    from drone_rl_amd import _lib
    L, b = _host_buffers(8, 15, 4)
    b.update({k: v for k, v in kw.items() if k not in ("n", "d")})
    n, d = kw.get("n", 8), kw.get("d", 15)
    cfg = ctypes.byref(_config(**ckw))
    rc = L.dr_sensor_step(cfg, n, d, b["obs"], b["done"], b["term"], b["state"], b["bias"],
                          b["ring"], b["out"], b["term_out"], None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_sensor_step" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    rc = L.dr_sensor_reset(cfg, n, d, b["obs"], b["state"], b["bias"], b["ring"], b["out"], None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_sensor_reset" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()


def test_step_only_argument_checks_need_no_gpu():
    from drone_rl_amd import _lib
    L, b = _host_buffers(8, 15, 4)
    cfg = ctypes.byref(_config())
    step = lambda **kw: L.dr_sensor_step(*[cfg, 8, 15] + [dict(b, **kw)[k] for k in (
        "obs", "done", "term", "state", "bias", "ring", "out", "term_out")] + [None])
    for kw, word in ((dict(done=None), "dones"), (dict(term=b["spare"]), "terminal_out"),
                     (dict(term_out=b["spare"]), "terminal_obs")):
        assert step(**kw) == _lib.DR_ERR_INVALID
        assert word in _lib.last_error(), _lib.last_error()
    assert L.dr_sensor_step(None, 8, 15, b["obs"], b["done"], None, b["state"], b["bias"],
                            b["ring"], b["out"], None, None) == _lib.DR_ERR_INVALID
    assert "config" in _lib.last_error()


def test_config_refuses_bad_sensor_values():
    from drone_rl_amd.ppo import PPOConfig
    c = PPOConfig()
    assert (tuple(c.obs_noise), tuple(c.obs_bias), tuple(c.obs_delay)) == \
        ((0, 0, 0, 0), (0, 0, 0, 0), (0, 0))
    assert not c.sensor_on()
    for kw in (dict(obs_noise=(0.1, 0, 0)), dict(obs_noise=(0.1, 0, 0, -1e-3)),
               dict(obs_noise=(float("nan"), 0, 0, 0)), dict(obs_noise=(float("inf"), 0, 0, 0)),
               dict(obs_noise=0.1), dict(obs_bias=(0, 0, 0, 0, 0)), dict(obs_bias=(0, -1, 0, 0)),
               dict(obs_bias=(0, float("inf"), 0, 0)), dict(obs_bias=(1e39, 0, 0, 0)),
               dict(obs_delay=(0, 16)), dict(obs_delay=(3, 2)), dict(obs_delay=(-1, 2)),
               dict(obs_delay=(0.5, 2)), dict(obs_delay=2), dict(obs_delay=(0, 1, 2))):
        with pytest.raises(ValueError):
            PPOConfig(**kw)
    for kw in (dict(obs_noise=(0.02, 0.05, 0.02, 0.1)), dict(obs_bias=(0.02, 0, 0.01, 0)),
               dict(obs_delay=(0, 2)), dict(obs_delay=(15, 15))):
        assert PPOConfig(**kw).sensor_on()
    # any variant and any env option take it
    PPOConfig(variant="rk4", obs_delay=(1, 1))
    PPOConfig(variant="tag", obs_noise=(0.1, 0, 0, 0))
    PPOConfig(wind_speed=1.0, obs_noise=(0.1, 0, 0, 0))


def test_step_limit_refusal_uses_the_wind_options_wording():
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.env import check_wind
    with pytest.raises(ValueError, match=r"max_steps below 2\^24") as e:
        K.check_sensor((0.1, 0, 0, 0), max_steps=1 << 24)
    with pytest.raises(ValueError) as w:
        check_wind("gym", gust_sigma=0.1, gust_rate=0.1, max_steps=1 << 24)
    assert str(e.value).split("needs")[1] == str(w.value).split("needs")[1]
    K.check_sensor((0.1, 0, 0, 0), max_steps=(1 << 24) - 1)


def test_train_flags_parse():
    from drone_rl_amd.train import build_parser, config_from_args
    a = build_parser().parse_args([])
    assert (a.obs_noise, a.obs_bias, a.obs_delay) == ((0.0,) * 4, (0.0,) * 4, (0, 0))
    assert not config_from_args(a).sensor_on()
    a = build_parser().parse_args(["--obs-noise", "0.02,0.05,0.02,0.1", "--obs-bias",
                                   "0.02,0,0.01,0", "--obs-delay", "0,2"])
    assert a.obs_noise == (0.02, 0.05, 0.02, 0.1) and a.obs_bias == (0.02, 0.0, 0.01, 0.0)
    assert a.obs_delay == (0, 2)
    c = config_from_args(a)
    assert c.sensor_on() and tuple(c.obs_delay) == (0, 2)
    for bad in (["--obs-noise", "0.1,0.1"], ["--obs-delay", "1"], ["--obs-delay", "a,b"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)
