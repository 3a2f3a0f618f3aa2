"""VecNormalize without a GPU: the NumPy restatement
against the moments of the concatenated stream, and every host-side check of
the new ABI, config fields and command-line flags."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from vecnorm_ref import RunningMeanStd, VecNormalizeRef

VECNORM_FUNCS = ("dr_vecnorm_workspace_bytes", "dr_vecnorm_init", "dr_vecnorm_step",
                 "dr_vecnorm_apply", "dr_vecnorm_unapply")


# ------------------------------------------------------------- restatement
def test_running_moments_equal_the_concatenated_stream():
    """After k batches from the initial state the statistics are the moments
    of the concatenated stream within 1e-9: the initial state weighs its
    count 1e-4 against k N = 4e5 rows, 2.5e-10, on columns whose mean and
    variance are of order 1."""
    rng = np.random.default_rng(0)
    n, d, k = 50000, 5, 8
    assert 1e-4 / (k * n) < 1e-9
    scale, offset = np.linspace(0.5, 2.0, d), np.linspace(-1.0, 1.0, d)
    batches = [rng.standard_normal((n, d)) * scale + offset for _ in range(k)]
    rms = RunningMeanStd((d,))
    for b in batches:
        rms.update(b)
    x = np.concatenate(batches)
    assert rms.count == 1e-4 + k * n
    assert np.all(np.abs(rms.mean - x.mean(axis=0)) <= 1e-9)
    assert np.all(np.abs(rms.var - x.var(axis=0)) <= 1e-9)


def test_constant_column_variance_goes_to_zero_and_output_to_zero():
    rng = np.random.default_rng(2)
    n, d = 512, 12
    ref = VecNormalizeRef(n, d)
    const = np.float32(3.25)
    out = None
    for k in range(6):
        obs = rng.standard_normal((n, d)).astype(np.float32)
        obs[:, 4] = const
        out = ref.reset(obs) if k == 0 else ref.step(obs, np.zeros(n, np.float32),
                                                     np.zeros(n, np.uint8))[0]
    # var = 1e-4 * (1 + const^2-ish) / count: the initial state's share only
    assert ref.obs_rms.var[4] < 1e-6
    assert abs(ref.obs_rms.mean[4] - const) < 1e-6
    assert np.all(np.abs(out[:, 4]) < 1e-2)
    # with the statistic exactly degenerate the output is exactly 0
    ref.obs_rms.mean[4], ref.obs_rms.var[4] = float(const), 0.0
    assert np.all(ref.normalize_obs(obs)[:, 4] == 0.0)


def test_step_order_and_done_handling():
    n, d = 4, 2
    ref = VecNormalizeRef(n, d, gamma=0.5)
    ref.reset(np.zeros((n, d), np.float32))
    rew = np.array([1, 2, 3, 4], np.float32)
    done = np.array([0, 1, 0, 1], np.uint8)
    term = np.full((n, d), 5, np.float32)
    sentinel = np.full((n, d), -1, np.float32)
    _, r, to = ref.step(np.ones((n, d), np.float32), rew, done, term, sentinel)
    # returns were updated over all envs before the zeroing of done ones
    assert ref.ret_rms.count == pytest.approx(1e-4 + n)
    assert np.array_equal(ref.returns, [1, 0, 3, 0])
    assert np.array_equal(to[0], sentinel[0]) and not np.array_equal(to[1], sentinel[1])
    assert np.allclose(r, rew / np.sqrt(ref.ret_rms.var + 1e-8))
    ref.step(np.ones((n, d), np.float32), rew, np.zeros(n, np.uint8))
    assert np.array_equal(ref.returns, [1.5, 2, 4.5, 4])


# -------------------------------------------------------------- validation
def test_header_declares_the_five_functions_and_abi_16():
    src = open(os.path.join(ROOT, "include", "dronerl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in VECNORM_FUNCS:
        assert re.search(r"\b%s\s*\(" % f, src), f
    assert re.search(r"#define\s+DR_ABI_VERSION\s+16\b", src)
    for name, val in (("DR_VECNORM_OBS", 1), ("DR_VECNORM_REWARD", 2), ("DR_VECNORM_TRAINING", 4)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, val), src), name
    from drone_rl_amd import _lib
    assert set(VECNORM_FUNCS) <= set(_lib.SIGNATURES)
    assert (_lib.DR_VECNORM_OBS, _lib.DR_VECNORM_REWARD, _lib.DR_VECNORM_TRAINING) == (1, 2, 4)
    assert _lib.lib().dr_abi_version() == 16


def _host_buffers(n, d):
    """Host memory standing in for device buffers: every call below must be
    refused before any HIP call, so nothing ever reads it."""
    from drone_rl_amd import _lib
    L = _lib.lib()
    mk = lambda k, t=ctypes.c_double: ctypes.cast((t * k)(), ctypes.c_void_p)
    b = dict(obs=mk(n * d, ctypes.c_float), rew=mk(n, ctypes.c_float),
             done=mk(n, ctypes.c_uint8), term=mk(n * d, ctypes.c_float),
             obs_rms=mk(1 + 2 * d), ret_rms=mk(3), returns=mk(n),
             obs_out=mk(n * d, ctypes.c_float), rew_out=mk(n, ctypes.c_float),
             term_out=mk(n * d, ctypes.c_float))
    nbytes = L.dr_vecnorm_workspace_bytes(n, d)
    b["ws"], b["ws_bytes"] = mk(nbytes // 8), nbytes
    return L, b


def _step(L, b, n=8, d=15, flags=7, gamma=0.99, clip_obs=10.0, clip_reward=10.0, eps=1e-8, **kw):
    a = dict(b)
    a.update(kw)
    return L.dr_vecnorm_step(n, d, a["obs"], a["rew"], a["done"], a["term"], flags, gamma,
                             clip_obs, clip_reward, eps, a["obs_rms"], a["ret_rms"], a["returns"],
                             a["obs_out"], a["rew_out"], a["term_out"], a["ws"], a["ws_bytes"],
                             None)


def test_workspace_bytes():
    from drone_rl_amd import _lib
    L = _lib.lib()
    assert L.dr_vecnorm_workspace_bytes(1, 15) > 0
    assert L.dr_vecnorm_workspace_bytes(65536, 15) >= L.dr_vecnorm_workspace_bytes(4099, 15)
    for n, d in ((0, 15), (8, 0), (8, 25), (-1, 15)):
        assert L.dr_vecnorm_workspace_bytes(n, d) == 0


@pytest.mark.parametrize("kw,word", [
    (dict(n=0), "n must"), (dict(d=0), "obs_dim"), (dict(d=25), "obs_dim"),
    (dict(clip_obs=0.0), "clip_obs"), (dict(clip_obs=-1.0), "clip_obs"),
    (dict(clip_obs=float("inf")), "clip_obs"), (dict(clip_obs=float("nan")), "clip_obs"),
    (dict(clip_reward=0.0), "clip_reward"), (dict(clip_reward=float("inf")), "clip_reward"),
    (dict(clip_reward=float("nan")), "clip_reward"),
    (dict(eps=-1e-9), "epsilon"), (dict(eps=float("nan")), "epsilon"),
    (dict(gamma=float("nan")), "gamma"), (dict(flags=8), "flag"),
    (dict(obs=None), "obs"), (dict(obs_out=None), "obs"), (dict(obs_rms=None), "obs_rms"),
    (dict(ret_rms=None), "ret_rms"), (dict(returns=None), "returns"),
    (dict(done=None), "dones"), (dict(rew_out=None), "rew_out"),
    (dict(term_out=None), "terminal"), (dict(term=None), "terminal"),
    (dict(rew=None, done=None, rew_out=None), "reset form"),
    (dict(ws=None), "workspace"), (dict(ws_bytes=8), "workspace"),
])
def test_step_argument_checks_need_no_gpu(kw, word):
    from drone_rl_amd import _lib
    L, b = _host_buffers(8, 15)
    rc = _step(L, b, **kw)
    assert rc == _lib.DR_ERR_INVALID
    assert word in _lib.last_error(), _lib.last_error()


def test_init_apply_unapply_argument_checks_need_no_gpu():
    from drone_rl_amd import _lib
    L, b = _host_buffers(8, 15)
    bad = _lib.DR_ERR_INVALID
    assert L.dr_vecnorm_init(0, 15, b["obs_rms"], b["ret_rms"], b["returns"], None) == bad
    assert L.dr_vecnorm_init(8, 25, b["obs_rms"], b["ret_rms"], b["returns"], None) == bad
    assert L.dr_vecnorm_init(8, 15, None, b["ret_rms"], b["returns"], None) == bad
    assert L.dr_vecnorm_init(8, 15, b["obs_rms"], None, b["returns"], None) == bad
    assert L.dr_vecnorm_init(8, 15, b["obs_rms"], b["ret_rms"], None, None) == bad
    ap = lambda m=8, d=15, obs=b["obs"], rms=b["obs_rms"], clip=10.0, eps=1e-8, out=b["obs_out"]: \
        L.dr_vecnorm_apply(m, d, obs, rms, clip, eps, out, None)
    for kw in (dict(m=0), dict(d=0), dict(d=25), dict(obs=None), dict(rms=None), dict(out=None),
               dict(clip=0.0), dict(clip=float("inf")), dict(clip=float("nan")), dict(eps=-1.0),
               dict(eps=float("nan"))):
        assert ap(**kw) == bad, kw
        assert "dr_vecnorm_apply" in _lib.last_error()
    un = lambda m=8, d=15, obs=b["obs"], rms=b["obs_rms"], eps=1e-8, out=b["obs_out"]: \
        L.dr_vecnorm_unapply(m, d, obs, rms, eps, out, None)
    for kw in (dict(m=0), dict(d=0), dict(d=25), dict(obs=None), dict(rms=None), dict(out=None),
               dict(eps=-1.0)):
        assert un(**kw) == bad, kw
        assert "dr_vecnorm_unapply" in _lib.last_error()


def test_config_refuses_bad_normalisation_values():
    from drone_rl_amd.ppo import PPOConfig
    c = PPOConfig()
    assert (c.normalize_obs, c.normalize_reward) == (False, False)
    assert (c.clip_obs, c.clip_reward, c.norm_epsilon) == (10.0, 10.0, 1e-8)
    for kw in (dict(clip_obs=0.0), dict(clip_obs=-1.0), dict(clip_reward=0.0),
               dict(clip_reward=float("inf")), dict(clip_obs=float("nan")),
               dict(norm_epsilon=-1e-8)):
        with pytest.raises(ValueError):
            PPOConfig(**kw)
    PPOConfig(normalize_obs=True, normalize_reward=True, clip_obs=5.0, norm_epsilon=0.0)


@pytest.mark.parametrize("kw", [dict(normalize_obs=True), dict(normalize_reward=True)])
def test_trainer_refuses_normalisation_across_ranks(kw):
    """Raised ahead of everything else: no device, no env is touched."""
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    with pytest.raises(ValueError, match="world_size"):
        PPOTrainer(PPOConfig(num_envs=256, n_steps=8, batch_size=256, **kw), device="cpu",
                   rank=0, world_size=2)


def test_train_flags_parse():
    from drone_rl_amd.train import build_parser
    a = build_parser().parse_args([])
    assert (a.normalize_obs, a.normalize_reward, a.clip_obs, a.clip_reward) == \
        (False, False, 10.0, 10.0)
    a = build_parser().parse_args(["--normalize-obs", "--normalize-reward", "--clip-obs", "5",
                                   "--clip-reward", "2.5"])
    assert (a.normalize_obs, a.normalize_reward, a.clip_obs, a.clip_reward) == \
        (True, True, 5.0, 2.5)
