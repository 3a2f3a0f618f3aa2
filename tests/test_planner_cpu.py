"""The MPPI planner without a GPU: every host-side
refusal of the new ABI and of the Python class, the restatement's fault modes
on the device comparison's own inputs, its noise statistics, and the law flown
closed-loop on the oracle's step."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from mppi_ref import (CALLS0, HOVER, MOTOR_MAX, SHAPES, START_ROWS, MppiRef, bits, chunks, clip,
                      make_ref)
from oracle.drone_np import gym_step_batched

MPPI_FUNCS = ("dr_mppi_reset", "dr_mppi_step")


# ---------------------------------------------------------------- the ABI
def test_header_and_binding_declare_the_planner():
    src = open(os.path.join(ROOT, "include", "dronerl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in MPPI_FUNCS:
        assert re.search(r"\b%s\s*\(" % f, src), f
    assert re.search(r"#define\s+DR_ABI_VERSION\s+16\b", src)
    assert re.search(r"#define\s+DR_MPPI_MAX_SAMPLES\s+1024\b", src)
    assert re.search(r"#define\s+DR_MPPI_MAX_HORIZON\s+32\b", src)
    from drone_rl_amd import _lib
    assert set(MPPI_FUNCS) <= set(_lib.SIGNATURES)
    assert ctypes.sizeof(_lib.dr_mppi_config) == 4 + 4 + 5 * 8 + 8 + 8
    assert _lib.lib().dr_abi_version() == 16
    common = open(os.path.join(ROOT, "drone_rl_amd", "csrc", "common.h")).read()
    tags = re.findall(r"TAG_[A-Z]+\s*=\s*0x([0-9A-Fa-f]{8})u", common)
    assert "4D000000" in [t.upper() for t in tags] and len(set(tags)) == len(tags)
    # no other consumer's top byte: the sensor model's 0x53 and 0x60..0x65 included
    tops = {int(t[:2], 16) for t in tags} | {0x53} | set(range(0x60, 0x66))
    assert len(tops) == len(tags) + 7


def _config(**kw):
    from drone_rl_amd import _lib
    d = dict(samples=256, horizon=16, sigma=0.3, temperature=0.05, gamma=1.0, crash_cost=10.0,
             terminal_weight=1.0, seed=1, env_id_offset=0)
    d.update(kw)
    return _lib.dr_mppi_config(**d)


def _host_buffers(n=8, S=256, H=16):
    """Host memory standing in for device buffers: every call below must be
    refused before any HIP call, so nothing ever reads it."""
    from drone_rl_amd import _lib
    mk = lambda k, t=ctypes.c_float: ctypes.cast((t * k)(), ctypes.c_void_p)
    return _lib.lib(), dict(obs=mk(n * 15), dones=None, nominal=mk(n * H * 4),
                            calls=mk(n, ctypes.c_uint32), actions_out=mk(n * 4), costs_out=None)


NAN, INF = float("nan"), float("inf")
# (call arguments, config fields, the word the message must hold); shared by both entry points
REFUSALS = [
    (dict(n=0), {}, "n must"), (dict(n=-3), {}, "n must"),
    ({}, dict(samples=0), "samples"), ({}, dict(samples=100), "samples"),
    ({}, dict(samples=2048), "samples"), ({}, dict(samples=32), "samples"),
    ({}, dict(horizon=0), "horizon"), ({}, dict(horizon=33), "horizon"),
    ({}, dict(sigma=-0.1), "sigma"), ({}, dict(sigma=NAN), "sigma"), ({}, dict(sigma=INF), "sigma"),
    ({}, dict(temperature=0.0), "temperature"), ({}, dict(temperature=-1.0), "temperature"),
    ({}, dict(temperature=NAN), "temperature"), ({}, dict(temperature=INF), "temperature"),
    ({}, dict(gamma=0.0), "gamma"), ({}, dict(gamma=1.01), "gamma"), ({}, dict(gamma=NAN), "gamma"),
    ({}, dict(crash_cost=-1.0), "crash_cost"), ({}, dict(crash_cost=INF), "crash_cost"),
    ({}, dict(crash_cost=NAN), "crash_cost"),
    ({}, dict(terminal_weight=-1.0), "terminal_weight"),
    ({}, dict(terminal_weight=INF), "terminal_weight"),
    ({}, dict(terminal_weight=NAN), "terminal_weight"),
    (dict(nominal=None), {}, "nominal"), (dict(calls=None), {}, "calls"),
]


@pytest.mark.parametrize("kw,ckw,word", REFUSALS)
def test_argument_checks_need_no_gpu(kw, ckw, word):
    from drone_rl_amd import _lib
    L, b = _host_buffers()
    b.update({k: v for k, v in kw.items() if k != "n"})
    n = kw.get("n", 8)
    cfg = ctypes.byref(_config(**ckw))
    rc = L.dr_mppi_step(cfg, n, b["obs"], b["dones"], b["nominal"], b["calls"], b["actions_out"],
                        b["costs_out"], None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_mppi_step" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    rc = L.dr_mppi_reset(cfg, n, b["nominal"], b["calls"], None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_mppi_reset" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()


def test_step_only_and_null_config_checks_need_no_gpu():
    from drone_rl_amd import _lib
    L, b = _host_buffers()
    cfg = ctypes.byref(_config())
    order = ("obs", "dones", "nominal", "calls", "actions_out", "costs_out")
    for kw, word in ((dict(obs=None), "obs"), (dict(actions_out=None), "actions_out")):
        rc = L.dr_mppi_step(*[cfg, 8] + [dict(b, **kw)[k] for k in order] + [None])
        assert rc == _lib.DR_ERR_INVALID
        assert "dr_mppi_step" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    assert L.dr_mppi_step(*[None, 8] + [b[k] for k in order] + [None]) == _lib.DR_ERR_INVALID
    assert "dr_mppi_step" in _lib.last_error() and "config" in _lib.last_error()
    assert L.dr_mppi_reset(None, 8, b["nominal"], b["calls"], None) == _lib.DR_ERR_INVALID
    assert "dr_mppi_reset" in _lib.last_error() and "config" in _lib.last_error()


# -------------------------------------------------------- the Python class
@pytest.mark.parametrize("kw,word", [
    (dict(n=0), "n"), (dict(n=2.5), "n"),
    (dict(samples=100), "samples"), (dict(samples=256.0), "samples"), (dict(samples=True), "samples"),
    (dict(horizon=0), "horizon"), (dict(horizon=33), "horizon"), (dict(horizon=4.0), "horizon"),
    (dict(sigma=-0.1), "sigma"), (dict(sigma=NAN), "sigma"), (dict(sigma="a"), "sigma"),
    (dict(temperature=0), "temperature"), (dict(temperature=INF), "temperature"),
    (dict(gamma=0), "gamma"), (dict(gamma=1.5), "gamma"), (dict(gamma=NAN), "gamma"),
    (dict(crash_cost=-1), "crash_cost"), (dict(crash_cost=INF), "crash_cost"),
    (dict(terminal_weight=-1), "terminal_weight"), (dict(terminal_weight=NAN), "terminal_weight"),
])
def test_the_class_refuses_bad_settings_before_any_device_work(kw, word):
    from drone_rl_amd import MPPIPlanner
    args = dict(n=4, device="cuda")
    args.update(kw)
    with pytest.raises(ValueError, match=r"\b%s\b" % word):
        MPPIPlanner(**args)


def test_the_class_refuses_other_obs_widths():
    import torch
    from drone_rl_amd import MPPIPlanner
    from drone_rl_amd.planner import OBS_DIM
    assert OBS_DIM == 15
    p = object.__new__(MPPIPlanner)        # the width is checked before any state is touched
    for od in (12, 16, 18, 19):
        with pytest.raises(ValueError, match="gym variant only"):
            p.plan(torch.zeros(4, od))
    with pytest.raises(ValueError, match="gym variant only"):
        p.plan(torch.zeros(15))


# ----------------------------------------------------------- restatement
@pytest.mark.parametrize("fault", ["perturb_sample0", "no_shift", "crash_sign", "stale_calls"])
def test_fault_modes_differ_on_the_device_comparisons_inputs(fault):
    """On the device comparison's start rows each wrong law gives other costs,
    actions or state than the law within two plan steps: the comparisons on
    the device can fail."""
    n, S, H, g = 3, 64, 16, 0.97
    assert (n, S, H, g) in SHAPES
    differ = False
    for names, obs, nom in chunks(n, H):
        a, b = make_ref(n, S, H, g, nom), make_ref(n, S, H, g, nom, fault=fault)
        for _ in range(2):
            oa, ob = a.plan(obs), b.plan(obs)
            differ |= not np.array_equal(bits(a.last_actions), bits(b.last_actions))
            differ |= not np.array_equal(bits(a.last_costs), bits(b.last_costs))
            differ |= not np.array_equal(bits(oa), bits(ob))
            differ |= not np.array_equal(bits(a.nominal), bits(b.nominal))
            differ |= not np.array_equal(a.calls, b.calls)
    assert differ
    assert (a.calls == CALLS0 + 2).all()


def test_the_start_rows_cover_what_they_claim():
    names = [r[0] for r in START_ROWS]
    assert names == ["hover", "tilted", "low", "edge", "far", "bonus", "clips"]
    for n, S, H, g in SHAPES:
        mixed = False
        for nm, obs, nom in chunks(n, H):
            ref = make_ref(n, S, H, g, nom)
            acts = ref.actions()
            assert np.array_equal(bits(acts[:, 0]), bits(clip(nom)))
            _, alive = ref.returns(obs, acts)
            mixed |= bool(((alive.sum(1) > 0) & (alive.sum(1) < S)).any())
            if "clips" in nm:
                a = acts[nm.index("clips")]
                assert (a == 0).any() and (a == MOTOR_MAX).any()
                assert ((a > 0) & (a < MOTOR_MAX)).any()
        assert mixed, (n, S, H, g)
    row = dict((r[0], r[1].astype(np.float64)) for r in START_ROWS)
    assert 49.9 < np.linalg.norm(row["far"][:3]) < 50 and row["far"][:3] @ row["far"][3:6] > 0
    assert np.linalg.norm(row["bonus"][12:15]) < 0.05
    assert np.abs(row["tilted"][6:8]).min() >= 0.6 - 1e-6 and np.abs(row["tilted"][9:12]).min() > 0
    assert np.float32(0.01) == row["low"][2].astype(np.float32) and row["low"][5] < 0


def test_restated_noise_has_mean_zero_and_the_given_std():
    sigma, S, H = 0.3, 1024, 32
    ref = MppiRef(2, S, H, sigma=sigma, seed=5)
    ref.nominal[:] = np.float32(3.0)            # far from both clips
    ref.calls[:] = [0, 7]
    e = (ref.actions()[:, 1:].astype(np.float64) - 3.0).ravel()
    m = e.size
    assert m >= 2 * 10 ** 5
    assert abs(e.mean()) < 5 * sigma / math.sqrt(m)
    # a uniform's variance estimate: var(e^2) = (9/5 - 1) sigma^4
    assert abs(e.var() - sigma ** 2) < 5 * math.sqrt(0.8 / m) * sigma ** 2
    assert np.abs(e).max() <= sigma * math.sqrt(3) * (1 + 1e-5)


# ------------------------------------------------------------ the law flies
def _fly(policy, n, steps, seed):
    """Mean undiscounted return of one episode per env on the oracle's step
    from the gym's eps = 0 reset (target (0, 0, 1)), up to the first done."""
    u = np.random.default_rng(seed).random((n, 2))
    z = np.zeros((n, 3))
    s = {"pos": np.stack([u[:, 0] - 0.5, u[:, 1] - 0.5, np.ones(n)], 1), "vel": z.copy(),
         "euler": z.copy(), "omega": z.copy(), "target": z + [0.0, 0.0, 1.0],
         "step": np.zeros(n, np.int32)}
    obs = np.concatenate([s["pos"], s["vel"], s["euler"], s["omega"], s["target"] - s["pos"]],
                         1).astype(np.float32)
    ret, alive = np.zeros(n), np.ones(n, bool)
    for t in range(steps):
        obs, r, d = gym_step_batched(s, policy(obs))
        ret += np.where(alive, r, 0.0)
        alive &= ~d
    return ret.mean()


def test_the_law_flies_on_the_oracle_step():
    n, steps = 8, 120
    ref = MppiRef(n, 128, 16, sigma=0.3, temperature=0.05)
    planned = _fly(ref.plan, n, steps, seed=5)
    hover = _fly(lambda o: np.full((n, 4), HOVER, np.float32), n, steps, seed=5)
    rng = np.random.default_rng(9)
    rand = _fly(lambda o: rng.uniform(0, MOTOR_MAX, (n, 4)).astype(np.float32), n, steps, seed=5)
    print("planned %.3f hover %.3f random %.3f" % (planned, hover, rand))
    # every step outside the 5 cm radius pays: a positive return needs steps inside it
    assert planned > 0
    assert planned > hover and planned > rand
    assert (ref.calls == steps).all()
