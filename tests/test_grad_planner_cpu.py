"""The gradient planner without a GPU: every host-side
refusal of the new ABI and of the Python class, the restatement's adjoint
against central differences of its own cost, its fault modes on the device
comparison's own inputs, the +-1-ulp twin on the rows the device's iterated
comparison uses, and the law flown closed-loop on the oracle's step."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from gplan_ref import (DEFAULTS, FAULTS, HOVER, ITER_CASES, MOTOR_MAX, GplanRef, batches, bits,
                       grad_ratio, random_ulps, twin_differences)
from oracle.drone_np import gym_step_batched

GPLAN_FUNCS = ("dr_gplan_workspace_bytes", "dr_gplan_reset", "dr_gplan_step")
NAN, INF = float("nan"), float("inf")


# ---------------------------------------------------------------- the ABI
def test_header_and_binding_declare_the_planner():
    src = open(os.path.join(ROOT, "include", "dronerl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in GPLAN_FUNCS:
        assert re.search(r"\b%s\s*\(" % f, src), f
    assert re.search(r"#define\s+DR_ABI_VERSION\s+16\b", src)
    assert re.search(r"#define\s+DR_GPLAN_MAX_HORIZON\s+32\b", src)
    assert re.search(r"#define\s+DR_GPLAN_MAX_ITERATIONS\s+64\b", src)
    from drone_rl_amd import _lib
    assert set(GPLAN_FUNCS) <= set(_lib.SIGNATURES)
    assert ctypes.sizeof(_lib.dr_gplan_config) == 4 + 4 + 11 * 8
    assert [f[0] for f in _lib.dr_gplan_config._fields_] == list(DEFAULTS)
    assert _lib.lib().dr_abi_version() == 16


def _config(**kw):
    from drone_rl_amd import _lib
    return _lib.dr_gplan_config(**dict(DEFAULTS, **kw))


def _host_buffers(n=8, H=16):
    """Host memory standing in for device buffers: every call below must be
    refused before any HIP call, so nothing ever reads it."""
    from drone_rl_amd import _lib
    L = _lib.lib()
    mk = lambda k, t=ctypes.c_float: ctypes.cast((t * k)(), ctypes.c_void_p)
    size = L.dr_gplan_workspace_bytes(n, H)
    return L, dict(obs=mk(n * 15), dones=None, nominal=mk(n * H * 4),
                   workspace=mk(size // 8 + 1, ctypes.c_double), workspace_bytes=size,
                   actions_out=mk(n * 4), cost_out=None, grad_out=None)


STEP_ORDER = ("obs", "dones", "nominal", "workspace", "workspace_bytes", "actions_out", "cost_out",
              "grad_out")
# (call arguments, config fields, the word the message must hold); shared by both entry points
REFUSALS = [
    (dict(n=0), {}, "n must"), (dict(n=-3), {}, "n must"), (dict(n=1 << 31), {}, "n must"),
    ({}, dict(horizon=0), "horizon"), ({}, dict(horizon=33), "horizon"),
    ({}, dict(iterations=0), "iterations"), ({}, dict(iterations=65), "iterations"),
    ({}, dict(lr=0.0), "lr"), ({}, dict(lr=-0.1), "lr"), ({}, dict(lr=NAN), "lr"),
    ({}, dict(lr=INF), "lr"),
    ({}, dict(beta1=-0.1), "beta1"), ({}, dict(beta1=1.0), "beta1"), ({}, dict(beta1=NAN), "beta1"),
    ({}, dict(beta2=-0.1), "beta2"), ({}, dict(beta2=1.0), "beta2"), ({}, dict(beta2=NAN), "beta2"),
    ({}, dict(adam_eps=0.0), "adam_eps"), ({}, dict(adam_eps=NAN), "adam_eps"),
    ({}, dict(adam_eps=INF), "adam_eps"),
] + [({}, {w: bad}, w) for w in list(DEFAULTS)[6:] for bad in (-1.0, NAN, INF)] + [
    (dict(nominal=None), {}, "nominal"),
]


@pytest.mark.parametrize("kw,ckw,word", REFUSALS)
def test_argument_checks_need_no_gpu(kw, ckw, word):
    from drone_rl_amd import _lib
    L, b = _host_buffers()
    b.update({k: v for k, v in kw.items() if k != "n"})
    n = kw.get("n", 8)
    cfg = ctypes.byref(_config(**ckw))
    rc = L.dr_gplan_step(*[cfg, n] + [b[k] for k in STEP_ORDER] + [None])
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_gplan_step" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    rc = L.dr_gplan_reset(cfg, n, b["nominal"], None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_gplan_reset" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()


def test_step_only_workspace_and_null_config_checks_need_no_gpu():
    from drone_rl_amd import _lib
    L, b = _host_buffers()
    cfg = ctypes.byref(_config())
    short = b["workspace_bytes"] - 1
    odd = ctypes.c_void_p(b["workspace"].value + 4)
    for kw, word in ((dict(obs=None), "obs"), (dict(actions_out=None), "actions_out"),
                     (dict(workspace=None), "workspace"),
                     (dict(workspace_bytes=short), "workspace_bytes"),
                     (dict(workspace_bytes=0), "workspace_bytes"),
                     (dict(workspace=odd), "aligned")):
        rc = L.dr_gplan_step(*[cfg, 8] + [dict(b, **kw)[k] for k in STEP_ORDER] + [None])
        assert rc == _lib.DR_ERR_INVALID
        assert "dr_gplan_step" in _lib.last_error() and word in _lib.last_error(), _lib.last_error()
    assert L.dr_gplan_step(*[None, 8] + [b[k] for k in STEP_ORDER] + [None]) == _lib.DR_ERR_INVALID
    assert "dr_gplan_step" in _lib.last_error() and "config" in _lib.last_error()
    assert L.dr_gplan_reset(None, 8, b["nominal"], None) == _lib.DR_ERR_INVALID
    assert "dr_gplan_reset" in _lib.last_error() and "config" in _lib.last_error()


def test_workspace_bytes_counts_the_words_and_refuses_by_returning_zero():
    from drone_rl_amd import _lib
    L = _lib.lib()
    for n, H in ((1, 1), (3, 2), (65, 16), (4096, 32), ((1 << 31) - 1, 32)):
        # m, s: 4 H f64 each; the tape: 12 f64 per state between two steps; U: 4 H f32
        assert L.dr_gplan_workspace_bytes(n, H) == n * (8 * (8 * H + 12 * (H - 1)) + 4 * 4 * H)
    for n, H in ((0, 16), (-1, 16), (1 << 31, 16), (8, 0), (8, 33), (8, -1)):
        assert L.dr_gplan_workspace_bytes(n, H) == 0


# -------------------------------------------------------- the Python class
@pytest.mark.parametrize("kw,word", [
    (dict(n=0), "n"), (dict(n=2.5), "n"), (dict(n=True), "n"),
    (dict(horizon=0), "horizon"), (dict(horizon=33), "horizon"), (dict(horizon=4.0), "horizon"),
    (dict(iterations=0), "iterations"), (dict(iterations=65), "iterations"),
    (dict(iterations=True), "iterations"),
    (dict(lr=0), "lr"), (dict(lr=NAN), "lr"), (dict(lr="a"), "lr"),
    (dict(beta1=1.0), "beta1"), (dict(beta1=-0.5), "beta1"),
    (dict(beta2=1.0), "beta2"), (dict(beta2=NAN), "beta2"),
    (dict(adam_eps=0), "adam_eps"), (dict(adam_eps=INF), "adam_eps"),
] + [({w: bad}, w) for w in list(DEFAULTS)[6:] for bad in (-1, NAN)])
def test_the_class_refuses_bad_settings_before_any_device_work(kw, word):
    from drone_rl_amd import GradPlanner
    args = dict(n=4, device="cuda")
    args.update(kw)
    with pytest.raises(ValueError, match=r"\b%s\b" % word):
        GradPlanner(**args)


def test_the_class_refuses_other_obs_widths():
    import torch
    from drone_rl_amd import GradPlanner
    from drone_rl_amd.grad_planner import OBS_DIM
    assert OBS_DIM == 15
    p = object.__new__(GradPlanner)        # the width is checked before any state is touched
    for od in (12, 16, 18, 19):
        with pytest.raises(ValueError, match="gym variant only"):
            p.plan(torch.zeros(4, od))
    with pytest.raises(ValueError, match="gym variant only"):
        p.plan(torch.zeros(15))


# ----------------------------------------------------------- restatement
def _tilted(n, H, seed):
    rng = np.random.default_rng(seed)
    s = np.concatenate([rng.uniform(-1, 1, (n, 3)) + [0, 0, 2], rng.uniform(-1, 1, (n, 3)),
                        rng.uniform(-0.5, 0.5, (n, 3)), rng.uniform(-1, 1, (n, 3))], 1)
    obs = np.concatenate([s, rng.uniform(-1, 1, (n, 3))], 1).astype(np.float32)
    U = (HOVER + rng.uniform(-0.5, 0.5, (n, H, 4))).astype(np.float32)
    return obs, U


@pytest.mark.parametrize("H", [1, 5, 16])
def test_the_adjoint_equals_central_differences_of_the_cost(H):
    """D(h) = (c(U + h e) - c(U - h e)) / 2h at h = 2^-10 (exact in f32) is
    within h^2 |c'''| / 6 of dc/dU plus the cost's rounding over 2h.  The
    first is measured by the same difference at 2h, which errs four times as
    much: |D(2h) - D(h)| / 3, taken twice; the second counts 64 roundings of
    relative size 2^-53 on a cost of size c, more than its ~ 50 H operations
    leave after cancellation.  One f32 cast is not the identity the adjoint
    takes it for and does not cancel in the difference: the yaw torque f32(K
    psi), psi = a0 - a1 + a2 - a3, is rounded by up to 2^-24 K |psi| in each
    of the two costs, and c moves by nu2 = dc/dtau_psi times that, K nu2 =
    (g0 - g1 + g2 - g3) / 4 by the sign rows.  (The f32 sums of the mixes
    round alike in both costs: 2^-10 leaves their low bits alone.)  The bound
    must itself stay below 10^-4 of the gradient, so that it cannot pass a
    wrong adjoint."""
    n, h = 6, 2.0 ** -10
    obs, U = _tilted(n, H, seed=H)
    ref = GplanRef(n, horizon=H, w_effort=0.3)
    c, g = ref.cost_grad(obs, U)
    assert np.isfinite(g).all() and (np.abs(g).max((1, 2)) > 1e-3).all()

    def diff(step):
        d = np.zeros_like(g)
        for k in range(H):
            for j in range(4):
                up, um = U.copy(), U.copy()
                up[:, k, j] += np.float32(step)
                um[:, k, j] -= np.float32(step)
                assert (up[:, k, j] - um[:, k, j] == np.float32(2 * step)).all()
                d[:, k, j] = (ref.cost_grad(obs, up)[0] - ref.cost_grad(obs, um)[0]) / (2 * step)
        return d
    d1, d2 = diff(h), diff(2 * h)
    scale = np.abs(g).max((1, 2))
    psi = np.abs(((U[..., 0] - U[..., 1]) + U[..., 2]) - U[..., 3]).astype(np.float64)
    knu2 = np.abs(((g[..., 0] - g[..., 1]) + g[..., 2]) - g[..., 3]) / 4
    cast = 2 * (2.0 ** -24 * psi * knu2).sum(1) / (2 * h)
    bound = 2 * np.abs(d2 - d1).max((1, 2)) / 3 + 64 * 2.0 ** -53 * c / (2 * h) + cast
    err = np.abs(g - d1).max((1, 2))
    print("H=%d relative error %.3g, bound %.3g" % (H, (err / scale).max(), (bound / scale).max()))
    assert (bound / scale < 1e-4).all()
    assert (err <= bound).all(), (err / scale, bound / scale)


@pytest.mark.parametrize("fault", [f for f in FAULTS if f])
def test_fault_modes_differ_on_the_device_comparisons_inputs(fault):
    """On the device comparison's start rows each wrong law gives another
    gradient, action or nominal than the law: the comparisons on the device
    can fail.  The adjoint's faults must move the gradient by more than any
    bar the device test may derive (10^-6 of its size)."""
    n, H = 3, 16
    differ, moved = False, 0.0
    for obs, nom, bad in batches(n, H):
        a, b = GplanRef(n, horizon=H, iterations=3), GplanRef(n, horizon=H, iterations=3,
                                                              fault=fault)
        a.nominal, b.nominal = nom.copy(), nom.copy()
        oa, ob = a.plan(obs), b.plan(obs)
        ok = np.arange(n) != (-1 if bad is None else bad)
        moved = max(moved, float(grad_ratio(b.last_grad[ok], a.last_grad[ok]).max()))
        differ |= not np.array_equal(bits(oa), bits(ob))
        differ |= not np.array_equal(bits(a.nominal), bits(b.nominal))
    assert differ
    if fault in ("no_lp_dt", "theta_sign"):
        assert moved > 1e-6, moved
    else:
        assert moved == 0.0


@pytest.mark.parametrize("n,H,I", ITER_CASES)
def test_the_one_ulp_twin_stays_inside_the_iterated_comparisons_cap(n, H, I):
    """The device's sin / cos are within 1 ulp of the restatement's.  A twin
    of the restatement whose sin / cos are moved by seeded +-1 ulp must itself
    pass what the device's iterated comparison asks on the same rows: every
    entry of the new nominal within 1 f32 ulp, at most 1 in 100 different."""
    total = differing = 0
    for seed in range(3):
        for obs, nom, bad in batches(n, H):
            far, diff, count = twin_differences(n, H, I, obs, nom, bad, seed)
            assert far == 0
            total += count
            differing += diff
    print("twin: %d of %d entries differ" % (differing, total))
    assert differing * 100 <= total


# ------------------------------------------------------------ the law flies
def test_the_law_flies_on_the_oracle_step():
    """8 envs, 120 steps, eps 0, the defaults: the mean return is above the
    20.70 MPPI's restatement collects on this shape (test_planner_cpu prints
    it) and no env crashes."""
    n, steps = 8, 120
    u = np.random.default_rng(5).random((n, 2))
    z = np.zeros((n, 3))
    s = {"pos": np.stack([u[:, 0] - 0.5, u[:, 1] - 0.5, np.ones(n)], 1), "vel": z.copy(),
         "euler": z.copy(), "omega": z.copy(), "target": z + [0.0, 0.0, 1.0],
         "step": np.zeros(n, np.int32)}
    obs = np.concatenate([s["pos"], s["vel"], s["euler"], s["omega"], s["target"] - s["pos"]],
                         1).astype(np.float32)
    ref = GplanRef(n)
    ret, crashed = np.zeros(n), np.zeros(n, bool)
    for t in range(steps):
        a = ref.plan(obs)
        assert ((a >= 0) & (a <= MOTOR_MAX)).all()
        obs, r, d = gym_step_batched(s, a)
        ret += r
        crashed |= d
    print("planned %.3f" % ret.mean())
    assert not crashed.any()
    assert ret.mean() > 20.70
