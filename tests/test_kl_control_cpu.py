"""KL control of the optimizer step without a GPU:
known answers of the NumPy restatement tests/kl_ref.py, and every host-side
check of the settings, the checkpoint formats, the ABI and the command line."""
import ctypes
import json
import os
import re
import zipfile

import numpy as np
import pytest
import torch

import kl_ref
from conftest import ROOT
from kl_ref import Slot, f32

KL_FUNCS = ("dr_clip_adam_kl", "dr_grad_finish_clip_adam_kl")


# ------------------------------------------------------------- restatement
def test_stop_is_sticky_and_the_tripping_step_is_unapplied():
    # 1.5 * 0.02 = 0.03: step 2 trips, later small KLs do not resume
    slots, applied = kl_ref.run([0.0, 0.01, 0.031, 0.0, 0.001], 3e-4, target_kl=0.02)
    assert [a is not None for a in applied] == [True, True, False, False, False]
    assert [s.stopped for s in slots] == [0, 0, 0, 1, 1, 1]
    assert [s.taken for s in slots] == [0, 1, 2, 2, 2, 2]
    assert all(s.lr == f32(3e-4) for s in slots)
    assert slots[4] == slots[3]                 # stopped: the next slot is a copy


def test_trip_compares_against_the_f32_product_strictly():
    t = 0.02
    edge = kl_ref.stop_kl(t)
    assert edge == f32(1.5 * t) and edge.dtype == np.float32
    assert kl_ref.run([edge], 1e-3, target_kl=t)[0][1] == Slot(0, 1, f32(1e-3))
    assert kl_ref.run([np.nextafter(edge, f32(1))], 1e-3, target_kl=t)[0][1].stopped == 1


def test_nan_does_not_stop_and_does_not_move_the_rate():
    slots, applied = kl_ref.run([np.nan, np.nan], 1e-3, target_kl=0.01, adaptive=True)
    assert all(a is not None for a in applied)
    assert slots[-1] == Slot(0, 2, f32(1e-3))


def test_zero_kl_never_raises_the_rate():
    slots, _ = kl_ref.run([0.0] * 4, 1e-4, adaptive=True, desired_kl=0.01)
    assert all(s.lr == f32(1e-4) for s in slots)
    # the smallest positive kl does
    slots, _ = kl_ref.run([np.float32(1e-45)], 1e-4, adaptive=True, desired_kl=0.01)
    assert slots[1].lr == f32(f32(1e-4) * f32(1.5))


def test_adaptive_moves_by_exact_factors_and_clamps():
    kw = dict(adaptive=True, desired_kl=0.01, lr_min=5e-4, lr_max=2e-3)
    # high KL: /1.5 down to the lower clamp, which then holds
    slots, _ = kl_ref.run([0.021] * 3, 1e-3, **kw)
    assert slots[1].lr == f32(f32(1e-3) / f32(1.5))
    assert slots[2].lr == f32(5e-4) and slots[3].lr == f32(5e-4)
    # low KL: *1.5 up to the upper clamp
    slots, _ = kl_ref.run([0.004] * 3, 1e-3, **kw)
    assert slots[1].lr == f32(f32(1e-3) * f32(1.5))
    assert slots[2].lr == f32(2e-3) and slots[3].lr == f32(2e-3)
    # inside [desired / 2, 2 desired], the bounds included: hold
    slots, _ = kl_ref.run([0.005, 0.01, 0.02, f32(0.02), f32(0.005)], 1e-3, **kw)
    assert all(s.lr == f32(1e-3) for s in slots)
    # the adjusted rate is the one the same step uses
    _, applied = kl_ref.run([0.021], 1e-3, **kw)
    assert applied[0] == (0, f32(f32(1e-3) / f32(1.5)))


def test_taken_indexes_the_schedule():
    table = kl_ref.adam_table(3e-4, 0.9, 0.999, 11, 4)
    assert table.dtype == np.float32 and table.shape == (4, 2)
    assert table[0][0] == f32(3e-4 / (1 - 0.9 ** 11))
    slots, applied = kl_ref.run([0.0, 0.01, 0.5, 0.0], 3e-4, target_kl=0.1)
    assert applied[:2] == [(0, f32(3e-4)), (1, f32(3e-4))] and applied[2:] == [None, None]
    assert kl_ref.step_scalars(table, applied[1]) == (table[1][0], table[1][1])
    unit = kl_ref.adam_table(1.0, 0.9, 0.999, 11, 4)
    s0, s1 = kl_ref.step_scalars(unit, (1, f32(2e-4)), adaptive=True)
    assert s0 == f32(f32(2e-4) * unit[1][0]) and s1 == unit[1][1]


def test_run_adam_skips_leave_the_state_alone():
    rng = np.random.default_rng(0)
    n = 33
    p, m, v = (rng.standard_normal(n).astype(f32), np.zeros(n, f32), np.zeros(n, f32))
    grads = [rng.standard_normal(n).astype(f32) for _ in range(4)]
    table = kl_ref.adam_table(1e-3, 0.9, 0.999, 1, 4)
    slots, applied, states = kl_ref.run_adam([0.0, 0.2, 0.0, 0.0], grads, p, m, v, table, 1e-3,
                                             target_kl=0.1)
    assert [a is not None for a in applied] == [True, False, False, False]
    want = kl_ref.clip_adam(p, grads[0], m, v, table[0][0], table[0][1])
    for j in range(4):
        for got, exp in zip(states[j], (want[0], want[2], want[3])):
            assert np.array_equal(got, exp)
    assert not np.array_equal(states[0][0], p)
    assert np.array_equal(slots[-1].words(), [1, 1, f32(1e-3).view(np.uint32), 0])


# -------------------------------------------------------------- refusals
def test_defaults_are_off():
    from drone_rl_amd.ppo import PPOConfig
    c = PPOConfig()
    assert (c.target_kl, c.lr_schedule, c.desired_kl, c.lr_min, c.lr_max) == \
        (None, "constant", 0.01, 1e-6, 1e-2)
    assert not c.kl_control_on()
    assert PPOConfig(target_kl=0.02).kl_control_on()
    assert PPOConfig(lr_schedule="linear").kl_control_on()
    d = PPOConfig.sb3_defaults()
    assert (d.target_kl, d.lr_schedule) == (None, "constant")


@pytest.mark.parametrize("kw,text", [
    (dict(target_kl=0.0), "target_kl must be None or > 0 and finite"),
    (dict(target_kl=-0.01), "target_kl must be None or > 0 and finite"),
    (dict(target_kl=float("nan")), "target_kl must be None or > 0 and finite"),
    (dict(target_kl=float("inf")), "target_kl must be None or > 0 and finite"),
    (dict(target_kl=1e39), "must fit f32"),
    (dict(desired_kl=0.0), "desired_kl must be > 0 and finite"),
    (dict(desired_kl=float("nan")), "desired_kl must be > 0 and finite"),
    (dict(desired_kl=float("inf")), "desired_kl must be > 0 and finite"),
    (dict(desired_kl=1e39), "desired_kl must be > 0 and finite"),
    (dict(lr_max=1e39), "lr_max must be > 0 and finite"),
    (dict(lr_min=1e-60), "lr_min must be > 0 and finite"),
    (dict(lr_schedule="cosine"), "unknown lr_schedule 'cosine'"),
    (dict(lr_min=0.0), "lr_min must be > 0 and finite"),
    (dict(lr_max=float("inf")), "lr_max must be > 0 and finite"),
    (dict(lr_max=float("nan")), "lr_max must be > 0 and finite"),
    (dict(lr_min=1e-2, lr_max=1e-3), "lr_min must be <= lr_max"),
])
def test_config_refuses(kw, text):
    from drone_rl_amd.ppo import PPOConfig
    with pytest.raises(ValueError, match=re.escape(text)):
        PPOConfig(**kw)


@pytest.mark.parametrize("kw", [dict(target_kl=0.02), dict(lr_schedule="linear"),
                                dict(lr_schedule="adaptive")])
@pytest.mark.parametrize("dp", [dict(world_size=2), dict(force_dp_path=True)])
def test_trainer_refuses_kl_control_across_ranks(kw, dp):
    """Raised ahead of everything else: no device, no env is touched."""
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    cfg = dict(num_envs=256, n_steps=8, batch_size=256, **kw)
    world = dp.get("world_size", 1)
    if "force_dp_path" in dp:
        cfg["force_dp_path"] = True
    with pytest.raises(ValueError, match="world_size 1 and the single-GPU step"):
        PPOTrainer(PPOConfig(**cfg), device="cpu", rank=0, world_size=world)


# ---------------------------------------------------------------- the ABI
def test_header_declares_the_entry_points_and_abi_16():
    src = open(os.path.join(ROOT, "include", "dronerl.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for f in KL_FUNCS:
        assert re.search(r"\b%s\s*\(" % f, src), f
    assert re.search(r"typedef struct dr_kl_gate\b", src)
    assert re.search(r"#define\s+DR_ABI_VERSION\s+16\b", src)
    from drone_rl_amd import _lib
    assert set(KL_FUNCS) <= set(_lib.SIGNATURES)
    assert _lib.lib().dr_abi_version() == 16


def test_gate_struct_layout():
    from drone_rl_amd import _lib
    g = _lib.dr_kl_gate
    assert ctypes.sizeof(g) == 64
    assert [getattr(g, n).offset for n, _ in g._fields_] == \
        [0, 8, 16, 24, 32, 40, 44, 48, 52, 56, 60]


def _gate(**kw):
    from drone_rl_amd import _lib
    buf = (ctypes.c_float * 64)()
    base = ctypes.addressof(buf)
    base += (-base) % 16
    a = dict(control=base, num_steps=3, step=0, kl=base + 64, sched=base + 96, stop_kl=0.03,
             adaptive=0, kl_high=0.02, kl_low=0.005, lr_min=1e-6, lr_max=1e-2)
    a.update(kw)
    g = _lib.dr_kl_gate(**a)
    g._keep = buf
    return g


@pytest.mark.parametrize("kw,word", [
    (dict(control=None), "control"), (dict(num_steps=0), "num_steps"),
    (dict(step=3), "num_steps"), (dict(step=-1), "num_steps"),
    (dict(kl=None), "kl and sched"), (dict(sched=None), "kl and sched"),
    (dict(stop_kl=-1.0), "stop_kl"), (dict(stop_kl=float("nan")), "stop_kl"),
    (dict(stop_kl=float("inf")), "stop_kl"), (dict(adaptive=2), "adaptive"),
    (dict(adaptive=1, kl_low=0.0), "kl_low"), (dict(adaptive=1, kl_high=0.001), "kl_low"),
    (dict(adaptive=1, lr_min=0.0), "lr_min"), (dict(adaptive=1, lr_max=1e-7), "lr_min"),
    (dict(adaptive=1, lr_max=float("inf")), "lr_min"),
])
def test_entry_points_check_the_gate_before_any_device_work(kw, word):
    """Host memory stands in for device buffers: every call is refused before
    any HIP call, so nothing reads it."""
    from drone_rl_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    g = _gate(**kw)
    rc = L.dr_clip_adam_kl(10, p, p, p, p, 0.9, 0.999, 1e-5, 0.5, ctypes.byref(g), None, p,
                           L.dr_adam_workspace_bytes(10), None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_clip_adam_kl" in _lib.last_error() and word in _lib.last_error()
    f = _lib.dr_grad_finish()
    rc = L.dr_grad_finish_clip_adam_kl(ctypes.byref(f), 10, p, p, p, p, 0.9, 0.999, 1e-5, 0.5,
                                       ctypes.byref(g), None, p, 4096, None)
    assert rc == _lib.DR_ERR_INVALID
    assert "dr_grad_finish_clip_adam_kl" in _lib.last_error() and word in _lib.last_error()


def test_entry_points_refuse_null_buffers_and_gate():
    from drone_rl_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    g = _gate()
    bad = _lib.DR_ERR_INVALID
    assert L.dr_clip_adam_kl(0, p, p, p, p, 0.9, 0.999, 1e-5, 0.5, ctypes.byref(g), None, p,
                             4096, None) == bad
    assert L.dr_clip_adam_kl(10, None, p, p, p, 0.9, 0.999, 1e-5, 0.5, ctypes.byref(g), None, p,
                             4096, None) == bad
    assert L.dr_clip_adam_kl(10, p, p, p, p, 0.9, 0.999, 1e-5, 0.5, None, None, p, 4096,
                             None) == bad
    assert "null gate" in _lib.last_error()
    assert L.dr_clip_adam_kl(10, p, p, p, p, 0.9, 0.999, 1e-5, 0.5, ctypes.byref(g), None, p, 0,
                             None) == bad
    assert "workspace" in _lib.last_error()
    assert L.dr_grad_finish_clip_adam_kl(None, 10, p, p, p, p, 0.9, 0.999, 1e-5, 0.5,
                                         ctypes.byref(g), None, p, 4096, None) == bad


# ------------------------------------------------------------- checkpoints
class _Recorder:
    """test_sb3_zip's stand-in trainer with the KL settings."""

    def __init__(self, seed, target_kl):
        from test_sb3_zip import _Cfg, _Env, _Opt
        from drone_rl_amd.policy import ActorCritic
        self.cfg = _Cfg()
        for k, v in dict(target_kl=target_kl, lr_schedule="constant", desired_kl=0.01,
                         lr_min=1e-6, lr_max=1e-2).items():
            setattr(self.cfg, k, v)
        self.policy = ActorCritic(15, 4, self.cfg.net_arch, "cpu", seed=seed)
        self.opt = _Opt(self.policy.num_params, 3)
        self.env = _Env(self.cfg.num_envs)
        self.num_timesteps, self.num_updates, self.world = 100, 1, 1
        self.enabled = None

    def _enable_kl(self, *a, **kw):
        self.enabled = a
        self.cfg.target_kl = a[0]


def test_sb3_zip_round_trips_target_kl(tmp_path):
    from drone_rl_amd import sb3_zip
    a = _Recorder(1, 0.015)
    sb3_zip.save(a, tmp_path / "a.zip")
    with zipfile.ZipFile(tmp_path / "a.zip") as z:
        assert json.loads(z.read("data"))["target_kl"] == 0.015
    b = _Recorder(2, None)
    sb3_zip.load_into(b, tmp_path / "a.zip")
    assert b.enabled == (0.015, "constant", 0.01, 1e-6, 1e-2) and b.cfg.target_kl == 0.015
    # a trainer with its own target keeps it; a zip without one enables nothing
    c = _Recorder(3, 0.5)
    sb3_zip.load_into(c, tmp_path / "a.zip")
    assert c.enabled is None and c.cfg.target_kl == 0.5
    sb3_zip.save(_Recorder(1, None), tmp_path / "n.zip")
    with zipfile.ZipFile(tmp_path / "n.zip") as z:
        assert json.loads(z.read("data"))["target_kl"] is None
    d = _Recorder(4, None)
    sb3_zip.load_into(d, tmp_path / "n.zip")
    assert d.enabled is None


# ------------------------------------------------------------ command line
def test_train_flags_parse_into_the_config():
    from drone_rl_amd.train import build_parser, config_from_args
    a = build_parser().parse_args([])
    assert a.target_kl is None
    assert (a.lr_schedule, a.desired_kl, a.lr_min, a.lr_max) == ("constant", 0.01, 1e-6, 1e-2)
    c = config_from_args(a)
    assert c.target_kl is None and not c.kl_control_on()
    a = build_parser().parse_args(["--target-kl", "0.02", "--lr-schedule", "adaptive",
                                   "--desired-kl", "0.008", "--lr-min", "1e-5", "--lr-max",
                                   "3e-3", "--envs", "256", "--batch-size", "256"])
    c = config_from_args(a)
    assert (c.target_kl, c.lr_schedule, c.desired_kl, c.lr_min, c.lr_max) == \
        (0.02, "adaptive", 0.008, 1e-5, 3e-3)
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--lr-schedule", "cosine"])


def test_lazy_step_count():
    """ClipAdam.t: a deferred count is fetched once, when t is first read."""
    from drone_rl_amd import ppo_kernels as K
    opt = K.ClipAdam.__new__(K.ClipAdam)
    opt._t, opt._t_pending = 4, None
    calls = []
    opt.defer_steps(lambda: calls.append(1) or 3)
    assert not calls
    assert opt.t == 7 and opt.t == 7 and calls == [1]
    opt.defer_steps(lambda: 100)
    opt.t = 2                       # an assignment drops a pending count
    assert opt.t == 2
    opt.t += 5
    assert opt.t == 7
