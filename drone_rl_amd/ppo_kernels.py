"""torch-facing wrappers of the PPO HIP kernels in libdronerl.so.

Each call enqueues work on the current HIP stream of the tensors' device and
returns device tensors; nothing here synchronises with the host.  Semantics
follow stable-baselines3 PPO (reference call sites
/root/reference/train.py:36-43, 63-68).
"""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._lib import check, ptr


def _s(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def _f32(t):
    assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), \
        "expected a contiguous f32 device tensor"
    return t


def gae(rewards, values, episode_starts, last_values, last_dones, gamma=0.99,
        gae_lambda=0.95, advantages=None, returns=None):
    """(T,N) rewards/values/episode_starts(u8), (N,) last_values/last_dones(u8)
    -> advantages, returns (T,N) f32 (RolloutBuffer.compute_returns_and_advantage)."""
    T, N = rewards.shape
    adv = torch.empty_like(rewards) if advantages is None else advantages
    ret = torch.empty_like(rewards) if returns is None else returns
    check(_lib.lib().dr_gae(T, N, ptr(_f32(rewards)), ptr(_f32(values)),
                            ptr(episode_starts.contiguous()), ptr(_f32(last_values)),
                            ptr(last_dones.contiguous()), float(gamma), float(gae_lambda),
                            ptr(adv), ptr(ret), _s(rewards)))
    return adv, ret


def policy_sample(mean, log_std, seed, counter, lo, hi, actions_raw=None,
                  actions_clipped=None, logp=None):
    """Diagonal-Gaussian sample a = mean + exp(log_std) z, its log-prob, and
    the clipped action passed to the env (SB3 collect_rollouts)."""
    n = mean.shape[0]
    check(_lib.lib().dr_policy_sample(n, ptr(_f32(mean)), ptr(_f32(log_std)),
                                      seed & (2**64 - 1), counter & (2**64 - 1),
                                      float(lo), float(hi), ptr(actions_raw),
                                      ptr(actions_clipped), ptr(logp), _s(mean)))
    return actions_raw, actions_clipped, logp


def policy_sample_dev(mean, log_std, seed, counter_base, counter_offset, lo, hi,
                      actions_raw=None, actions_clipped=None, logp=None):
    """policy_sample with counter = counter_base[0] + counter_offset, the
    base an int64 device tensor (read by the kernel: graph-capturable)."""
    n = mean.shape[0]
    assert counter_base.dtype == torch.int64 and counter_base.device == mean.device
    check(_lib.lib().dr_policy_sample_dev(n, ptr(_f32(mean)), ptr(_f32(log_std)),
                                          seed & (2**64 - 1), ptr(counter_base),
                                          counter_offset & (2**64 - 1), float(lo), float(hi),
                                          ptr(actions_raw), ptr(actions_clipped), ptr(logp),
                                          _s(mean)))
    return actions_raw, actions_clipped, logp


class Permuter:
    """Uniform random permutations of [0, n) (RolloutBuffer.get)."""

    def __init__(self, n: int, device):
        self.n = n
        nbytes = _lib.lib().dr_permutation_workspace_bytes(n)
        self.ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=device)
        self.out = torch.empty(n, dtype=torch.int32, device=device)

    def __call__(self, seed: int, counter: int, out=None):
        o = self.out if out is None else out
        check(_lib.lib().dr_permutation(self.n, seed & (2**64 - 1), counter & (2**64 - 1),
                                        ptr(o), ptr(self.ws), self.ws.numel(), _s(o)))
        return o

    def dev(self, seed: int, counter_base: torch.Tensor, counter_offset: int, out=None):
        """__call__ with counter = counter_base[0] + counter_offset, the base
        an int64 device tensor read by the kernel (graph-capturable)."""
        o = self.out if out is None else out
        assert counter_base.dtype == torch.int64 and counter_base.device == o.device
        check(_lib.lib().dr_permutation_dev(self.n, seed & (2**64 - 1), ptr(counter_base),
                                            counter_offset & (2**64 - 1), ptr(o), ptr(self.ws),
                                            self.ws.numel(), _s(o)))
        return o


def gather_rows(idx, src, out=None):
    """out[k] = src[idx[k]] for a 2-D f32 src (row width = src.shape[1])."""
    src2 = src.reshape(src.shape[0], -1)
    m, w = idx.shape[0], src2.shape[1]
    o = torch.empty(m, w, dtype=torch.float32, device=src.device) if out is None else out
    check(_lib.lib().dr_gather_rows(m, w, ptr(idx), ptr(_f32(src2)), ptr(o), _s(src)))
    return o


def tanh_backward_workspace_bytes(m: int, n: int) -> int:
    return int(_lib.lib().dr_tanh_backward_workspace_bytes(m, n))


def tanh_backward(grad_h, h, grad_z, bias_grad, workspace):
    """grad_z = grad_h * (1 - h^2); bias_grad = grad_z.sum(0) (one pass).
    grad_h / h / grad_z: contiguous (m, n) f32; bias_grad: contiguous (n,)."""
    m, n = h.shape
    for t in (grad_h, h, grad_z):
        assert t.is_contiguous() and t.dtype == torch.float32
    check(_lib.lib().dr_tanh_backward(m, n, ptr(grad_h), ptr(h), ptr(grad_z), ptr(bias_grad),
                                      ptr(workspace), workspace.numel() * workspace.element_size(),
                                      _s(h)))
    return grad_z


class PPOLoss:
    """Fused PPO minibatch loss and its gradient w.r.t. the policy head
    outputs (mean (m,4), log_std (4,), values (m,))."""

    STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "clip_fraction",
             "approx_kl", "adv_mean", "adv_std")

    def __init__(self, m: int, device, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 normalize_advantage=True):
        self.m = m
        self.clip, self.ent, self.vf = clip_range, ent_coef, vf_coef
        self.norm = int(bool(normalize_advantage))
        nbytes = _lib.lib().dr_ppo_loss_workspace_bytes(m)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=device)
        self.grad_mean = torch.empty(m, 4, dtype=torch.float32, device=device)
        self.grad_values = torch.empty(m, dtype=torch.float32, device=device)
        self.grad_log_std = torch.empty(4, dtype=torch.float32, device=device)
        self.stats = torch.empty(8, dtype=torch.float32, device=device)

    def __call__(self, mean, log_std, values, actions, old_logp=None, advantages=None,
                 returns=None, aux=None):
        """Either old_logp / advantages / returns as three (m,) arrays, or
        aux = one contiguous (m,3) array of (old_logp, advantage, return)
        rows (read in place with stride 3)."""
        m = mean.shape[0]
        assert m == self.m
        if aux is not None:
            assert aux.shape == (m, 3)
            base = _f32(aux)
            p_lp, p_adv, p_ret = ptr(base), ptr(base) + 4, ptr(base) + 8
            stride = 3
        else:
            p_lp, p_adv, p_ret = ptr(_f32(old_logp)), ptr(_f32(advantages)), ptr(_f32(returns))
            stride = 1
        check(_lib.lib().dr_ppo_loss(
            m, ptr(_f32(mean)), ptr(_f32(log_std)), ptr(_f32(values)), ptr(_f32(actions)),
            p_lp, p_adv, p_ret, stride,
            float(self.clip), float(self.ent), float(self.vf), self.norm,
            ptr(self.grad_mean), ptr(self.grad_values), ptr(self.grad_log_std),
            ptr(self.stats), ptr(self.ws), self.ws.numel(), _s(mean)))
        return self.grad_mean, self.grad_log_std, self.grad_values, self.stats


class ClipAdam:
    """clip_grad_norm_(max_norm) + torch.optim.Adam over one flat f32 buffer."""

    def __init__(self, params: torch.Tensor, lr=3e-4, betas=(0.9, 0.999), eps=1e-5,
                 max_grad_norm=0.5):
        self.p = params
        self.m = torch.zeros_like(params)
        self.v = torch.zeros_like(params)
        self.lr, self.b1, self.b2, self.eps = lr, betas[0], betas[1], eps
        self.max_norm = max_grad_norm
        self._t, self._t_pending = 0, None
        n = params.numel()
        self.ws = torch.empty(_lib.lib().dr_adam_workspace_bytes(n), dtype=torch.uint8,
                              device=params.device)
        self.grad_norm = torch.zeros(1, dtype=torch.float32, device=params.device)

    @property
    def t(self) -> int:
        """Adam's step count.  Behind a KL gate the steps an iteration took
        are known on the device only; the trainer leaves a callable that
        fetches them, called here the first time the count is needed."""
        if self._t_pending is not None:
            fetch, self._t_pending = self._t_pending, None
            self._t += int(fetch())
        return self._t

    @t.setter
    def t(self, value: int):
        self._t_pending = None
        self._t = int(value)

    def defer_steps(self, fetch):
        """Advance t by fetch() when t is next read (see t)."""
        self.t                      # settle an earlier one first
        self._t_pending = fetch

    def _finish_ws(self, finish: "GradFinish"):
        f = ctypes.byref(finish.desc)
        need = _lib.lib().dr_grad_finish_workspace_bytes(f)
        if finish.ws is None or finish.ws.numel() < need:
            finish.ws = torch.empty(need, dtype=torch.uint8, device=self.p.device)
        return f

    def step_kl(self, grads: torch.Tensor, ctl: "KLControl", j: int, kl: torch.Tensor,
                sched: torch.Tensor):
        """step_sched at grad_scale 1 behind the KL gate (dr_clip_adam_kl):
        optimizer step j of ctl's iteration, `kl` this step's approx_kl (one
        f32 on the device), `sched` the iteration's whole (steps, 2) table.
        Graph-capturable; advances nothing on the host."""
        g = ctl.gate(j, kl, sched)
        check(_lib.lib().dr_clip_adam_kl(
            self.p.numel(), ptr(self.p), ptr(_f32(grads)), ptr(self.m), ptr(self.v),
            float(self.b1), float(self.b2), float(self.eps), float(self.max_norm),
            ctypes.byref(g), ptr(self.grad_norm), ptr(self.ws), self.ws.numel(), _s(self.p)))
        return self.grad_norm

    def step_finish_kl(self, grads: torch.Tensor, finish: "GradFinish", ctl: "KLControl",
                       j: int, kl: torch.Tensor, sched: torch.Tensor):
        """step_finish_sched behind the KL gate (dr_grad_finish_clip_adam_kl);
        arguments as step_kl."""
        f = self._finish_ws(finish)
        g = ctl.gate(j, kl, sched)
        check(_lib.lib().dr_grad_finish_clip_adam_kl(
            f, self.p.numel(), ptr(self.p), ptr(_f32(grads)), ptr(self.m), ptr(self.v),
            float(self.b1), float(self.b2), float(self.eps), float(self.max_norm),
            ctypes.byref(g), ptr(self.grad_norm), ptr(finish.ws), finish.ws.numel(),
            _s(self.p)))
        return self.grad_norm

    def step_finish(self, grads: torch.Tensor, finish: "GradFinish", lr=None):
        """step() for a gradient whose last reductions were deferred
        (dr_grad_finish_clip_adam: the finish and the norm in one launch,
        then clip + Adam)."""
        self.t += 1
        L = _lib.lib()
        f = ctypes.byref(finish.desc)
        need = L.dr_grad_finish_workspace_bytes(f)
        if finish.ws is None or finish.ws.numel() < need:
            finish.ws = torch.empty(need, dtype=torch.uint8, device=self.p.device)
        check(L.dr_grad_finish_clip_adam(
            f, self.p.numel(), ptr(self.p), ptr(_f32(grads)), ptr(self.m), ptr(self.v),
            float(self.lr if lr is None else lr), float(self.b1), float(self.b2),
            float(self.eps), float(self.max_norm), self.t, ptr(self.grad_norm),
            ptr(finish.ws), finish.ws.numel(), _s(self.p)))
        return self.grad_norm

    def schedule(self, first_step: int, count: int, out: torch.Tensor | None = None, lr=None):
        """(count, 2) f32 of Adam's step-dependent scalars for steps
        first_step .. first_step + count - 1 (dr_adam_schedule, host), at
        `lr` when given (the adaptive KL gate's table is built at 1)."""
        L = _lib.lib()
        buf = (ctypes.c_float * (2 * count))()
        lr = self.lr if lr is None else lr
        for j in range(count):
            check(L.dr_adam_schedule(float(lr), float(self.b1), float(self.b2),
                                     first_step + j, ctypes.byref(buf, 8 * j)))
        t = torch.frombuffer(bytearray(buf), dtype=torch.float32).view(count, 2)
        if out is None:
            return t
        out.copy_(t)
        return out

    def step_finish_sched(self, grads: torch.Tensor, finish: "GradFinish", sched: torch.Tensor):
        """step_finish with this step's scalars read on the device from
        `sched` (2 f32, from schedule()); advances nothing on the host (the
        caller owns the step count: graph replays)."""
        L = _lib.lib()
        f = ctypes.byref(finish.desc)
        need = L.dr_grad_finish_workspace_bytes(f)
        if finish.ws is None or finish.ws.numel() < need:
            finish.ws = torch.empty(need, dtype=torch.uint8, device=self.p.device)
        check(L.dr_grad_finish_clip_adam_sched(
            f, self.p.numel(), ptr(self.p), ptr(_f32(grads)), ptr(self.m), ptr(self.v),
            float(self.lr), float(self.b1), float(self.b2), float(self.eps),
            float(self.max_norm), ptr(sched), ptr(self.grad_norm), ptr(finish.ws),
            finish.ws.numel(), _s(self.p)))
        return self.grad_norm

    def step_sched(self, grads: torch.Tensor, sched: torch.Tensor, grad_scale: float = 1.0):
        """clip_grad_norm_ + Adam on grad_scale * grads (1 / world after a
        summing all-reduce) with this step's scalars read on the device
        from `sched` (dr_clip_adam_sched; graph-capturable, advances nothing
        on the host).  After dr_grad_finish_run at grad_scale 1 this is
        bitwise step_finish_sched."""
        check(_lib.lib().dr_clip_adam_sched(
            self.p.numel(), ptr(self.p), ptr(_f32(grads)), ptr(self.m), ptr(self.v),
            float(self.b1), float(self.b2), float(self.eps), float(self.max_norm),
            float(grad_scale), ptr(sched), ptr(self.grad_norm), ptr(self.ws), self.ws.numel(),
            _s(self.p)))
        return self.grad_norm

    def step(self, grads: torch.Tensor, lr=None):
        self.t += 1
        check(_lib.lib().dr_clip_adam(
            self.p.numel(), ptr(self.p), ptr(_f32(grads)), ptr(self.m), ptr(self.v),
            float(self.lr if lr is None else lr), float(self.b1), float(self.b2),
            float(self.eps), float(self.max_norm), self.t, ptr(self.grad_norm),
            ptr(self.ws), self.ws.numel(), _s(self.p)))
        return self.grad_norm


LR_SCHEDULES = ("constant", "linear", "adaptive")


def _f32_round(x: float) -> float:
    """x rounded to f32, as a Python float."""
    import struct
    try:
        return struct.unpack("f", struct.pack("f", float(x)))[0]
    except OverflowError:
        return float("inf") if x > 0 else float("-inf")


def check_kl_control(target_kl, lr_schedule, desired_kl, lr_min, lr_max):
    """The value rules of the KL-control settings, raised as ValueError on the
    host before any device work."""
    import math

    def positive(v):
        return isinstance(v, (int, float)) and not isinstance(v, bool) and \
            math.isfinite(v) and v > 0

    if target_kl is not None:
        if not positive(target_kl):
            raise ValueError(f"target_kl must be None or > 0 and finite, got {target_kl!r}")
        if 1.5 * target_kl > 3.0e38 or _f32_round(1.5 * target_kl) <= 0.0:
            raise ValueError(f"target_kl: 1.5 * target_kl must fit f32, got {target_kl!r}")
    if lr_schedule not in LR_SCHEDULES:
        raise ValueError(f"unknown lr_schedule {lr_schedule!r}: one of {LR_SCHEDULES}")
    if not positive(desired_kl) or _f32_round(desired_kl / 2) <= 0.0 or 2 * desired_kl > 3.0e38:
        raise ValueError(f"desired_kl must be > 0 and finite, got {desired_kl!r}")
    for name, v in (("lr_min", lr_min), ("lr_max", lr_max)):
        if not positive(v) or _f32_round(v) <= 0.0 or v > 3.0e38:
            raise ValueError(f"{name} must be > 0 and finite, got {v!r}")
    if lr_min > lr_max:
        raise ValueError(f"lr_min must be <= lr_max, got {lr_min!r} > {lr_max!r}")


class KLControl:
    """The control block of the KL gate (dr_kl_gate):
    `steps` + 1 slots of (stopped u32, taken u32, lr f32, pad) on the device.
    Optimizer step j of an iteration reads slot j and writes slot j + 1; slot
    0 keeps stopped = taken = 0 and gets the iteration's learning rate --
    from the host (set_lr), or with `adaptive` from the last slot of the
    iteration before, copied on the device by begin() (capturable)."""

    def __init__(self, steps: int, device, target_kl=None, adaptive=False, desired_kl=0.01,
                 lr_min=1e-6, lr_max=1e-2, lr=3e-4):
        check_kl_control(target_kl, "adaptive" if adaptive else "constant", desired_kl, lr_min,
                         lr_max)
        if steps < 1:
            raise ValueError("KLControl needs steps >= 1")
        self.steps, self.adaptive = int(steps), bool(adaptive)
        self.target_kl = None if target_kl is None else float(target_kl)
        # f32(1.5 * target_kl): the product in double, one rounding
        self.stop_kl = 0.0 if target_kl is None else _f32_round(1.5 * target_kl)
        self.desired_kl = float(desired_kl)
        self.kl_high, self.kl_low = _f32_round(2 * desired_kl), _f32_round(desired_kl / 2)
        self.lr_min, self.lr_max = _f32_round(lr_min), _f32_round(lr_max)
        self.slots = torch.zeros(self.steps + 1, 4, dtype=torch.int32, device=device)
        self._lr = self.slots.view(torch.float32)[:, 2]
        self.set_lr(lr, carry=True)

    def set_lr(self, lr: float, carry=False):
        """Slot 0's learning rate from the host; with `carry` also the last
        slot's, which an adaptive begin() copies into slot 0."""
        self._lr[0].fill_(float(lr))
        if carry:
            self._lr[self.steps].fill_(float(lr))

    def begin(self):
        """Start of an iteration, on the device: adaptive carries the rate the
        last iteration ended at."""
        if self.adaptive:
            self._lr[0:1].copy_(self._lr[self.steps:self.steps + 1])

    def gate(self, j: int, kl: torch.Tensor, sched: torch.Tensor) -> "_lib.dr_kl_gate":
        assert 0 <= j < self.steps and tuple(sched.shape) == (self.steps, 2)
        assert kl.numel() == 1 and _f32(sched).device == kl.device == self.slots.device
        assert kl.dtype == torch.float32
        return _lib.dr_kl_gate(control=ptr(self.slots), num_steps=self.steps, step=j,
                               kl=ptr(kl), sched=ptr(sched), stop_kl=self.stop_kl,
                               adaptive=int(self.adaptive), kl_high=self.kl_high,
                               kl_low=self.kl_low, lr_min=self.lr_min, lr_max=self.lr_max)

    def applied_mask(self) -> torch.Tensor:
        """(steps,) bool on the device: the steps that ran before the stop,
        the tripping one included (slot j not yet stopped)."""
        return self.slots[:self.steps, 0] == 0

    def final(self) -> torch.Tensor:
        """The last slot's (taken, lr) as two int32 words on the device."""
        return self.slots[self.steps, 1:3]


LINEAR_TANH_K = (4, 8, 12, 15, 16, 18, 19, 24, 32)


def _rows(rows):
    if rows is None:
        return None
    assert rows.dtype == torch.int32 and rows.is_contiguous()
    return ptr(rows)


def linear_tanh(x, w, b, out, rows=None):
    """out = tanh(x w^T + b) for a narrow input x (., k), k in LINEAR_TANH_K;
    row r of the input is x[rows[r]] when rows (int32) is given."""
    k = x.shape[1]
    m = out.shape[0]
    n = w.shape[0]
    check(_lib.lib().dr_linear_tanh(m, k, n, ptr(_f32(x)), _rows(rows), ptr(_f32(w)),
                                    ptr(_f32(b)), ptr(out), _s(x)))
    return out


def linear_tanh2(x, w0, b0, h0, w1, b1, h1, rows=None):
    """linear_tanh for both MLPs (pi: w0/b0 -> h0, vf: w1/b1 -> h1) over the
    same input rows, one launch."""
    k = x.shape[1]
    m, n = h0.shape
    assert h1.shape == (m, n) and w0.shape == w1.shape == (n, k)
    check(_lib.lib().dr_linear_tanh2(m, k, n, ptr(_f32(x)), _rows(rows), ptr(_f32(w0)),
                                     ptr(_f32(b0)), ptr(h0), ptr(_f32(w1)), ptr(_f32(b1)),
                                     ptr(h1), _s(x)))
    return h0, h1


def linear_tanh2_x6(x, w0, b0, h0, w1, b1, h1, w256, img, ximg=None, rows=None):
    """linear_tanh2 (k 15, n 256) with the 256 x 256 layer's x6 weight images
    (both forms, from w256 (2, 256, 256)) into img and, with ximg, the
    observation image of dr_gemm_x6_bwd_first built in the same launch."""
    k = x.shape[1]
    m, n = h0.shape
    assert h1.shape == (m, n) and w0.shape == w1.shape == (n, k)
    assert w256.shape == (2, 256, 256) and w256.is_contiguous()
    check(_lib.lib().dr_linear_tanh2_x6(m, k, n, ptr(_f32(x)), _rows(rows), ptr(_f32(w0)),
                                        ptr(_f32(b0)), ptr(h0), ptr(_f32(w1)), ptr(_f32(b1)),
                                        ptr(h1), ptr(w256), ptr(img), ptr(ximg), _s(x)))
    return h0, h1


def gather_minibatch(idx, obs, actions, aux, obs_out, actions_out, aux_out, adv_part=None):
    """obs_out / actions_out / aux_out = rows idx of obs (., d) / actions
    (., 4) / aux (., 3), one launch; with adv_part (a HeadLossBackward's
    `adv_part`) also the advantage partials its normalisation needs."""
    m = idx.numel()
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert obs_out.shape == (m, obs.shape[1]) and actions_out.shape == (m, 4)
    assert aux_out.shape == (m, 3) and actions.shape[1] == 4 and aux.shape[1] == 3
    check(_lib.lib().dr_gather_minibatch(m, ptr(idx), obs.shape[1], ptr(_f32(obs)),
                                         ptr(_f32(actions)), ptr(_f32(aux)), ptr(obs_out),
                                         ptr(actions_out), ptr(aux_out), ptr(adv_part),
                                         _s(obs)))


RECORD_FLOATS = 32      # DR_RECORD_FLOATS: one 128-B rollout record


def pack_rollout_records(obs, actions, logp, adv, ret, records):
    """records (n, 32) f32: rollout row r as one 128-B record (obs, action,
    old log-prob, advantage, return; dr_pack_rollout_records), for
    gather_records."""
    n, d = obs.shape
    assert actions.shape == (n, 4) and records.shape == (n, RECORD_FLOATS)
    assert logp.numel() == adv.numel() == ret.numel() == n and records.is_contiguous()
    check(_lib.lib().dr_pack_rollout_records(n, d, ptr(_f32(obs)), ptr(_f32(actions)),
                                             ptr(_f32(logp)), ptr(_f32(adv)), ptr(_f32(ret)),
                                             ptr(records), _s(obs)))


def gather_records(idx, records, obs_dim, obs_out, actions_out, aux_out, adv_part=None):
    """gather_minibatch's outputs (the same bytes) from the packed records:
    one cache line per gathered row."""
    m = idx.numel()
    assert idx.dtype == torch.int32 and idx.is_contiguous()
    assert records.shape[1] == RECORD_FLOATS and records.is_contiguous()
    assert obs_out.shape == (m, obs_dim) and actions_out.shape == (m, 4)
    assert aux_out.shape == (m, 3)
    check(_lib.lib().dr_gather_records(m, ptr(idx), obs_dim, ptr(records), ptr(obs_out),
                                       ptr(actions_out), ptr(aux_out), ptr(adv_part),
                                       _s(records)))


def policy_heads(h_pi, h_vf, w_act, b_act, w_val, b_val, mean, value, preact=False,
                 zb_pi=None, zb_vf=None):
    """mean (m,4) = h_pi w_act^T + b_act, value (m) = h_vf w_val^T + b_val;
    with preact the inputs are pre-activations and tanh(z + zb) is applied
    on load (zb_pi / zb_vf: the top layer's biases, when its GEMM left them
    out)."""
    m, hd = h_pi.shape
    check(_lib.lib().dr_policy_heads(m, hd, int(bool(preact)), ptr(_f32(h_pi)), ptr(_f32(h_vf)),
                                     ptr(zb_pi), ptr(zb_vf), ptr(_f32(w_act)),
                                     ptr(_f32(b_act)), ptr(_f32(w_val)), ptr(_f32(b_val)),
                                     ptr(mean), ptr(value), _s(h_pi)))
    return mean, value


class HeadLossBackward:
    """dr_ppo_head_loss_backward: heads + PPO loss + backward through the
    heads and the top tanh of both MLPs, one minibatch of m rows."""

    def __init__(self, m: int, hd: int, device, clip_range=0.2, ent_coef=0.0, vf_coef=0.5,
                 normalize_advantage=True):
        self.m, self.hd = m, hd
        self.clip, self.ent, self.vf = clip_range, ent_coef, vf_coef
        self.norm = int(bool(normalize_advantage))
        self.ws = torch.empty(_lib.lib().dr_ppo_head_workspace_bytes(m, hd), dtype=torch.uint8,
                              device=device)
        self.stats = torch.empty(8, dtype=torch.float32, device=device)

    @property
    def adv_part(self):
        """Where gather_minibatch writes the advantage partials (the head of
        the workspace) for a call with adv_ready=True."""
        return self.ws

    def __call__(self, h_pi, h_vf, w_act, b_act, w_val, b_val, log_std, actions, aux,
                 gz_pi, gz_vf, g_w_act, g_b_act, g_w_val, g_b_val, g_b_pi, g_b_vf, g_log_std,
                 rows=None, preact=False, adv_ready=False, stats_out=None, zb_pi=None,
                 zb_vf=None, defer=False):
        """actions (.,4) / aux (.,3) rows are read as [rows[r]] when rows
        (int32, m) is given, else the first m rows; with preact h_pi / h_vf
        are the top layer's pre-activations (tanh applied on load).  With
        adv_ready the advantage partials were written by gather_minibatch
        (adv_part=self.adv_part) for this minibatch; stats_out (8 f32)
        receives the stats instead of self.stats; zb_pi / zb_vf as
        policy_heads.  With defer the gradient / stats outputs are written
        later by ClipAdam.step_finish (GradFinish); defer=2 leaves the
        per-block rows unreduced for a finish with head_direct = 1."""
        assert h_pi.shape == (self.m, self.hd) and aux.shape[1] == 3
        assert rows is not None or aux.shape[0] == self.m
        stats = self.stats if stats_out is None else stats_out
        assert stats.numel() == 8 and stats.dtype == torch.float32 and stats.is_contiguous()
        norm = 2 if (self.norm and adv_ready) else self.norm
        check(_lib.lib().dr_ppo_head_loss_backward(
            self.m, self.hd, int(bool(preact)), ptr(_f32(h_pi)), ptr(_f32(h_vf)), ptr(zb_pi),
            ptr(zb_vf), ptr(_f32(w_act)),
            ptr(_f32(b_act)), ptr(_f32(w_val)), ptr(_f32(b_val)), ptr(_f32(log_std)),
            ptr(_f32(actions)), ptr(_f32(aux)), _rows(rows), float(self.clip), float(self.ent),
            float(self.vf), norm, ptr(gz_pi), ptr(gz_vf), ptr(g_w_act), ptr(g_b_act),
            ptr(g_w_val), ptr(g_b_val), ptr(g_b_pi), ptr(g_b_vf), ptr(g_log_std),
            ptr(stats), int(defer), ptr(self.ws), self.ws.numel(), _s(h_pi)))
        return stats


class FirstLayerBackward:
    """dr_first_layer_backward: grad_w (n,k), grad_b (n) of h = tanh(x W^T + b)
    from grad_h, without materialising grad_z."""

    def __init__(self, m: int, k: int, n: int, device):
        self.m, self.k, self.n = m, k, n
        self.ws = torch.empty(_lib.lib().dr_first_layer_backward_workspace_bytes(m, k, n),
                              dtype=torch.uint8, device=device)

    def __call__(self, grad_h, h, x, grad_w, grad_b, rows=None):
        assert grad_h.shape == (self.m, self.n) and x.shape[1] == self.k
        assert rows is not None or x.shape[0] == self.m
        check(_lib.lib().dr_first_layer_backward(
            self.m, self.k, self.n, ptr(_f32(grad_h)), ptr(_f32(h)), ptr(_f32(x)), _rows(rows),
            ptr(grad_w), ptr(grad_b), ptr(self.ws), self.ws.numel(), _s(h)))


class FirstLayerBackward2:
    """dr_first_layer_backward2: FirstLayerBackward for both MLPs over the
    same input in one launch (bitwise the same as two single calls)."""

    def __init__(self, m: int, k: int, n: int, device):
        self.m, self.k, self.n = m, k, n
        self.ws = torch.empty(_lib.lib().dr_first_layer_backward2_workspace_bytes(m, k, n),
                              dtype=torch.uint8, device=device)

    def __call__(self, x, grad_h0, h0, grad_w0, grad_b0, grad_h1, h1, grad_w1, grad_b1,
                 rows=None, defer=False):
        for g, h in ((grad_h0, h0), (grad_h1, h1)):
            assert g.shape == (self.m, self.n) and h.shape == (self.m, self.n)
        assert x.shape[1] == self.k and (rows is not None or x.shape[0] == self.m)
        check(_lib.lib().dr_first_layer_backward2(
            self.m, self.k, self.n, ptr(_f32(x)), _rows(rows), ptr(_f32(grad_h0)), ptr(_f32(h0)),
            ptr(grad_w0), ptr(grad_b0), ptr(_f32(grad_h1)), ptr(_f32(h1)), ptr(grad_w1),
            ptr(grad_b1), int(bool(defer)), ptr(self.ws), self.ws.numel(), _s(x)))


class GradFinish:
    """The deferred reductions of one fused minibatch step (the
    dr_grad_finish descriptor: head / first-layer partials, split-K chunks),
    consumed by ClipAdam.step_finish.  `desc` holds raw device pointers: the
    tensors it points into must stay alive (FusedTrainStep owns them)."""

    def __init__(self):
        self.desc = _lib.dr_grad_finish()
        self.ws = None

    def _workspace(self, device):
        need = _lib.lib().dr_grad_finish_workspace_bytes(ctypes.byref(self.desc))
        if self.ws is None or self.ws.numel() < need:
            self.ws = torch.empty(need, dtype=torch.uint8, device=device)
        return self.ws

    def run(self, device):
        """dr_grad_finish_run: every deferred partial reduced into the flat
        gradient (and the loss stats) on the current stream -- the
        data-parallel step's finish, ahead of the gradient all-reduce."""
        ws = self._workspace(device)
        check(_lib.lib().dr_grad_finish_run(ctypes.byref(self.desc), ptr(ws), ws.numel(),
                                            torch.cuda.current_stream(device).cuda_stream))


def check_vecnorm(clip_obs, clip_reward, epsilon, gamma=0.99):
    """The value rules of dr_vecnorm_step, raised as ValueError on the host."""
    import math
    for name, v in (("clip_obs", clip_obs), ("clip_reward", clip_reward)):
        if not (isinstance(v, (int, float)) and math.isfinite(v) and v > 0):
            raise ValueError(f"{name} must be > 0 and finite, got {v!r}")
    if not (isinstance(epsilon, (int, float)) and math.isfinite(epsilon) and epsilon >= 0):
        raise ValueError(f"epsilon must be >= 0 and finite, got {epsilon!r}")
    if not (isinstance(gamma, (int, float)) and math.isfinite(gamma)):
        raise ValueError(f"gamma must be finite, got {gamma!r}")


class VecNormalize:
    """stable-baselines3's VecNormalize on device tensors (dr_vecnorm_*,
    DESIGN.md section 21): running f64 statistics of the observations and of
    the discounted returns, advanced and applied by at most three launches per
    step with no host round trip, so a captured rollout can hold it.

    State: obs_rms f64 (1 + 2 D,) = count, mean, var; ret_rms f64 (3,);
    returns f64 (n,).  `training` False freezes the statistics (evaluation)."""

    NPZ_KEYS = ("obs_count", "obs_mean", "obs_var", "ret_count", "ret_mean", "ret_var",
                "clip_obs", "clip_reward", "gamma", "epsilon")

    def __init__(self, n: int, obs_dim: int, device, gamma=0.99, clip_obs=10.0, clip_reward=10.0,
                 epsilon=1e-8, norm_obs=True, norm_reward=True):
        check_vecnorm(clip_obs, clip_reward, epsilon, gamma)
        if n < 1 or not 1 <= obs_dim <= 24:
            raise ValueError("VecNormalize needs n >= 1 and 1 <= obs_dim <= 24")
        self.n, self.obs_dim, self.device = int(n), int(obs_dim), torch.device(device)
        self.gamma, self.clip_obs, self.clip_reward = float(gamma), float(clip_obs), \
            float(clip_reward)
        self.epsilon = float(epsilon)
        self.norm_obs, self.norm_reward = bool(norm_obs), bool(norm_reward)
        self.training = True
        f64 = dict(dtype=torch.float64, device=self.device)
        self.obs_rms = torch.empty(1 + 2 * self.obs_dim, **f64)
        self.ret_rms = torch.empty(3, **f64)
        self.returns = torch.empty(self.n, **f64)
        nbytes = _lib.lib().dr_vecnorm_workspace_bytes(self.n, self.obs_dim)
        self.ws = torch.empty(max(nbytes // 8, 1), **f64)
        check(_lib.lib().dr_vecnorm_init(self.n, self.obs_dim, ptr(self.obs_rms),
                                         ptr(self.ret_rms), ptr(self.returns),
                                         _s(self.obs_rms)))

    # views of the statistics (device tensors, no copy)
    @property
    def obs_count(self):
        return self.obs_rms[0]

    @property
    def obs_mean(self):
        return self.obs_rms[1:1 + self.obs_dim]

    @property
    def obs_var(self):
        return self.obs_rms[1 + self.obs_dim:]

    def flags(self) -> int:
        return ((_lib.DR_VECNORM_OBS if self.norm_obs else 0) |
                (_lib.DR_VECNORM_REWARD if self.norm_reward else 0) |
                (_lib.DR_VECNORM_TRAINING if self.training else 0))

    def _rows(self, t, what):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), \
            f"{what}: expected a contiguous f32 device tensor"
        assert t.dim() == 2 and t.shape[1] == self.obs_dim, f"{what}: expected (rows, obs_dim)"
        return t

    def _step(self, obs, rew, done, term_obs, obs_out, rew_out, term_out):
        check(_lib.lib().dr_vecnorm_step(
            self.n, self.obs_dim, ptr(obs), ptr(rew), ptr(done), ptr(term_obs), self.flags(),
            self.gamma, self.clip_obs, self.clip_reward, self.epsilon, ptr(self.obs_rms),
            ptr(self.ret_rms), ptr(self.returns), ptr(obs_out), ptr(rew_out), ptr(term_out),
            ptr(self.ws), self.ws.numel() * 8, _s(obs)))

    def reset(self, obs, out=None):
        """VecNormalize.reset on the raw reset observations (n, obs_dim):
        returns <- 0, the statistics advance (training), out = normalised."""
        assert self._rows(obs, "obs").shape[0] == self.n
        o = torch.empty_like(obs) if out is None else self._rows(out, "out")
        assert o.shape == obs.shape
        self._step(obs, None, None, None, o, None, None)
        return o

    def step(self, obs, rew, done, term_obs=None, obs_out=None, rew_out=None, term_out=None):
        """VecNormalize.step_wait on one raw env step: obs (n, obs_dim) f32,
        rew (n,) f32, done (n,) u8, term_obs (n, obs_dim) f32 whose rows of
        done envs hold the terminal observations.  Outputs may alias their
        inputs.  Returns (obs_out, rew_out) or, with term_obs, also term_out
        (rows of envs that are not done are left as they were)."""
        assert self._rows(obs, "obs").shape[0] == self.n
        assert rew.dtype == torch.float32 and rew.is_contiguous() and rew.shape == (self.n,)
        assert done.dtype == torch.uint8 and done.is_contiguous() and done.shape == (self.n,)
        o = torch.empty_like(obs) if obs_out is None else self._rows(obs_out, "obs_out")
        r = torch.empty_like(rew) if rew_out is None else rew_out
        assert o.shape == obs.shape and r.shape == rew.shape and r.dtype == torch.float32 \
            and r.is_contiguous()
        if term_obs is None:
            assert term_out is None, "term_out needs term_obs"
            self._step(obs, rew, done, None, o, r, None)
            return o, r
        assert self._rows(term_obs, "term_obs").shape == obs.shape
        to = torch.empty_like(term_obs) if term_out is None else self._rows(term_out, "term_out")
        assert to.shape == obs.shape
        self._step(obs, rew, done, term_obs, o, r, to)
        return o, r, to

    def normalize_obs(self, obs, out=None):
        """Normalise m rows (any m) with the statistics as they are (a copy
        when norm_obs is off)."""
        self._rows(obs, "obs")
        o = torch.empty_like(obs) if out is None else self._rows(out, "out")
        assert o.shape == obs.shape
        if not self.norm_obs:
            if o.data_ptr() != obs.data_ptr():
                o.copy_(obs)
            return o
        check(_lib.lib().dr_vecnorm_apply(obs.shape[0], self.obs_dim, ptr(obs), ptr(self.obs_rms),
                                          self.clip_obs, self.epsilon, ptr(o), _s(obs)))
        return o

    def unnormalize_obs(self, obs, out=None):
        """The inverse of normalize_obs up to the clip."""
        self._rows(obs, "obs")
        o = torch.empty_like(obs) if out is None else self._rows(out, "out")
        assert o.shape == obs.shape
        if not self.norm_obs:
            if o.data_ptr() != obs.data_ptr():
                o.copy_(obs)
            return o
        check(_lib.lib().dr_vecnorm_unapply(obs.shape[0], self.obs_dim, ptr(obs),
                                            ptr(self.obs_rms), self.epsilon, ptr(o), _s(obs)))
        return o

    # ------------------------------------------------------------ checkpoint
    def state_dict(self):
        return {"obs_rms": self.obs_rms.cpu().clone(), "ret_rms": self.ret_rms.cpu().clone(),
                "returns": self.returns.cpu().clone(), "gamma": self.gamma,
                "clip_obs": self.clip_obs, "clip_reward": self.clip_reward,
                "epsilon": self.epsilon, "norm_obs": self.norm_obs,
                "norm_reward": self.norm_reward, "training": self.training}

    def load_state_dict(self, sd):
        if tuple(sd["obs_rms"].shape) != tuple(self.obs_rms.shape):
            raise ValueError("VecNormalize: the checkpoint's obs_dim differs")
        check_vecnorm(sd["clip_obs"], sd["clip_reward"], sd["epsilon"], sd["gamma"])
        self.obs_rms.copy_(sd["obs_rms"].to(self.device))
        self.ret_rms.copy_(sd["ret_rms"].to(self.device))
        if tuple(sd["returns"].shape) == tuple(self.returns.shape):
            self.returns.copy_(sd["returns"].to(self.device))
        else:                       # another env count: the statistics carry over
            self.returns.zero_()
        self.gamma, self.clip_obs = float(sd["gamma"]), float(sd["clip_obs"])
        self.clip_reward, self.epsilon = float(sd["clip_reward"]), float(sd["epsilon"])
        self.norm_obs, self.norm_reward = bool(sd["norm_obs"]), bool(sd["norm_reward"])
        self.training = bool(sd.get("training", True))

    def npz_dict(self):
        """The statistics and settings as numpy values (NPZ_KEYS)."""
        import numpy as np
        o, r, D = self.obs_rms.cpu().numpy(), self.ret_rms.cpu().numpy(), self.obs_dim
        return {"obs_count": np.float64(o[0]), "obs_mean": o[1:1 + D].copy(),
                "obs_var": o[1 + D:].copy(), "ret_count": np.float64(r[0]),
                "ret_mean": np.float64(r[1]), "ret_var": np.float64(r[2]),
                "clip_obs": np.float64(self.clip_obs), "clip_reward": np.float64(self.clip_reward),
                "gamma": np.float64(self.gamma), "epsilon": np.float64(self.epsilon),
                "norm_obs": np.bool_(self.norm_obs), "norm_reward": np.bool_(self.norm_reward)}

    def load_npz_dict(self, z):
        import numpy as np
        D = self.obs_dim
        mean, var = np.asarray(z["obs_mean"], np.float64), np.asarray(z["obs_var"], np.float64)
        if mean.shape != (D,) or var.shape != (D,):
            raise ValueError("VecNormalize: the file's obs_dim differs")
        check_vecnorm(float(z["clip_obs"]), float(z["clip_reward"]), float(z["epsilon"]),
                      float(z["gamma"]))
        o = np.concatenate([[float(z["obs_count"])], mean, var])
        r = np.array([float(z["ret_count"]), float(z["ret_mean"]), float(z["ret_var"])])
        self.obs_rms.copy_(torch.from_numpy(o).to(self.device))
        self.ret_rms.copy_(torch.from_numpy(r).to(self.device))
        self.returns.zero_()
        self.clip_obs, self.clip_reward = float(z["clip_obs"]), float(z["clip_reward"])
        self.gamma, self.epsilon = float(z["gamma"]), float(z["epsilon"])
        if "norm_obs" in z:
            self.norm_obs, self.norm_reward = bool(z["norm_obs"]), bool(z["norm_reward"])

    def save_npz(self, path):
        """obs / ret count, mean and var, the clips, gamma and epsilon as one
        .npz (how to copy them into an SB3 VecNormalize)."""
        import numpy as np
        np.savez(path, **self.npz_dict())

    def load_npz(self, path):
        import numpy as np
        with np.load(path) as z:
            self.load_npz_dict(z)


# ---------------------------------------------------------------- SensorModel
SENSOR_GROUPS = ("pos", "vel", "att", "rate")
# per variant: the columns of each group (each with draws of its own), and
# (first mirror column, first source column, count): columns that show their
# source's error with the opposite sign (target - p next to p).  Columns in
# neither stay clean.  DESIGN.md section 23
SENSOR_COLUMNS = {
    "gym": ({"pos": range(0, 3), "vel": range(3, 6), "att": range(6, 9), "rate": range(9, 12)},
            (12, 0, 3)),
    "vectorized": ({"pos": range(0, 3), "vel": range(3, 6), "att": range(6, 9),
                    "rate": range(9, 12)}, None),
    "moving": ({"pos": range(0, 3), "vel": range(3, 6), "att": range(6, 9),
                "rate": range(9, 12)}, (12, 0, 3)),
    "smooth": ({"pos": range(0, 3), "vel": range(3, 6), "att": range(6, 9),
                "rate": range(9, 12)}, (12, 0, 3)),
    # the attitude is the quaternion's four components, not renormalised
    "rk4": ({"pos": range(0, 3), "vel": range(3, 6), "att": range(6, 10),
             "rate": range(10, 13)}, (13, 0, 3)),
    # the other drone's relative position and velocity: estimates of their own
    "tag": ({"pos": (0, 1, 2, 12, 13, 14), "vel": (3, 4, 5, 15, 16, 17), "att": range(6, 9),
             "rate": range(9, 12)}, None),
}


def _pair(v, what):
    try:
        lo, hi = v
    except (TypeError, ValueError):
        raise ValueError(f"{what} takes two values (lo, hi), got {v!r}") from None
    return lo, hi


def check_sensor(noise=(0, 0, 0, 0), bias=(0, 0, 0, 0), delay=(0, 0), max_steps=None):
    """The value rules of the sensor model's settings,
    raised as ValueError on the host: four noise stds and four bias
    half-widths (pos, vel, att, rate), each finite and >= 0 in f32; integers
    0 <= lo <= hi <= 15; a step limit below 2^24 where given.  Returns
    (noise4, bias4, (lo, hi)) as floats / ints."""
    import math
    import numpy as np
    out = []
    for name, v in (("obs_noise", noise), ("obs_bias", bias)):
        try:
            v = tuple(v)
        except TypeError:
            raise ValueError(f"{name} takes four values (pos, vel, att, rate), got {v!r}") from None
        if len(v) != 4:
            raise ValueError(f"{name} takes four values (pos, vel, att, rate), got {v!r}")
        for x in v:
            if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x) \
                    or x < 0 or x > float(np.finfo(np.float32).max):
                raise ValueError(f"{name} values must be >= 0 and finite, got {x!r}")
        out.append(tuple(float(x) for x in v))
    lo, hi = _pair(delay, "obs_delay")
    for x in (lo, hi):
        if isinstance(x, bool) or not isinstance(x, int):
            raise ValueError(f"obs_delay takes integers, got {x!r}")
    if not 0 <= lo <= hi <= _lib.DR_SENSOR_MAX_DELAY:
        raise ValueError(f"obs_delay needs 0 <= lo <= hi <= {_lib.DR_SENSOR_MAX_DELAY}, "
                         f"got {(lo, hi)!r}")
    if max_steps is not None and int(max_steps) >= 1 << 24:
        raise ValueError("the sensor model needs max_steps below 2^24")
    return out[0], out[1], (int(lo), int(hi))


def sensor_neutral(noise, bias, delay) -> bool:
    """True when the three settings leave the observation as it is."""
    return not any(noise) and not any(bias) and tuple(delay) == (0, 0)


def sensor_columns(variant: str, noise4, bias4):
    """The per-column (sigma, beta, mirror) lists of a variant from the four
    group values (SENSOR_COLUMNS)."""
    from .env import OBS_DIM
    if variant not in SENSOR_COLUMNS:
        raise ValueError(f"unknown variant {variant!r}")
    noise4, bias4, _ = check_sensor(noise4, bias4)
    groups, mirror = SENSOR_COLUMNS[variant]
    od = OBS_DIM[variant]
    sigma, beta, mir = [0.0] * od, [0.0] * od, [-1] * od
    for g, s, b in zip(SENSOR_GROUPS, noise4, bias4):
        for c in groups[g]:
            sigma[c], beta[c] = s, b
    if mirror is not None:
        first, src, count = mirror
        for k in range(count):
            mir[first + k] = src + k
    return sigma, beta, mir


class SensorModel:
    """Observation noise, bias and latency on device tensors (dr_sensor_*,
    DESIGN.md section 23): obs (n, obs_dim) f32 of the env in, what the policy
    sees out, one launch per reset / step and no host round trip, so a
    captured rollout can hold it.

    `columns` = (sigma, beta, mirror), each obs_dim long (sensor_columns);
    `delay` = (lo, hi): each episode's delay is drawn from [lo, hi] steps.
    State: `state` int32 (3, n) = ep, s, d per env; `bias` f32 (n, obs_dim);
    `ring` f32 (hi + 1, n, obs_dim), the clean observations."""

    def __init__(self, n: int, obs_dim: int, device, columns=None, delay=(0, 0), seed: int = 0,
                 env_id_offset: int = 0):
        if n < 1 or not 1 <= obs_dim <= _lib.DR_SENSOR_MAX_DIM:
            raise ValueError("SensorModel needs n >= 1 and 1 <= obs_dim <= 24")
        self.n, self.obs_dim, self.device = int(n), int(obs_dim), torch.device(device)
        if columns is None:
            columns = ([0.0] * obs_dim, [0.0] * obs_dim, [-1] * obs_dim)
        sigma, beta, mirror = (list(v) for v in columns)
        if not len(sigma) == len(beta) == len(mirror) == self.obs_dim:
            raise ValueError("SensorModel: columns must hold obs_dim values each")
        _, _, (lo, hi) = check_sensor(delay=delay)
        self.sigma, self.beta = [float(x) for x in sigma], [float(x) for x in beta]
        self.mirror = [int(x) for x in mirror]
        self.delay = (lo, hi)
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)
        c = self.cfg = _lib.dr_sensor_config(delay_lo=lo, delay_hi=hi,
                                             seed=self.seed & (2**64 - 1),
                                             env_id_offset=self.env_id_offset)
        for k in range(self.obs_dim):
            c.sigma[k], c.beta[k], c.mirror[k] = self.sigma[k], self.beta[k], self.mirror[k]
        dev = self.device
        self.state = torch.zeros(3, self.n, dtype=torch.int32, device=dev)
        self.bias = torch.zeros(self.n, self.obs_dim, dtype=torch.float32, device=dev)
        self.ring = torch.zeros(hi + 1, self.n, self.obs_dim, dtype=torch.float32, device=dev)

    def flags(self) -> int:
        """1: some column has noise, 2: some has a bias, 4: a delay can occur."""
        return (1 if any(self.sigma) else 0) | (2 if any(self.beta) else 0) | \
            (4 if self.delay[1] else 0)

    def key(self) -> tuple:
        """Every value a captured launch holds as a kernel argument."""
        return (self.flags(), tuple(self.sigma), tuple(self.beta), tuple(self.mirror),
                self.delay, self.seed, self.env_id_offset)

    def _rows(self, t, what):
        assert t.dtype == torch.float32 and t.is_cuda and t.is_contiguous(), \
            f"{what}: expected a contiguous f32 device tensor"
        assert t.shape == (self.n, self.obs_dim), f"{what}: expected (n, obs_dim)"
        return t

    def reset(self, obs, out=None):
        """Every env starts episode 0 on its reset observation; returns what
        the policy sees of it."""
        self._rows(obs, "obs")
        o = torch.empty_like(obs) if out is None else self._rows(out, "out")
        check(_lib.lib().dr_sensor_reset(ctypes.byref(self.cfg), self.n, self.obs_dim, ptr(obs),
                                         ptr(self.state), ptr(self.bias), ptr(self.ring), ptr(o),
                                         _s(obs)))
        return o

    def step(self, obs, dones, term_obs=None, obs_out=None, term_out=None):
        """One env step: obs (n, obs_dim) f32 (of done envs the new episode's
        first observation), dones (n,) u8, term_obs (n, obs_dim) f32 whose
        rows of done envs hold the terminal observations.  Returns obs_out or,
        with term_obs, (obs_out, term_out); rows of term_out of envs that are
        not done are left as they were."""
        self._rows(obs, "obs")
        assert dones.dtype == torch.uint8 and dones.is_contiguous() and dones.shape == (self.n,)
        o = torch.empty_like(obs) if obs_out is None else self._rows(obs_out, "obs_out")
        if term_obs is None:
            assert term_out is None, "term_out needs term_obs"
            to = None
        else:
            self._rows(term_obs, "term_obs")
            to = torch.empty_like(term_obs) if term_out is None else self._rows(term_out,
                                                                                "term_out")
        check(_lib.lib().dr_sensor_step(ctypes.byref(self.cfg), self.n, self.obs_dim, ptr(obs),
                                        ptr(dones), ptr(term_obs), ptr(self.state),
                                        ptr(self.bias), ptr(self.ring), ptr(o), ptr(to), _s(obs)))
        return o if term_obs is None else (o, to)

    # ------------------------------------------------------------ checkpoint
    def state_dict(self):
        return {"sigma": list(self.sigma), "beta": list(self.beta), "mirror": list(self.mirror),
                "delay": list(self.delay), "seed": self.seed,
                "env_id_offset": self.env_id_offset, "state": self.state.cpu().clone(),
                "bias": self.bias.cpu().clone(), "ring": self.ring.cpu().clone()}

    def load_state_dict(self, sd):
        """The per-env state and the ring of a checkpoint with the same
        settings and shapes (the settings are the constructor's)."""
        mine = (self.sigma, self.beta, self.mirror, list(self.delay))
        theirs = ([float(x) for x in sd["sigma"]], [float(x) for x in sd["beta"]],
                  [int(x) for x in sd["mirror"]], [int(x) for x in sd["delay"]])
        if mine != theirs:
            raise ValueError("SensorModel: the checkpoint's settings differ")
        for k in ("state", "bias", "ring"):
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"SensorModel: the checkpoint's {k} has another shape")
            getattr(self, k).copy_(sd[k].to(self.device))
