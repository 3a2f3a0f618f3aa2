"""MPPIPlanner: sampled trajectory planning on the gym env's own physics
(dr_mppi_*).

A controller that is not learned: for every env it flies `samples` perturbed
action sequences `horizon` steps ahead on the device, weights them by
exponentiated return and applies the first action of the weighted mean.  It
plans from the 15-float observation a policy sees, on the nominal airframe in
still air, so it can sit behind wind, an airframe spread or a SensorModel
unchanged.  One launch per plan step and no host round trip: a captured
(env step -> plan) loop holds it.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import check, ptr

OBS_DIM = 15
SAMPLES = (64, 128, 256, 512, 1024)


def _s(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def check_mppi(samples=256, horizon=16, sigma=0.3, temperature=0.05, gamma=1.0, crash_cost=10.0,
               terminal_weight=1.0) -> None:
    """The value rules of the planner's settings, raised
    as ValueError on the host, each message naming its argument."""
    def real(x):
        return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)
    if isinstance(samples, bool) or not isinstance(samples, int) or samples not in SAMPLES:
        raise ValueError(f"samples must be one of {SAMPLES}, got {samples!r}")
    if isinstance(horizon, bool) or not isinstance(horizon, int) or \
            not 1 <= horizon <= _lib.DR_MPPI_MAX_HORIZON:
        raise ValueError(f"horizon must be an integer in [1, {_lib.DR_MPPI_MAX_HORIZON}], "
                         f"got {horizon!r}")
    if not real(sigma) or sigma < 0:
        raise ValueError(f"sigma must be >= 0 and finite, got {sigma!r}")
    if not real(temperature) or temperature <= 0:
        raise ValueError(f"temperature must be > 0 and finite, got {temperature!r}")
    if not real(gamma) or not 0 < gamma <= 1:
        raise ValueError(f"gamma must be in (0, 1], got {gamma!r}")
    if not real(crash_cost) or crash_cost < 0:
        raise ValueError(f"crash_cost must be >= 0 and finite, got {crash_cost!r}")
    if not real(terminal_weight) or terminal_weight < 0:
        raise ValueError(f"terminal_weight must be >= 0 and finite, got {terminal_weight!r}")


class MPPIPlanner:
    """Model-predictive path integral control for `n` gym envs on device
    tensors.  State: `nominal` f32 (n, horizon, 4), the warm start, and `calls`
    (n,) int32 holding the u32 count of plan steps since the reset."""

    SETTINGS = ("samples", "horizon", "sigma", "temperature", "gamma", "crash_cost",
                "terminal_weight", "seed", "env_id_offset")

    def __init__(self, n, device, samples=256, horizon=16, sigma=0.3, temperature=0.05,
                 gamma=1.0, crash_cost=10.0, terminal_weight=1.0, seed=0, env_id_offset=0):
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"MPPIPlanner needs n >= 1, got {n!r}")
        check_mppi(samples, horizon, sigma, temperature, gamma, crash_cost, terminal_weight)
        self.n, self.device = n, torch.device(device)
        self.samples, self.horizon = samples, horizon
        self.sigma, self.temperature, self.gamma = float(sigma), float(temperature), float(gamma)
        self.crash_cost, self.terminal_weight = float(crash_cost), float(terminal_weight)
        self.seed, self.env_id_offset = int(seed), int(env_id_offset)
        self.cfg = _lib.dr_mppi_config(
            samples=samples, horizon=horizon, sigma=self.sigma, temperature=self.temperature,
            gamma=self.gamma, crash_cost=self.crash_cost, terminal_weight=self.terminal_weight,
            seed=self.seed & (2**64 - 1), env_id_offset=self.env_id_offset)
        self.nominal = torch.empty(n, horizon, 4, dtype=torch.float32, device=self.device)
        self.calls = torch.empty(n, dtype=torch.int32, device=self.device)
        self.reset()

    def key(self) -> tuple:
        """Every value a captured launch holds as a kernel argument."""
        return tuple(getattr(self, k) for k in self.SETTINGS)

    def reset(self):
        """Every env's nominal back to hover thrust, every call count to 0."""
        check(_lib.lib().dr_mppi_reset(ctypes.byref(self.cfg), self.n, ptr(self.nominal),
                                       ptr(self.calls), _s(self.nominal)))

    def _out(self, t, shape, dtype, what):
        if t.dtype != dtype or t.device != self.nominal.device or not t.is_contiguous() \
                or tuple(t.shape) != shape:
            raise ValueError(f"{what}: expected a contiguous {dtype} device tensor of shape "
                             f"{shape}, got {t.dtype} {tuple(t.shape)}")
        return t

    def plan(self, obs, dones=None, out=None, costs_out=None):
        """One plan step: obs (n, 15) f32 as the env (or a SensorModel) delivers
        it; dones (n,) u8, optional: a set flag says obs[i] opens a new episode,
        so env i plans from hover.  Returns the actions (n, 4) f32 (`out` if
        given); costs_out (n, samples) f64 receives every sample's return."""
        if obs.dim() != 2 or obs.shape[1] != OBS_DIM:
            raise ValueError(f"MPPIPlanner plans on the 15-float observation (gym variant only), "
                             f"got obs of shape {tuple(obs.shape)}")
        self._out(obs, (self.n, OBS_DIM), torch.float32, "obs")
        if dones is not None:
            self._out(dones, (self.n,), torch.uint8, "dones")
        a = torch.empty(self.n, 4, dtype=torch.float32, device=obs.device) if out is None \
            else self._out(out, (self.n, 4), torch.float32, "out")
        if costs_out is not None:
            self._out(costs_out, (self.n, self.samples), torch.float64, "costs_out")
        check(_lib.lib().dr_mppi_step(ctypes.byref(self.cfg), self.n, ptr(obs), ptr(dones),
                                      ptr(self.nominal), ptr(self.calls), ptr(a), ptr(costs_out),
                                      _s(obs)))
        return a

    # ------------------------------------------------------------ checkpoint
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self.SETTINGS}
        sd["nominal"] = self.nominal.cpu().clone()
        sd["calls"] = self.calls.cpu().clone()
        return sd

    def load_state_dict(self, sd):
        """The warm start and call counts of a checkpoint with the same
        settings and shapes (the settings are the constructor's)."""
        for k in self.SETTINGS:
            if sd[k] != getattr(self, k):
                raise ValueError(f"MPPIPlanner: the checkpoint's {k} differs")
        for k in ("nominal", "calls"):
            if tuple(sd[k].shape) != tuple(getattr(self, k).shape):
                raise ValueError(f"MPPIPlanner: the checkpoint's {k} has another shape")
        self.nominal.copy_(sd["nominal"])
        self.calls.copy_(sd["calls"])
