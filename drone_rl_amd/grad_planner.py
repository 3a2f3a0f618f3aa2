"""GradPlanner: gradient trajectory planning by the adjoint of the gym env's
own physics (dr_gplan_*).

A controller that is not learned and does not sample: for every env it takes
`iterations` Adam steps on the warm-started action sequence, each on the
gradient of a quadratic tracking cost through `horizon` steps of the env's f64
step, and applies the first action.  Like MPPIPlanner it plans from the
15-float observation a policy sees, on the nominal airframe in still air, so
it can sit behind wind, an airframe spread or a SensorModel unchanged.  One
launch per plan step and no host round trip: a captured (env step -> plan)
loop holds it.
"""
from __future__ import annotations

import ctypes
import math

import torch

from . import _lib
from ._lib import check, ptr

OBS_DIM = 15
WEIGHTS = ("w_pos", "w_vel", "w_att", "w_rate", "w_effort", "w_pos_final", "w_vel_final")


def _s(t: torch.Tensor) -> int:
    return torch.cuda.current_stream(t.device).cuda_stream


def check_gplan(horizon=16, iterations=10, lr=0.05, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                w_pos=1.0, w_vel=0.05, w_att=0.05, w_rate=0.005, w_effort=0.0, w_pos_final=10.0,
                w_vel_final=1.0) -> None:
    """The value rules of the planner's settings, raised
    as ValueError on the host, each message naming its argument."""
    def real(x):
        return not isinstance(x, bool) and isinstance(x, (int, float)) and math.isfinite(x)

    def whole(x, lo, hi):
        return not isinstance(x, bool) and isinstance(x, int) and lo <= x <= hi
    if not whole(horizon, 1, _lib.DR_GPLAN_MAX_HORIZON):
        raise ValueError(f"horizon must be an integer in [1, {_lib.DR_GPLAN_MAX_HORIZON}], "
                         f"got {horizon!r}")
    if not whole(iterations, 1, _lib.DR_GPLAN_MAX_ITERATIONS):
        raise ValueError(f"iterations must be an integer in [1, {_lib.DR_GPLAN_MAX_ITERATIONS}], "
                         f"got {iterations!r}")
    if not real(lr) or lr <= 0:
        raise ValueError(f"lr must be > 0 and finite, got {lr!r}")
    if not real(beta1) or not 0 <= beta1 < 1:
        raise ValueError(f"beta1 must be in [0, 1), got {beta1!r}")
    if not real(beta2) or not 0 <= beta2 < 1:
        raise ValueError(f"beta2 must be in [0, 1), got {beta2!r}")
    if not real(adam_eps) or adam_eps <= 0:
        raise ValueError(f"adam_eps must be > 0 and finite, got {adam_eps!r}")
    for name, w in zip(WEIGHTS, (w_pos, w_vel, w_att, w_rate, w_effort, w_pos_final,
                                 w_vel_final)):
        if not real(w) or w < 0:
            raise ValueError(f"{name} must be >= 0 and finite, got {w!r}")


class GradPlanner:
    """Shooting by gradient for `n` gym envs on device tensors.  State:
    `nominal` f32 (n, horizon, 4), the warm start.  `workspace` is scratch of
    one plan step (dr_gplan_workspace_bytes) and holds nothing between calls."""

    SETTINGS = ("horizon", "iterations", "lr", "beta1", "beta2", "adam_eps") + WEIGHTS

    def __init__(self, n, device, horizon=16, iterations=10, lr=0.05, beta1=0.9, beta2=0.999,
                 adam_eps=1e-8, w_pos=1.0, w_vel=0.05, w_att=0.05, w_rate=0.005, w_effort=0.0,
                 w_pos_final=10.0, w_vel_final=1.0):
        if isinstance(n, bool) or not isinstance(n, int) or n < 1:
            raise ValueError(f"GradPlanner needs n >= 1, got {n!r}")
        check_gplan(horizon, iterations, lr, beta1, beta2, adam_eps, w_pos, w_vel, w_att, w_rate,
                    w_effort, w_pos_final, w_vel_final)
        self.n, self.device = n, torch.device(device)
        self.horizon, self.iterations = horizon, iterations
        self.lr, self.beta1, self.beta2 = float(lr), float(beta1), float(beta2)
        self.adam_eps = float(adam_eps)
        for name, w in zip(WEIGHTS, (w_pos, w_vel, w_att, w_rate, w_effort, w_pos_final,
                                     w_vel_final)):
            setattr(self, name, float(w))
        self.cfg = _lib.dr_gplan_config(**{k: getattr(self, k) for k in self.SETTINGS})
        self.nominal = torch.empty(n, horizon, 4, dtype=torch.float32, device=self.device)
        self.workspace_bytes = _lib.lib().dr_gplan_workspace_bytes(n, horizon)
        self.workspace = torch.empty((self.workspace_bytes + 7) // 8, dtype=torch.float64,
                                     device=self.device)
        self.reset()

    def key(self) -> tuple:
        """Every value a captured launch holds as a kernel argument."""
        return tuple(getattr(self, k) for k in self.SETTINGS)

    def reset(self):
        """Every env's nominal back to hover thrust."""
        check(_lib.lib().dr_gplan_reset(ctypes.byref(self.cfg), self.n, ptr(self.nominal),
                                        _s(self.nominal)))

    def _out(self, t, shape, dtype, what):
        if t.dtype != dtype or t.device != self.nominal.device or not t.is_contiguous() \
                or tuple(t.shape) != shape:
            raise ValueError(f"{what}: expected a contiguous {dtype} device tensor of shape "
                             f"{shape}, got {t.dtype} {tuple(t.shape)}")
        return t

    def plan(self, obs, dones=None, out=None, cost_out=None, grad_out=None):
        """One plan step: obs (n, 15) f32 as the env (or a SensorModel) delivers
        it; dones (n,) u8, optional: a set flag says obs[i] opens a new episode,
        so env i plans from hover.  Returns the actions (n, 4) f32 (`out` if
        given); cost_out (n,) f64 receives the cost of the incoming nominal and
        grad_out (n, horizon, 4) f64 its gradient."""
        if obs.dim() != 2 or obs.shape[1] != OBS_DIM:
            raise ValueError(f"GradPlanner plans on the 15-float observation (gym variant only), "
                             f"got obs of shape {tuple(obs.shape)}")
        self._out(obs, (self.n, OBS_DIM), torch.float32, "obs")
        if dones is not None:
            self._out(dones, (self.n,), torch.uint8, "dones")
        a = torch.empty(self.n, 4, dtype=torch.float32, device=obs.device) if out is None \
            else self._out(out, (self.n, 4), torch.float32, "out")
        if cost_out is not None:
            self._out(cost_out, (self.n,), torch.float64, "cost_out")
        if grad_out is not None:
            self._out(grad_out, (self.n, self.horizon, 4), torch.float64, "grad_out")
        check(_lib.lib().dr_gplan_step(ctypes.byref(self.cfg), self.n, ptr(obs), ptr(dones),
                                       ptr(self.nominal), ptr(self.workspace),
                                       self.workspace_bytes, ptr(a), ptr(cost_out),
                                       ptr(grad_out), _s(obs)))
        return a

    # ------------------------------------------------------------ checkpoint
    def state_dict(self):
        sd = {k: getattr(self, k) for k in self.SETTINGS}
        sd["nominal"] = self.nominal.cpu().clone()
        return sd

    def load_state_dict(self, sd):
        """The warm start of a checkpoint with the same settings and shape (the
        settings are the constructor's)."""
        for k in self.SETTINGS:
            if sd[k] != getattr(self, k):
                raise ValueError(f"GradPlanner: the checkpoint's {k} differs")
        if tuple(sd["nominal"].shape) != tuple(self.nominal.shape):
            raise ValueError("GradPlanner: the checkpoint's nominal has another shape")
        self.nominal.copy_(sd["nominal"])
