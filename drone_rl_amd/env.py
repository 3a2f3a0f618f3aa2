"""GPU-resident batch of quadrotor envs over libdronerl.so.

`DroneBatch` is the zero-copy torch path (every buffer is a device tensor,
all work is enqueued on the current HIP stream); `DroneGymEnv` mirrors the
reference's single-env gym class (/root/reference/drone.py:254-274) on top of
a one-env batch.  The SB3 / gymnasium vector facades live in vec_env.py.
"""
from __future__ import annotations

import ctypes
from typing import Callable, NamedTuple

import numpy as np
import torch

from . import _lib
from ._lib import check, ptr

# Physical constants of the reference (drone.py:14-43, 263); exposed as
# attributes because callers read them (e.g. env.mass, env.g: drone.py:263,292).
DT = 0.02
MASS = 1.0
G = 9.81
INERTIA = (0.005, 0.005, 0.01)
ARM_LENGTH = 0.5
K_YAW = 0.01
MAX_STEPS = 200
MOTOR_MAX = 3 * MASS * G / 4.0          # 7.3575, action_space.high
OBS_DIM = {"gym": 15, "vectorized": 12, "moving": 18, "smooth": 19, "tag": 19, "rk4": 16}
# the force each motor applies after a reset of the "smooth" variant
# (DESIGN.md section 14): f32(mass * g / 4)
HOVER = float(np.float32(MASS * G / 4.0))
# reset uniforms per env and reset for rng="host" 
RESET_UNIFORMS = {"gym": 5, "vectorized": 5, "moving": 14, "smooth": 5, "tag": 5, "rk4": 5}
_VARIANT_ID = {"gym": _lib.DR_VARIANT_GYM, "vectorized": _lib.DR_VARIANT_VECTORIZED,
               "moving": _lib.DR_VARIANT_MOVING, "smooth": _lib.DR_VARIANT_SMOOTH,
               "tag": _lib.DR_VARIANT_TAG, "rk4": _lib.DR_VARIANT_RK4}
# the "tag" variant's defaults
TAG_RADIUS = 0.25
CRASH_PENALTY = 0.0

_VEC_FIELDS = ("pos", "vel", "euler", "omega", "target")
# (N, width) f32 fields a single variant owns
_F32_ROW_FIELDS = {"motion": 9, "motor": 4, "wind": 6, "airframe": 6}
# (N, width) i32 fields
_I32_ROW_FIELDS = {"waypoint": 2}
# dr_set_waypoints' defaults where only one of the two values is given
REACH_RADIUS = 0.25
REACH_BONUS = 1.0
# the gym options that exclude each other (a handle has one option slot), by
# ENV_OPTIONS name, and the refusal of each pair
EXCLUSIONS = {
    frozenset(("wind", "waypoints")): "a gym env has wind or a waypoint course, not both",
    frozenset(("wind", "airframe")): "a gym env has wind or randomised airframes, not both",
    frozenset(("waypoints", "airframe")):
        "a gym env has a waypoint course or randomised airframes, not both",
}


def quat_to_euler(q) -> np.ndarray:
    """(..., 4) unit quaternions (w, x, y, z), body -> world, to the ZYX Euler
    angles (roll, pitch, yaw) the other variants keep; f64.  Pitch comes back
    in [-pi/2, pi/2]: the round trip holds for |pitch| < pi/2."""
    q = np.asarray(q, np.float64)
    a, b, c, d = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    roll = np.arctan2(2.0 * (a * b + c * d), 1.0 - 2.0 * (b * b + c * c))
    pitch = np.arcsin(np.clip(2.0 * (a * c - d * b), -1.0, 1.0))
    yaw = np.arctan2(2.0 * (a * d + b * c), 1.0 - 2.0 * (c * c + d * d))
    return np.stack([roll, pitch, yaw], axis=-1)


def euler_to_quat(e) -> np.ndarray:
    """(..., 3) ZYX Euler angles (roll, pitch, yaw) to unit quaternions
    (w, x, y, z); f64.  The inverse of quat_to_euler up to the sign of q."""
    e = np.asarray(e, np.float64)
    cr, sr = np.cos(e[..., 0] * 0.5), np.sin(e[..., 0] * 0.5)
    cp, sp = np.cos(e[..., 1] * 0.5), np.sin(e[..., 1] * 0.5)
    cy, sy = np.cos(e[..., 2] * 0.5), np.sin(e[..., 2] * 0.5)
    return np.stack([cr * cp * cy + sr * sp * sy, sr * cp * cy - cr * sp * sy,
                     cr * sp * cy + sr * cp * sy, cr * cp * sy - sr * sp * cy], axis=-1)


def check_field(variant: str, field: str) -> None:
    """The "quat" field exists only on the "rk4" variant (where "euler" is
    derived from it on the host): raised as ValueError before any device
    work.  ("motion" and "motor" on the wrong variant are refused by the C
    call.)"""
    if field == "quat" and variant != "rk4":
        raise ValueError(f"field 'quat' exists only on variant 'rk4', not {variant!r}")


def check_smoothing(variant: str, motor_alpha: float, rate_penalty: float) -> None:
    """The argument rules of dr_set_smoothing, raised as ValueError before any
    device work: alpha in (0, 1], rate_penalty finite and >= 0, and both at
    their neutral values (1, 0) on every variant but "smooth"."""
    a, lam = float(motor_alpha), float(rate_penalty)
    if not (0.0 < a <= 1.0):
        raise ValueError(f"motor_alpha must be in (0, 1], got {motor_alpha!r}")
    if not (0.0 <= lam < float("inf")):
        raise ValueError(f"rate_penalty must be finite and >= 0, got {rate_penalty!r}")
    if variant != "smooth" and (a != 1.0 or lam != 0.0):
        raise ValueError(f"motor_alpha / rate_penalty need variant='smooth', not {variant!r}")


def check_wind(variant: str, drag=0.0, wind_speed=0.0, gust_sigma=0.0, gust_rate=0.0,
               max_steps: int | None = None) -> tuple[float, float, float, float]:
    """The argument rules of dr_set_wind, raised as
    ValueError before any device work: drag, wind_speed and gust_sigma finite
    and >= 0 in f32, gust_rate in [0, 1], drag * dt <= 1 (the explicit drag
    update must not overshoot), all four at 0 on every variant but "gym", and
    a step limit below 2^24 where any is not.  Returns the four values as the
    kernels see them (rounded to f32)."""
    names = ("drag", "wind_speed", "gust_sigma", "gust_rate")
    vals = []
    with np.errstate(over="ignore", invalid="ignore"):
        for name, x in zip(names, (drag, wind_speed, gust_sigma, gust_rate)):
            v = float(np.float32(x))
            if not (0.0 <= v < float("inf")):
                raise ValueError(f"{name} must be finite and >= 0, got {x!r}")
            vals.append(v)
    if vals[3] > 1.0:
        raise ValueError(f"gust_rate must be in [0, 1], got {gust_rate!r}")
    if vals[0] * DT > 1.0:
        raise ValueError(f"drag * dt must be <= 1 (dt = {DT}), got drag = {drag!r}")
    if any(vals):
        if variant != "gym":
            raise ValueError("drag / wind_speed / gust_sigma / gust_rate need variant='gym', "
                             f"not {variant!r}")
        if max_steps is not None and int(max_steps) >= 1 << 24:
            raise ValueError("wind needs max_steps below 2^24")
    return tuple(vals)


def check_waypoints(variant: str, reach_radius=None, reach_bonus=None,
                    max_steps: int | None = None, wind=None) -> tuple[float, float] | None:
    """The argument rules of dr_set_waypoints, raised
    as ValueError before any device work.  None / None means the option is off
    and returns None; giving one of the two enables it with the other at its
    default (0.25 / 1.0).  reach_radius must be finite and > 0 in f32,
    reach_bonus finite and >= 0; the variant must be "gym", its step limit
    below 2^24, and `wind` (the four dr_set_wind values, if given) all zero.
    Returns the two values as the kernels see them (rounded to f32)."""
    if reach_radius is None and reach_bonus is None:
        return None
    with np.errstate(over="ignore", invalid="ignore"):
        r = float(np.float32(REACH_RADIUS if reach_radius is None else reach_radius))
        b = float(np.float32(REACH_BONUS if reach_bonus is None else reach_bonus))
    if not (0.0 < r < float("inf")):
        raise ValueError(f"reach_radius must be finite and > 0, got {reach_radius!r}")
    if not (0.0 <= b < float("inf")):
        raise ValueError(f"reach_bonus must be finite and >= 0, got {reach_bonus!r}")
    if variant != "gym":
        raise ValueError(f"reach_radius / reach_bonus need variant='gym', not {variant!r}")
    if max_steps is not None and int(max_steps) >= 1 << 24:
        raise ValueError("waypoint courses need max_steps below 2^24")
    if wind is not None and any(float(w) != 0.0 for w in wind):
        raise ValueError(EXCLUSIONS[frozenset(("wind", "waypoints"))])
    return r, b


def check_airframe(variant: str, mass_spread=0.0, inertia_spread=0.0, motor_spread=0.0, *,
                   wind=None, waypoints=None) -> tuple[float, float, float]:
    """The argument rules of dr_set_airframe, raised as
    ValueError before any device work: each spread finite and in [0, 0.9] in
    f32, all three at 0 on every variant but "gym", and, where any is not 0,
    `wind` (the four dr_set_wind values, if given) all zero and `waypoints`
    (check_waypoints' result, if given) None.  Returns the three values as the
    kernels see them (rounded to f32)."""
    names = ("mass_spread", "inertia_spread", "motor_spread")
    vals = []
    with np.errstate(over="ignore", invalid="ignore"):
        for name, x in zip(names, (mass_spread, inertia_spread, motor_spread)):
            v = float(np.float32(x))
            if not (0.0 <= v <= float(np.float32(0.9))):
                raise ValueError(f"{name} must be in [0, 0.9], got {x!r}")
            vals.append(v)
    if any(vals):
        if variant != "gym":
            raise ValueError("mass_spread / inertia_spread / motor_spread need variant='gym', "
                             f"not {variant!r}")
        if wind is not None and any(float(w) != 0.0 for w in wind):
            raise ValueError(EXCLUSIONS[frozenset(("wind", "airframe"))])
        if waypoints is not None:
            raise ValueError(EXCLUSIONS[frozenset(("waypoints", "airframe"))])
    return tuple(vals)


def check_tag(variant: str, tag_radius, crash_penalty, num_envs: int | None = None,
              env_id_offset: int = 0) -> tuple[float, float]:
    """The argument rules of the "tag" variant (dr_create / dr_set_tag), raised
    as ValueError before any device work: tag_radius finite and > 0,
    crash_penalty finite and >= 0, both None (the variant's defaults) on every
    other variant, and an even number of drones at an even env_id_offset.
    Returns the two values with the defaults filled in."""
    if variant != "tag":
        if tag_radius is not None or crash_penalty is not None:
            raise ValueError(f"tag_radius / crash_penalty need variant='tag', not {variant!r}")
        return TAG_RADIUS, CRASH_PENALTY
    r = TAG_RADIUS if tag_radius is None else float(tag_radius)
    c = CRASH_PENALTY if crash_penalty is None else float(crash_penalty)
    if not (0.0 < r < float("inf")):
        raise ValueError(f"tag_radius must be finite and > 0, got {tag_radius!r}")
    if not (0.0 <= c < float("inf")):
        raise ValueError(f"crash_penalty must be finite and >= 0, got {crash_penalty!r}")
    if num_envs is not None and (int(num_envs) % 2 or int(env_id_offset) % 2):
        raise ValueError("variant='tag' pairs env 2j with env 2j+1: num_envs and env_id_offset "
                         f"must be even, got {num_envs!r} and {env_id_offset!r}")
    return r, c


class EnvOption(NamedTuple):
    """One optional mechanism of the env, as every Python layer reads it."""
    name: str
    variant: str        # the variant that owns it
    keys: tuple         # its keywords, in the order of its check_* and set_*
    defaults: tuple     # ... and their values where the option is off
    idle: tuple         # what DroneBatch's attributes of those names read while it is off
    field: str | None   # the state field it enables ("<name>_enabled" says whether it has)
    check: Callable     # check_*(variant, *values, **context)
    context: tuple      # the keywords of check_env_options its check_* also takes
    setter: str         # the DroneBatch method that applies it
    help: tuple         # one command-line help text per keyword


ENV_OPTIONS = (
    EnvOption("smoothing", "smooth", ("motor_alpha", "rate_penalty"), (1.0, 0.0), (1.0, 0.0),
              None, check_smoothing, (), "set_smoothing",
              ("--variant smooth: lag blend dt / (tau + dt) in (0, 1] (1 = no lag)",
               "--variant smooth: penalty on |command - motor force|^2 per step")),
    EnvOption("tag", "tag", ("tag_radius", "crash_penalty"), (None, None),
              (TAG_RADIUS, CRASH_PENALTY), None, check_tag, ("num_envs", "env_id_offset"),
              "set_tag",
              ("--variant tag: the pursuer's bonus radius in m (default 0.25)",
               "--variant tag: what a crashing drone pays (default 0)")),
    EnvOption("wind", "gym", ("drag", "wind_speed", "gust_sigma", "gust_rate"), (0.0,) * 4,
              (0.0,) * 4, "wind", check_wind, ("max_steps",), "set_wind",
              ("--variant gym: linear drag per unit mass in 1/s (0 = vacuum)",
               "--variant gym: bound of each axis of the per-episode mean wind, m/s",
               "--variant gym: stationary std of each gust axis, m/s",
               "--variant gym: the gusts' per-step mean reversion in [0, 1]")),
    EnvOption("waypoints", "gym", ("reach_radius", "reach_bonus"), (None, None), (0.0, 0.0),
              "waypoint", check_waypoints, ("max_steps",), "set_waypoints",
              ("--variant gym: fly waypoint courses; the target moves on inside "
               "this distance (default 0.25 when only --reach-bonus is given)",
               "--variant gym: reward added in the step of a reach (default 1.0 "
               "when only --reach-radius is given)")),
    EnvOption("airframe", "gym", ("mass_spread", "inertia_spread", "motor_spread"), (0.0,) * 3,
              (0.0,) * 3, "airframe", check_airframe, (), "set_airframe",
              ("--variant gym: per-episode mass scale drawn in 1 +- this, in [0, 0.9]",
               "--variant gym: per-episode inertia scale drawn in 1 +- this",
               "--variant gym: per-episode gain of each motor drawn in 1 +- this")),
)
ENV_OPTION_KEYS = tuple(k for o in ENV_OPTIONS for k in o.keys)
ENV_OPTION = {o.name: o for o in ENV_OPTIONS}


def _excluded(name: str, others) -> None:
    """Refuse option `name` beside any of the options `others` that excludes it."""
    for other in others:
        if frozenset((name, other)) in EXCLUSIONS:
            raise ValueError(EXCLUSIONS[frozenset((name, other))])


def check_env_options(variant: str, options: dict, *, num_envs=None, env_id_offset=0,
                      max_steps=None, last=()) -> dict:
    """Every option's check_* on the keywords in `options` (a missing one is
    at its default), in table order with the options named in `last` behind
    the others, then the exclusions: raised as ValueError before any device
    work.  Returns, per option name, the values its set_* takes, or None where
    the option is off (a variant's own parameters are on with the variant, a
    gym option with a value off neutral)."""
    context = {"num_envs": num_envs, "env_id_offset": env_id_offset, "max_steps": max_steps}
    checked = {}
    for o in sorted(ENV_OPTIONS, key=lambda o: o.name in last):
        given = tuple(options.get(k, d) for k, d in zip(o.keys, o.defaults))
        vals = o.check(variant, *given, **{k: context[k] for k in o.context})
        if o.field is None:
            vals = (given if vals is None else vals) if variant == o.variant else None
        elif vals is not None and any(vals):
            _excluded(o.name, (n for n, v in checked.items() if v is not None))
        else:
            vals = None
        checked[o.name] = vals
    return checked


def add_option_arguments(parser, first=()) -> None:
    """One --flag per option keyword, off by default, in table order with the
    options named in `first` ahead of the others."""
    for o in sorted(ENV_OPTIONS, key=lambda o: o.name not in first):
        for k, d, h in zip(o.keys, o.defaults, o.help):
            parser.add_argument("--" + k.replace("_", "-"), type=float, default=d, help=h)


def option_values(namespace) -> dict:
    """The option keywords of a namespace add_option_arguments' parser filled."""
    return {k: getattr(namespace, k) for k in ENV_OPTION_KEYS}


def _stream(device):
    return torch.cuda.current_stream(device).cuda_stream


class DroneBatch:
    """N independent quadrotor envs in HBM (struct of arrays).

    variant    "gym" (DroneGymEnv, drone.py), "vectorized"
               (VectorizedDroneEnv, vectorized_drone.py) or "moving" (the
               moving-target curriculum of BASELINE configs[4]; 18-d obs)
               or "smooth" (the gym env behind a first-order motor lag with
               an action-rate penalty; 19-d obs)
               or "tag" (envs 2j / 2j+1 are a pursuer / evader pair with a
               zero-sum reward; 19-d obs; num_envs
               counts drones and is even)
               or "rk4" (the gym env's task on a unit-quaternion attitude
               advanced by one RK4 step; 16-d obs; the
               attitude is the field "quat", "euler" is derived from it)
    dtype      torch.float64 (reference precision) or torch.float32 state
    rng        "philox" (counter-based, seeded) or "host" (caller supplies
               the reset uniforms: numpy-MT19937 replay for parity tests)
    auto_reset DummyVecEnv semantics: a done env is reset inside the step
               and obs holds the reset observation.
    motor_alpha, rate_penalty
               "smooth" only: the lag blend alpha = dt / (tau + dt) in (0, 1]
               and the penalty on |command - motor force|^2 (>= 0).  At the
               defaults (1, 0) the variant is "gym" bit for bit.
    tag_radius, crash_penalty
               "tag" only: the distance inside which the pursuer collects its
               bonus (> 0) and what a crashing drone pays (>= 0).  None = the
               variant's defaults (0.25, 0).
    drag, wind_speed, gust_sigma, gust_rate
               "gym" only: linear drag per unit mass
               (1/s), the bound of each axis of the per-episode mean wind
               (m/s), the gusts' stationary standard deviation per axis (m/s)
               and their per-step mean reversion in [0, 1].  All neutral at 0;
               the wind is not observed (the obs stays the gym's 15 floats).
               Any non-zero value enables the "wind" field ((N,6) f32: mean
               wind xyz, gust xyz).
    reach_radius, reach_bonus
               "gym" only: a waypoint course.  The
               target moves on to a fresh draw when the drone comes closer
               than reach_radius (> 0), and that step's reward gains
               reach_bonus (>= 0).  None / None = off; giving one enables the
               option with the other at its default (0.25 / 1.0), and with it
               the "waypoint" field ((N,2) i32: index within the episode,
               reaches since enabling).  Not together with wind.
    mass_spread, inertia_spread, motor_spread
               "gym" only: per-episode airframe
               randomisation.  Each episode draws a mass scale m in
               1 +- mass_spread, an inertia scale s in 1 +- inertia_spread and
               four motor gains in 1 +- motor_spread, each spread in [0, 0.9].
               All neutral at 0; the airframe is not observed.  Any non-zero
               value enables the "airframe" field ((N,6) f32: m, s, g0..g3).
               Not together with wind or a waypoint course.
    """

    def __init__(self, num_envs: int, variant: str = "gym",
                 dtype: torch.dtype = torch.float64, device=None, seed: int = 0,
                 auto_reset: bool = True, rng: str = "philox",
                 env_id_offset: int = 0, max_steps: int | None = None,
                 keep_terminal_obs: bool = False, monitor: bool = False, **options):
        for k in options:
            if k not in ENV_OPTION_KEYS:
                raise TypeError(f"DroneBatch.__init__() got an unexpected keyword argument '{k}'")
        if variant not in OBS_DIM:
            raise ValueError(f"unknown variant {variant!r}")
        # (the tag rules last: the order these refusals have always come in)
        options = check_env_options(variant, options, num_envs=num_envs,
                                    env_id_offset=env_id_offset, max_steps=max_steps,
                                    last=("tag",))
        if dtype not in (torch.float64, torch.float32):
            raise ValueError("dtype must be torch.float64 or torch.float32")
        if rng not in ("philox", "host"):
            raise ValueError("rng must be 'philox' or 'host'")
        if not torch.cuda.is_available():
            raise RuntimeError("DroneBatch needs a HIP device (no CPU fallback)")
        self.L = _lib.lib()
        self.device = torch.device("cuda", torch.cuda.current_device()) \
            if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.num_envs = int(num_envs)
        self.variant = variant
        self.dtype = dtype
        self.obs_dim = OBS_DIM[variant]
        self.auto_reset = bool(auto_reset) and variant != "vectorized"
        self.monitor = monitor
        self.seed_value = int(seed)
        self.env_id_offset = int(env_id_offset)
        cfg = _lib.dr_config(
            num_envs=self.num_envs,
            variant=_VARIANT_ID[variant],
            state_dtype=_lib.DR_STATE_F64 if dtype == torch.float64 else _lib.DR_STATE_F32,
            rng_mode=_lib.DR_RNG_PHILOX if rng == "philox" else _lib.DR_RNG_HOST_UNIFORMS,
            auto_reset=int(self.auto_reset), device=self.device.index,
            max_steps=int(max_steps or 0), seed=self.seed_value & (2**64 - 1),
            env_id_offset=self.env_id_offset, dt=DT)
        h = ctypes.c_void_p()
        check(self.L.dr_create(ctypes.byref(cfg), ctypes.byref(h)))
        self.handle = h
        self.max_steps = int(max_steps or (1000 if variant == "vectorized" else MAX_STEPS))
        n, od, dev = self.num_envs, self.obs_dim, self.device
        self.obs = torch.zeros(n, od, dtype=torch.float32, device=dev)
        self.rew = torch.zeros(n, dtype=torch.float32, device=dev)
        self.done = torch.zeros(n, dtype=torch.uint8, device=dev)
        self.term_obs = torch.zeros(n, od, dtype=torch.float32, device=dev) \
            if keep_terminal_obs else None
        self.ep_ret = torch.zeros(n, dtype=torch.float32, device=dev) if monitor else None
        self.ep_len = torch.zeros(n, dtype=torch.int32, device=dev) if monitor else None
        self._uniforms = None
        for o in ENV_OPTIONS:
            self.__dict__.update(zip(o.keys, o.idle))
            if o.field is not None:
                setattr(self, o.name + "_enabled", False)
        for o in ENV_OPTIONS:
            if options[o.name] is not None:
                getattr(self, o.setter)(*options[o.name])

    # -- lifecycle -------------------------------------------------------
    def close(self):
        if getattr(self, "handle", None) is not None and self.handle.value:
            self.L.dr_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- core API ----------------------------------------------------------
    def reset(self, obs_out: torch.Tensor | None = None) -> torch.Tensor:
        out = self.obs if obs_out is None else obs_out
        self._check_out(out, (self.num_envs, self.obs_dim), torch.float32)
        check(self.L.dr_reset(self.handle, ptr(out), _stream(self.device)), self.handle)
        return out

    def reset_masked(self, mask: torch.Tensor, obs_out: torch.Tensor | None = None):
        out = self.obs if obs_out is None else obs_out
        mask = mask.to(device=self.device, dtype=torch.uint8).contiguous()
        check(self.L.dr_reset_masked(self.handle, ptr(mask), ptr(out),
                                     _stream(self.device)), self.handle)
        return out

    def step(self, actions: torch.Tensor, obs_out=None, rew_out=None, done_out=None,
             trunc_out=None):
        """Advance every env one step.  `actions` (N,4) f32 on the device.
        Returns (obs, rew, done) device tensors (the batch's own buffers unless
        *_out are given: copy them before the next step if you keep them).
        `trunc_out` (N,) u8, monitor=True only: 1 where the episode ended at
        the step limit without a crash (dr_step_monitored_trunc)."""
        obs = self.obs if obs_out is None else obs_out
        rew = self.rew if rew_out is None else rew_out
        done = self.done if done_out is None else done_out
        a = actions
        if a.dtype != torch.float32 or a.device != self.device or not a.is_contiguous() \
                or a.data_ptr() % 16:
            a = a.to(device=self.device, dtype=torch.float32).contiguous()
        if a.shape != (self.num_envs, 4):
            raise ValueError(f"actions must be ({self.num_envs}, 4), got {tuple(a.shape)}")
        self._check_out(obs, (self.num_envs, self.obs_dim), torch.float32)
        self._check_out(rew, (self.num_envs,), torch.float32)
        self._check_out(done, (self.num_envs,), torch.uint8)
        s = _stream(self.device)
        if trunc_out is not None:
            if not self.monitor:
                raise ValueError("trunc_out needs a monitor=True batch")
            self._check_out(trunc_out, (self.num_envs,), torch.uint8)
            check(self.L.dr_step_monitored_trunc(self.handle, ptr(a), ptr(obs), ptr(rew),
                                                 ptr(done), ptr(self.term_obs), ptr(self.ep_ret),
                                                 ptr(self.ep_len), ptr(trunc_out), s),
                  self.handle)
        elif self.monitor:
            check(self.L.dr_step_monitored(self.handle, ptr(a), ptr(obs), ptr(rew), ptr(done),
                                           ptr(self.term_obs), ptr(self.ep_ret),
                                           ptr(self.ep_len), s), self.handle)
        else:
            check(self.L.dr_step(self.handle, ptr(a), ptr(obs), ptr(rew), ptr(done),
                                 ptr(self.term_obs), s), self.handle)
        return obs, rew, done

    def rollout(self, k: int, actions: torch.Tensor | None = None, *, seed: int = 0,
                step0: int = 0, lo: float = 0.0, hi: float = MOTOR_MAX,
                actions_out: torch.Tensor | None = None,
                obs_out=None, rew_out=None, done_out=None):
        """k steps in one launch (dr_rollout): outputs identical to k calls of
        step().  `actions` (k,N,4) f32 on the device, or None for the
        in-kernel random policy (step t draws random_actions(N, seed, step0+t,
        env_id_offset, lo, hi); `actions_out` (k,N,4) receives them if given).
        Returns (obs (k,N,obs_dim), rew (k,N), done (k,N)); no terminal obs or
        VecMonitor counters (use step() for those).  Refused on a monitor=True
        batch: the launch does not advance the running episode return /
        length, so a later step() would report wrong episodes."""
        if self.monitor:
            raise ValueError("rollout() on a monitor=True batch would leave the VecMonitor "
                             "episode counters stale; use step() or a monitor=False batch")
        k = int(k)
        n, od, dev = self.num_envs, self.obs_dim, self.device
        obs = torch.empty(k, n, od, dtype=torch.float32, device=dev) if obs_out is None else obs_out
        rew = torch.empty(k, n, dtype=torch.float32, device=dev) if rew_out is None else rew_out
        done = torch.empty(k, n, dtype=torch.uint8, device=dev) if done_out is None else done_out
        self._check_out(obs, (k, n, od), torch.float32)
        self._check_out(rew, (k, n), torch.float32)
        self._check_out(done, (k, n), torch.uint8)
        s = _stream(dev)
        if actions is None:
            if actions_out is not None:
                self._check_out(actions_out, (k, n, 4), torch.float32)
            check(self.L.dr_rollout_random(self.handle, k, seed & (2**64 - 1), step0, lo, hi,
                                           ptr(actions_out), ptr(obs), ptr(rew), ptr(done), s),
                  self.handle)
        else:
            a = actions
            if a.dtype != torch.float32 or a.device != dev or not a.is_contiguous() \
                    or a.data_ptr() % 16:
                a = a.to(device=dev, dtype=torch.float32).contiguous()
            if a.shape != (k, n, 4):
                raise ValueError(f"actions must be ({k}, {n}, 4), got {tuple(a.shape)}")
            check(self.L.dr_rollout(self.handle, k, ptr(a), ptr(obs), ptr(rew), ptr(done), s),
                  self.handle)
        return obs, rew, done

    # -- host-buffer I/O (the drop-in surfaces) ------------------------------
    def _host_buffers(self):
        """Pinned host buffers the kernels read / write directly (zero-copy
        over PCIe): a host-buffer step is one launch and one stream sync, no
        separate H2D / D2H copies."""
        hb = getattr(self, "_hb", None)
        if hb is None:
            n, od = self.num_envs, self.obs_dim
            pin = dict(device="cpu", pin_memory=True)
            f32 = dict(dtype=torch.float32, **pin)
            hb = {"act": torch.zeros(n, 4, **f32), "obs": torch.zeros(n, od, **f32),
                  "rew": torch.zeros(n, **f32),
                  "done": torch.zeros(n, dtype=torch.uint8, **pin),
                  "term": torch.zeros(n, od, **f32) if self.term_obs is not None else None,
                  "ep_ret": torch.zeros(n, **f32) if self.monitor else None,
                  "ep_len": torch.zeros(n, dtype=torch.int32, **pin) if self.monitor else None}
            hb["np"] = {k: (v.numpy() if v is not None else None) for k, v in hb.items()}
            self._hb = hb
        return hb

    def reset_host(self) -> np.ndarray:
        """reset() into a pinned host buffer; returns a numpy view of it
        (overwritten by the next host-buffer call: copy to keep)."""
        hb = self._host_buffers()
        check(self.L.dr_reset(self.handle, ptr(hb["obs"]), _stream(self.device)), self.handle)
        torch.cuda.current_stream(self.device).synchronize()
        return hb["np"]["obs"]

    def step_host(self, actions):
        """step() with host buffers: `actions` any (N,4)-shaped array-like;
        the kernel reads them from, and writes obs / rew / done (and, when
        kept, the terminal obs and VecMonitor outputs of done rows) to, pinned
        host memory.  Returns the numpy views {"obs", "rew", "done", "term",
        "ep_ret", "ep_len"}, valid until the next host-buffer call."""
        hb = self._host_buffers()
        a = np.asarray(actions, dtype=np.float32)
        if a.size != self.num_envs * 4:
            raise ValueError(f"actions must be ({self.num_envs}, 4), got {a.shape}")
        np.copyto(hb["np"]["act"], a.reshape(self.num_envs, 4))
        s = _stream(self.device)
        if self.monitor:
            check(self.L.dr_step_monitored(self.handle, ptr(hb["act"]), ptr(hb["obs"]),
                                           ptr(hb["rew"]), ptr(hb["done"]), ptr(hb["term"]),
                                           ptr(hb["ep_ret"]), ptr(hb["ep_len"]), s),
                  self.handle)
        else:
            check(self.L.dr_step(self.handle, ptr(hb["act"]), ptr(hb["obs"]), ptr(hb["rew"]),
                                 ptr(hb["done"]), ptr(hb["term"]), s), self.handle)
        torch.cuda.current_stream(self.device).synchronize()
        return hb["np"]

    # -- state access ------------------------------------------------------
    def _field_out(self, field: str, **where) -> torch.Tensor:
        n = self.num_envs
        if field in _VEC_FIELDS:
            return torch.empty(n, 3, dtype=torch.float64, **where)
        if field == "eps":
            return torch.empty(n, dtype=torch.float64, **where)
        if field == "ep_return":
            return torch.empty(n, dtype=torch.float32, **where)
        if field in _F32_ROW_FIELDS:
            return torch.empty(n, _F32_ROW_FIELDS[field], dtype=torch.float32, **where)
        if field in _I32_ROW_FIELDS:
            return torch.empty(n, _I32_ROW_FIELDS[field], dtype=torch.int32, **where)
        if field == "quat":
            return torch.empty(n, 4, dtype=self.dtype, **where)
        return torch.empty(n, dtype=torch.int32, **where)

    def _derived_euler(self, field: str) -> bool:
        """rk4 keeps no Euler angles: "euler" is converted from / to "quat"
        on the host."""
        check_field(self.variant, field)
        return self.variant == "rk4" and field == "euler"

    def get(self, field: str) -> torch.Tensor:
        if self._derived_euler(field):
            return torch.from_numpy(quat_to_euler(self.get_host("quat"))).to(self.device)
        fid = _lib.FIELDS[field]
        out = self._field_out(field, device=self.device)
        check(self.L.dr_get_state(self.handle, fid, ptr(out), _stream(self.device)), self.handle)
        return out

    def get_host(self, field: str) -> np.ndarray:
        """get(field) as a fresh numpy array: the field kernel writes into a
        pinned host buffer (one launch + one sync, no D2H copy)."""
        if self._derived_euler(field):
            return quat_to_euler(self.get_host("quat"))
        fid = _lib.FIELDS[field]
        bufs = self.__dict__.setdefault("_field_host", {})
        out = bufs.get(field)
        if out is None:
            out = bufs[field] = self._field_out(field, device="cpu", pin_memory=True)
        check(self.L.dr_get_state(self.handle, fid, ptr(out), _stream(self.device)), self.handle)
        torch.cuda.current_stream(self.device).synchronize()
        return out.numpy().copy()

    def gather(self, field: str, env_ids: torch.Tensor, out: torch.Tensor | None = None):
        """`get(field)` for the envs in env_ids (int32 device tensor), into
        `out` if given (k,3) f64 / (k,) / (k,9) f32 for "motion" / (k,4) f32 for
        "motor" / (k,4) in the state dtype for "quat"."""
        if self._derived_euler(field):
            e = torch.from_numpy(quat_to_euler(self.gather("quat", env_ids).cpu().numpy()))
            if out is None:
                return e.to(self.device)
            out.copy_(e)
            return out
        fid = _lib.FIELDS[field]
        k = env_ids.numel()
        if out is None and field == "quat":
            out = torch.empty(k, 4, dtype=self.dtype, device=self.device)
        if out is None:
            if field in _VEC_FIELDS:
                out = torch.empty(k, 3, dtype=torch.float64, device=self.device)
            elif field == "eps":
                out = torch.empty(k, dtype=torch.float64, device=self.device)
            elif field == "ep_return":
                out = torch.empty(k, dtype=torch.float32, device=self.device)
            elif field in _F32_ROW_FIELDS:
                out = torch.empty(k, _F32_ROW_FIELDS[field], dtype=torch.float32,
                                  device=self.device)
            elif field in _I32_ROW_FIELDS:
                out = torch.empty(k, _I32_ROW_FIELDS[field], dtype=torch.int32,
                                  device=self.device)
            else:
                out = torch.empty(k, dtype=torch.int32, device=self.device)
        ids = env_ids.to(device=self.device, dtype=torch.int32).contiguous()
        check(self.L.dr_gather_state(self.handle, fid, ptr(ids), k, ptr(out),
                                     _stream(self.device)), self.handle)
        return out

    def set(self, field: str, value) -> None:
        if self._derived_euler(field):
            e = torch.as_tensor(value, dtype=torch.float64).reshape(self.num_envs, 3)
            return self.set("quat", euler_to_quat(e.cpu().numpy()))
        fid = _lib.FIELDS[field]
        if field == "quat":
            dt, shape = self.dtype, (self.num_envs, 4)
        elif field in _VEC_FIELDS:
            dt, shape = torch.float64, (self.num_envs, 3)
        elif field == "eps":
            dt, shape = torch.float64, (self.num_envs,)
        elif field == "ep_return":
            dt, shape = torch.float32, (self.num_envs,)
        elif field in _F32_ROW_FIELDS:
            dt, shape = torch.float32, (self.num_envs, _F32_ROW_FIELDS[field])
        elif field in _I32_ROW_FIELDS:
            dt, shape = torch.int32, (self.num_envs, _I32_ROW_FIELDS[field])
        else:
            dt, shape = torch.int32, (self.num_envs,)
        v = torch.as_tensor(value, dtype=dt).to(self.device).reshape(shape).contiguous()
        check(self.L.dr_set_state(self.handle, fid, ptr(v), _stream(self.device)), self.handle)
        torch.cuda.current_stream(self.device).synchronize()   # v may be freed

    def seed(self, seed: int) -> None:
        """New Philox key for every later reset (order-free per env)."""
        self.seed_value = int(seed)
        check(self.L.dr_set_seed(self.handle, self.seed_value & (2**64 - 1)), self.handle)

    def _check_set(self, name: str, *values):
        """What every set_* refuses, as ValueError before any device work: a
        batch of another variant, the option's argument rules and, where the
        values would switch a gym option on, an enabled option that excludes
        it.  Returns its check_*'s result."""
        o = ENV_OPTION[name]
        if self.variant != o.variant:
            raise ValueError(f"{o.setter} needs variant={o.variant!r}, not {self.variant!r}")
        context = {"max_steps": self.max_steps} if "max_steps" in o.context else {}
        vals = o.check(self.variant, *values, **context)
        if o.field is not None and any(vals):
            _excluded(name, (e.name for e in self._enabled_options()))
        return vals

    def option_state(self) -> tuple:
        """Per option in table order, its values and, where it has a state
        field, whether it is enabled: everything about the options that a
        captured graph holds (the kernels launched and their arguments)."""
        return tuple(tuple(getattr(self, k) for k in o.keys) +
                     ((getattr(self, o.name + "_enabled"),) if o.field is not None else ())
                     for o in ENV_OPTIONS)

    def _enabled_options(self) -> list:
        return [o for o in ENV_OPTIONS
                if o.field is not None and getattr(self, o.name + "_enabled")]

    def option_fields(self) -> tuple:
        """The state fields of the enabled options, in table order."""
        return tuple(o.field for o in self._enabled_options())

    def set_smoothing(self, motor_alpha: float, rate_penalty: float) -> None:
        """variant="smooth": new lag blend and action-rate penalty for every
        step / rollout enqueued after the call (a captured graph keeps the
        values it was captured with)."""
        self._check_set("smoothing", motor_alpha, rate_penalty)
        check(self.L.dr_set_smoothing(self.handle, float(motor_alpha), float(rate_penalty)),
              self.handle)
        self.motor_alpha, self.rate_penalty = float(motor_alpha), float(rate_penalty)

    def set_tag(self, tag_radius: float | None = None,
                crash_penalty: float | None = None) -> None:
        """variant="tag": new tag radius and crash penalty (None = the default)
        for every step / rollout enqueued after the call (a captured graph
        keeps the values it was captured with)."""
        r, c = self._check_set("tag", tag_radius, crash_penalty)
        check(self.L.dr_set_tag(self.handle, r, c), self.handle)
        # what the kernels see: the f32 values
        rr, cc = ctypes.c_float(), ctypes.c_float()
        check(self.L.dr_get_tag(self.handle, ctypes.byref(rr), ctypes.byref(cc)), self.handle)
        self.tag_radius, self.crash_penalty = float(rr.value), float(cc.value)

    def set_wind(self, drag: float = 0.0, wind_speed: float = 0.0, gust_sigma: float = 0.0,
                 gust_rate: float = 0.0) -> None:
        """variant="gym": linear drag, per-episode mean wind and gusts
        (dr_set_wind) for every step / rollout enqueued
        after the call; a new wind_speed applies from each env's next reset.
        The first call with a non-zero value allocates the "wind" field and
        draws every env's mean wind for its current episode: it waits for the
        device and must not be made while a graph is being captured (a
        captured graph keeps the kernels and values it was captured with)."""
        w = self._check_set("wind", drag, wind_speed, gust_sigma, gust_rate)
        check(self.L.dr_set_wind(self.handle, *w), self.handle)
        self.drag, self.wind_speed, self.gust_sigma, self.gust_rate = w
        self.wind_enabled = self.wind_enabled or any(w)

    def set_waypoints(self, reach_radius: float | None = None,
                      reach_bonus: float | None = None) -> None:
        """variant="gym": fly a waypoint course (dr_set_waypoints, DESIGN.md
        section 18) with this reach radius and bonus (None = 0.25 / 1.0) in
        every step / rollout enqueued after the call.  The first call
        allocates the "waypoint" field, zeroed: it waits for the device and
        must not be made while a graph is being captured (a captured graph
        keeps the kernels and values it was captured with).  The option
        cannot be switched off again."""
        if reach_radius is None and reach_bonus is None:
            reach_radius = REACH_RADIUS
        rb = self._check_set("waypoints", reach_radius, reach_bonus)
        check(self.L.dr_set_waypoints(self.handle, *rb), self.handle)
        self.reach_radius, self.reach_bonus = rb
        self.waypoints_enabled = True

    def set_airframe(self, mass_spread: float = 0.0, inertia_spread: float = 0.0,
                     motor_spread: float = 0.0) -> None:
        """variant="gym": per-episode airframe randomisation (dr_set_airframe,
        DESIGN.md section 19).  The spreads apply from each env's next reset
        (resets are their only readers).  The first call with a non-zero
        value allocates the "airframe" field and draws every env's airframe
        for its current episode: it waits for the device and must not be made
        while a graph is being captured (a captured graph keeps the kernels
        and values it was captured with).  All zeros on a batch that never
        enabled the option enables nothing."""
        a = self._check_set("airframe", mass_spread, inertia_spread, motor_spread)
        if (self.wind_enabled or self.waypoints_enabled) and not any(a):
            return   # neutral on a handle that carries another option: nothing to do
        check(self.L.dr_set_airframe(self.handle, *a), self.handle)
        self.mass_spread, self.inertia_spread, self.motor_spread = a
        self.airframe_enabled = self.airframe_enabled or any(a)

    def set_reset_uniforms(self, u) -> None:
        """rng='host': (N,5) f64 uniforms ((N,14) for "moving") consumed by
        the next resets."""
        t = torch.as_tensor(u, dtype=torch.float64).to(self.device).reshape(
            self.num_envs, RESET_UNIFORMS[self.variant]).contiguous()
        self._uniforms = t          # keep alive while kernels may read it
        check(self.L.dr_set_reset_uniforms(self.handle, ptr(t)), self.handle)

    @staticmethod
    def _check_out(t, shape, dtype):
        if t.dtype != dtype or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"output buffer must be contiguous {dtype} {shape}")


def random_actions(n: int, seed: int, step: int, env_id_offset: int = 0,
                   lo: float = 0.0, hi: float = MOTOR_MAX, out=None, device=None):
    """Synthetic random policy: (n,4) f32 i.i.d. U[lo,hi) (Philox)."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else device
    if out is None:
        out = torch.empty(n, 4, dtype=torch.float32, device=dev)
    check(_lib.lib().dr_random_actions(n, seed & (2**64 - 1), env_id_offset, step, lo, hi,
                                       ptr(out), _stream(out.device)))
    return out


class _Box:
    """Minimal gym.spaces.Box stand-in (gym/gymnasium are optional)."""

    def __init__(self, low, high, shape, dtype=np.float32):
        self.shape = tuple(shape)
        self.dtype = np.dtype(dtype)
        self.low = np.full(self.shape, low, dtype=self.dtype)
        self.high = np.full(self.shape, high, dtype=self.dtype)
        self._rng = np.random.default_rng()

    def sample(self):
        lo = np.where(np.isfinite(self.low), self.low, -1.0)
        hi = np.where(np.isfinite(self.high), self.high, 1.0)
        return self._rng.uniform(lo, hi).astype(self.dtype)

    def contains(self, x):
        x = np.asarray(x)
        return x.shape == self.shape and bool(np.all(x >= self.low) and np.all(x <= self.high))

    def seed(self, seed=None):
        self._rng = np.random.default_rng(seed)
        return [seed]

    def __repr__(self):
        return f"Box({self.low.min()}, {self.high.max()}, {self.shape}, {self.dtype})"


def make_box(low, high, shape, dtype=np.float32):
    """gymnasium.spaces.Box if importable, then gym's, else a stand-in."""
    for mod in ("gymnasium", "gym"):
        try:
            spaces = __import__(mod + ".spaces", fromlist=["Box"])
            return spaces.Box(low=low, high=high, shape=shape, dtype=dtype)
        except Exception:
            continue
    return _Box(low, high, shape, dtype)


class DroneGymEnv:
    """Single-env drop-in for the reference's DroneGymEnv (drone.py:254-274),
    backed by a one-env GPU batch with raw (non-auto-reset) semantics:
    reset() -> obs (15,) f32; step(a) -> (obs, reward float, done bool, {})."""

    metadata = {"render_modes": []}

    def __init__(self, dt: float = DT, device=None, seed: int | None = None,
                 dtype: torch.dtype = torch.float64):
        if dt != DT:
            raise ValueError("only the reference dt=0.02 is supported")
        seed = int(np.random.randint(0, 2**31 - 1)) if seed is None else seed
        self._b = DroneBatch(1, "gym", dtype=dtype, device=device, seed=seed,
                             auto_reset=False)
        self.mass, self.g, self.dt = MASS, G, DT
        self.I = np.array(INERTIA)
        self.arm_length, self.k_yaw, self.max_steps = ARM_LENGTH, K_YAW, MAX_STEPS
        self.observation_space = make_box(-np.inf, np.inf, (15,), np.float32)
        self.action_space = make_box(0, MOTOR_MAX, (4,), np.float32)

    def reset(self):
        return self._b.reset_host()[0].copy()

    def step(self, action):
        # one launch + one sync: the kernel reads the action from and writes
        # its outputs to pinned host memory (DroneBatch.step_host)
        o = self._b.step_host(np.asarray(action, np.float32).reshape(1, 4))
        return (o["obs"][0].copy(), float(o["rew"][0]), bool(o["done"][0]), {})

    def _vec(self, f):
        return self._b.get_host(f)[0]

    pos = property(lambda self: self._vec("pos"))
    vel = property(lambda self: self._vec("vel"))
    euler = property(lambda self: self._vec("euler"))
    omega = property(lambda self: self._vec("omega"))
    target = property(lambda self: self._vec("target"))
    current_step = property(lambda self: int(self._b.get_host("current_step")[0]))
    ep_num = property(lambda self: int(self._b.get_host("ep_num")[0]))
    eps = property(lambda self: float(self._b.get_host("eps")[0]))

    # ---- recording (drone.py:189-248; test.py:9-21) -------------------------
    def _recorder(self):
        if getattr(self, "_rec", None) is None:
            from .render import DroneRecorder
            self._rec = DroneRecorder()
        return self._rec

    def start_record(self, filename="drone_run.mp4", dpi=200, fps=20, bitrate=-1):
        """Start a GIF (PillowWriter) of the frames render() draws."""
        self._recorder().start_record(filename, dpi=dpi, fps=fps, bitrate=bitrate)

    def stop_record(self):
        """Finish and save the recording."""
        self._recorder().stop_record()

    def render(self, mode="human", close=False, ax=None):
        """DroneGymEnv.render(mode="human", close=False) (drone.py:273-274):
        draw the drone (motors, arms, centre) and the target in 3-D from the
        device state; grabs a frame when recording.  `mode` and `close` are
        accepted as the reference accepts them (it ignores both); `ax` is this
        build's optional target axes.  Returns the (4, 3) motor positions."""
        return self._recorder().render(self.pos, self.euler, self.target, self.arm_length, ax)

    def close(self):
        if getattr(self, "_rec", None) is not None:
            self._rec.close()
        self._b.close()
