"""NumPy restatement of the gym env's wind option (DESIGN.md section 17;
dr_set_wind) around the CPU oracle's gym step: the Philox draws through
oracle.cref.philox_np, the gust's AR(1) update in np.float32 (one IEEE
operation per numpy call, no FMA), the drag impulse on the velocity in f64,
then oracle.cref.gym_step, unchanged, on the updated velocity."""
import math

import numpy as np

from oracle import cref
from philox_ref import blocks as _blocks, pm1 as _pm1

DT = 0.02
TAG_RESET = 0x52000000
TAG_GUST = 0x47000000


def mean_wind(seed, gids, ep, wind_speed):
    """(n,3) f32: the mean wind of envs `gids` in episodes `ep`."""
    r = _blocks(seed, gids, ep, TAG_RESET | 2)
    return np.float32(wind_speed) * _pm1(r[:, :3])


def gust_noise(seed, gids, ep, step):
    """(n,3) f32 in [-1, 1): the gust noise of a step from counter `step`."""
    r = _blocks(seed, gids, ep, TAG_GUST | np.asarray(step).astype(np.int64))
    return _pm1(r[:, :3])


def gust_coefficients(gust_sigma, gust_rate):
    """b = 1 - beta in f32; c = sigma sqrt(3 (1 - b^2)) in f64, then f32."""
    b = np.float32(1.0) - np.float32(gust_rate)
    c = np.float32(float(np.float32(gust_sigma)) * math.sqrt(3.0 * (1.0 - float(b) * float(b))))
    return b, c


def gust_update(g, xi, b, c):
    """g <- b g + c xi on f32 arrays, three roundings per element."""
    g = np.asarray(g, np.float32)
    xi = np.asarray(xi, np.float32)
    return np.float32(b) * g + np.float32(c) * xi


def wind_step(state, action, params, seed, gids, fault=None):
    """One step for n envs.  `state`: cref.gym_step's dict plus "wind" (n,6)
    f32 (mean wind xyz, gust xyz) and "ep_num" (n,), mutated in place;
    `params`: dict of drag, wind_speed, gust_sigma, gust_rate.  Returns obs
    (n,15) f32, reward (n,) f64, done (n,) bool: the gym's.

    `fault` selects a deliberately WRONG law, for the tests that show the
    checks can fail: "no_gust" leaves the gust out of the air's velocity,
    "drag_after" takes the drag impulse on the velocity the gym step leaves
    (and carries it into the position)."""
    w6 = np.ascontiguousarray(state["wind"], np.float32)
    b, c = gust_coefficients(params["gust_sigma"], params["gust_rate"])
    xi = gust_noise(seed, gids, state["ep_num"], state["step"])
    g = gust_update(w6[:, 3:], xi, b, c)
    w = (w6[:, :3] if fault == "no_gust" else w6[:, :3] + g).astype(np.float64)
    k = np.float64(np.float32(params["drag"]))
    state["wind"] = np.concatenate([w6[:, :3], g], 1)
    if fault == "drag_after":
        out = cref.gym_step(state, action)
        dv = (k * (w - state["vel"])) * DT
        state["vel"] = state["vel"] + dv
        state["pos"] = state["pos"] + dv * DT
        return out
    v = state["vel"]
    state["vel"] = np.ascontiguousarray(v + (k * (w - v)) * DT)
    return cref.gym_step(state, action)
