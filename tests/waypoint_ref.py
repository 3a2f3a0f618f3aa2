"""NumPy restatement of the gym env's waypoint courses (DESIGN.md section 18;
dr_set_waypoints) around the CPU oracle's gym step: oracle.cref.gym_step runs
the physics, crash, step counter and done; the distance to the current
waypoint, the reward and the advance are recomputed here per the law, the
draws through oracle.cref.philox_np."""
import numpy as np

from oracle import cref
from philox_ref import blocks as _blocks

TAG_WAYPOINT = 0x57000000


def waypoint(seed, gids, ep, j, eps):
    """(n,3) f64: waypoint number `j` (>= 1) of envs `gids` in episodes `ep`
    at curriculum `eps`: (eps u_0, eps u_1, eps u_2 + 1.0 + 0.0) of the block's
    first three uniforms u = w * 2^-32, the expressions of the reset's target
    draw."""
    j = np.asarray(j).astype(np.int64) & 0xffffffff
    r = _blocks(seed, gids, ep, TAG_WAYPOINT | j)
    u = r[:, :3].astype(np.float64) * 2.0 ** -32
    eps = np.broadcast_to(np.asarray(eps, np.float64), (len(u),))
    return np.stack([eps * u[:, 0], eps * u[:, 1], eps * u[:, 2] + 1.0 + 0.0], 1)


def distance(pos, target):
    """The gym's sqrt((dx dx + dy dy) + dz dz), f64."""
    d = pos - target
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])


def waypoint_step(state, action, params, seed, gids, fault=None):
    """One step for n envs.  `state`: cref.gym_step's dict plus "waypoint"
    (n,2) i32 (j, q), "ep_num" (n,) and "eps" (n,) f64, mutated in place;
    `params`: dict of reach_radius, reach_bonus.  Returns obs (n,15) f32,
    reward (n,) f64, done (n,) bool, and what the tests look at besides: the
    reached mask and the distance d.

    `fault` selects a deliberately WRONG law, for the tests that show the
    checks can fail: "reach_le" reaches at d <= R, "reward_new" takes the
    reward's distance to the waypoint the step ends with."""
    c = np.ascontiguousarray(state["target"], np.float64)
    state["target"] = c
    obs, _, done = cref.gym_step(state, action)
    R = np.float64(np.float32(params["reach_radius"]))
    B = np.float64(np.float32(params["reach_bonus"]))
    d = distance(state["pos"], c)
    rew = 0.01 * (-d)
    with np.errstate(invalid="ignore"):
        reached = d <= R if fault == "reach_le" else d < R      # NaN compares false
    rew = np.where(reached, rew + B, rew)
    wp = np.array(state["waypoint"], np.int32)
    wp[reached] += 1
    state["waypoint"] = wp
    if reached.any():
        gids = np.atleast_1d(np.asarray(gids)).astype(np.uint64)
        ep = np.broadcast_to(np.asarray(state["ep_num"]), (len(d),))
        eps = np.broadcast_to(np.asarray(state["eps"], np.float64), (len(d),))
        c[reached] = waypoint(seed, gids[reached], ep[reached], wp[reached, 0], eps[reached])
        obs = obs.copy()
        obs[reached, 12:15] = (c[reached] - state["pos"][reached]).astype(np.float32)
    if fault == "reward_new":
        rew = 0.01 * (-distance(state["pos"], c))
        rew = np.where(reached, rew + B, rew)
    return obs, rew, done, reached, d
