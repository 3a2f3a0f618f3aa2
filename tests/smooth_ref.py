"""NumPy restatement of the "smooth" variant's step law (DESIGN.md section
14) around the CPU oracle's gym step: the motor lag and the action-rate
penalty in np.float32 (one IEEE operation per numpy call, no FMA), the
dynamics from oracle.cref.gym_step on the lagged forces."""
import numpy as np

from oracle import cref

HOVER = np.float32(1.0 * 9.81 / 4)


def smooth_step(state, command, alpha, rate_penalty):
    """One step for n envs.  `state`: cref.gym_step's dict plus "motor"
    (n,4) f32, all mutated in place.  Returns obs (n,19) f32, reward (n,) f32,
    done (n,) bool."""
    a = np.ascontiguousarray(command, np.float32)
    f = np.ascontiguousarray(state["motor"], np.float32)
    alpha, lam = np.float32(alpha), np.float32(rate_penalty)
    d = a - f
    s = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3]
    b = np.float32(1.0) - alpha
    f = b * f + alpha * a
    obs, rew, done = cref.gym_step(state, f)
    rew = rew.astype(np.float32)
    if lam != 0:
        rew = rew - lam * s
    state["motor"] = f
    return np.concatenate([obs, f], axis=1), rew, done
