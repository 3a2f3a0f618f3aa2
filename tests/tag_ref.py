"""NumPy restatement of the "tag" variant's step law
around the CPU oracle's gym step: the dynamics and the step counters come
from oracle.cref.gym_step, each drone on its own action; the crash flag, the
pair's common end, the distance, the zero-sum reward and the 19-d obs are
recomputed here in np.float64 (one IEEE operation per numpy call, no FMA) in
the operation order of the section, the crash penalty in np.float32."""
import numpy as np

from oracle import cref


def tag_step(state, action, tag_radius, crash_penalty, max_steps=200):
    """One step for n drones (n even; rows 2j pursue, rows 2j+1 evade).
    `state`: cref.gym_step's dict, mutated in place (its "target" is carried,
    never read by the law).  Returns obs (n,19) f32, reward (n,) f32, done
    (n,) bool, crash (n,) bool (the drone's own)."""
    n = len(action)
    assert n % 2 == 0
    obs15, _, _ = cref.gym_step(state, action)
    pos, vel = state["pos"], state["vel"]
    x, y, z = pos[:, 0], pos[:, 1], pos[:, 2]
    crash = (z < 0) | ((x * x + y * y) + z * z > 2500.0)
    own_done = crash | (state["step"] >= max_steps)
    swap = np.arange(n) ^ 1
    ppos, pvel = pos[swap], vel[swap]
    done = own_done | own_done[swap]
    dx, dy, dz = x - ppos[:, 0], y - ppos[:, 1], z - ppos[:, 2]
    d = np.sqrt((dx * dx + dy * dy) + dz * dz)
    g = 0.01 * (-d)
    g = np.where(d < np.float64(np.float32(tag_radius)), g + 1.0, g)
    sigma = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
    r = np.where(sigma > 0, g, -g)
    rf = r.astype(np.float32)
    c = np.float32(crash_penalty)
    if c != 0:
        rf = np.where(crash, rf - c, rf).astype(np.float32)
    obs = np.concatenate([obs15[:, :12], (ppos - pos).astype(np.float32),
                          (pvel - vel).astype(np.float32),
                          sigma.astype(np.float32)[:, None]], axis=1)
    return obs, rf, done, crash


def tag_random_state(n, rng, tag_radius, z0=0.5):
    """Tumbling states for n drones (test_moving_gpu._random_state's spreads,
    started `z0` m above the ground so that a share of them reaches it within
    30 steps), each evader at its pursuer plus an offset of length
    U[0, 2 * tag_radius) in a uniform direction and with its pursuer's
    velocity, so that the pairs sit on both sides of the radius."""
    s = {"pos": rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, z0 + 0.5],
         "vel": rng.normal(0, 0.5, (n, 3)), "euler": rng.normal(0, 0.2, (n, 3)),
         "omega": rng.normal(0, 0.5, (n, 3)), "target": rng.uniform(-1, 1, (n, 3)) + [0, 0, 1],
         "step": rng.integers(0, 190, n).astype(np.int32)}
    u = rng.normal(size=(n // 2, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    s["pos"][1::2] = s["pos"][0::2] + u * rng.uniform(0, 2 * tag_radius, (n // 2, 1))
    s["vel"][1::2] = s["vel"][0::2]
    return s
