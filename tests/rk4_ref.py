"""NumPy restatement of the "rk4" variant's step law:
the gym env's task on the state (p, v, unit quaternion q = (w, x, y, z) body
-> world, body rates omega), advanced by one classic RK4 step with the action
held, then q normalised.  One numpy call per IEEE operation, no FMA, generic
over np.float64 and np.float32 (the dtype of state["pos"]); `dt` is an
argument.  This file fixes the expression order; the kernels follow it.
Resets come from oracle.cref.gym_reset with the attitude replaced."""
import numpy as np

from oracle import cref

G = 9.81
MASS = 1.0
IXX, IYY, IZZ = 0.005, 0.005, 0.01
FACTOR = 0.5 / 1.4142135623730951        # arm length / sqrt(2)
K_YAW32 = np.float32(0.01)
VEC = ("pos", "vel", "quat", "omega", "target")


def motor_mix(action):
    """The gym's f32 motor mixes: thrust sum and the three torque sums."""
    a = np.ascontiguousarray(action, np.float32)
    a0, a1, a2, a3 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return (((a0 + a1) + a2) + a3, ((a0 + a1) - a2) - a3,
            ((-a0 + a1) + a2) - a3, ((a0 - a1) + a2) - a3)


def deriv(y, T, tau, S):
    """dy/dt at y = (p[3], v[3], q[4], w[3]), each a list of (n,) arrays."""
    p, v, q, w = y
    a, b, c, d = q
    w0, w1, w2 = w
    one, two, half = S(1), S(2), S(0.5)
    rM, rIx, rIy, rIz = one / S(MASS), one / S(IXX), one / S(IYY), one / S(IZZ)
    r02 = two * (b * d + a * c)
    r12 = two * (c * d - a * b)
    r22 = one - two * (b * b + c * c)
    vd = [(r02 * T) * rM, (r12 * T) * rM, S(-G) + (r22 * T) * rM]
    qd = [half * ((((-b) * w0) - c * w1) - d * w2),
          half * ((a * w0 + c * w2) - d * w1),
          half * ((a * w1 - b * w2) + d * w0),
          half * ((a * w2 + b * w1) - c * w0)]
    wd = [(tau[0] - (S(IYY - IZZ) * w1) * w2) * rIx,
          (tau[1] - (S(IZZ - IXX) * w0) * w2) * rIy,
          (tau[2] - (S(IXX - IYY) * w0) * w1) * rIz]
    return [list(v), vd, qd, wd]


def _flat(y):
    return [x for part in y for x in part]


def _shape(f):
    return [f[0:3], f[3:6], f[6:10], f[10:13]]


def integrate(state, action, dt):
    """The RK4 step and the normalisation on state's pos / vel / quat / omega
    (in place).  No reward, no counters."""
    S = state["pos"].dtype.type
    thr, phi, theta, psi = motor_mix(action)
    T = thr.astype(S)
    tau = [S(FACTOR) * phi.astype(S), S(FACTOR) * theta.astype(S), (K_YAW32 * psi).astype(S)]
    y = [state["pos"][:, k].copy() for k in range(3)] + \
        [state["vel"][:, k].copy() for k in range(3)] + \
        [state["quat"][:, k].copy() for k in range(4)] + \
        [state["omega"][:, k].copy() for k in range(3)]
    dt = S(dt)
    h2 = dt * S(0.5)
    h6 = dt / S(6)
    two = S(2)
    with np.errstate(all="ignore"):
        k1 = _flat(deriv(_shape(y), T, tau, S))
        k2 = _flat(deriv(_shape([yj + h2 * kj for yj, kj in zip(y, k1)]), T, tau, S))
        k3 = _flat(deriv(_shape([yj + h2 * kj for yj, kj in zip(y, k2)]), T, tau, S))
        k4 = _flat(deriv(_shape([yj + dt * kj for yj, kj in zip(y, k3)]), T, tau, S))
        y = [yj + h6 * ((a + two * b) + (two * c + d))
             for yj, a, b, c, d in zip(y, k1, k2, k3, k4)]
        qa, qb, qc, qd = y[6:10]
        n2 = ((qa * qa + qb * qb) + qc * qc) + qd * qd
        r = S(1) / np.sqrt(n2)
        y[6:10] = [qa * r, qb * r, qc * r, qd * r]
    for k in range(3):
        state["pos"][:, k] = y[k]
        state["vel"][:, k] = y[3 + k]
        state["omega"][:, k] = y[10 + k]
    for k in range(4):
        state["quat"][:, k] = y[6 + k]


def rk4_obs(state):
    """(n,16) f32: p, v, q, omega, target - p."""
    return np.concatenate([state["pos"], state["vel"], state["quat"], state["omega"],
                           state["target"] - state["pos"]], axis=1).astype(np.float32)


def rk4_step(state, action, dt=0.02, max_steps=200):
    """One step without auto-reset.  `state`: pos / vel / omega / target (n,3)
    and quat (n,4) in one dtype, step (n,) i32; mutated in place.  Returns
    obs (n,16) f32, reward (n,) f32, done (n,) bool, crash (n,) bool."""
    S = state["pos"].dtype.type
    integrate(state, action, dt)
    with np.errstate(all="ignore"):
        p, t = state["pos"], state["target"]
        dx, dy, dz = p[:, 0] - t[:, 0], p[:, 1] - t[:, 1], p[:, 2] - t[:, 2]
        dist = np.sqrt((dx * dx + dy * dy) + dz * dz)
        rew = S(0.01) * -dist
        rew = np.where(dist < S(0.05), rew + S(1), rew)
        pn2 = (p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2]
        crash = (p[:, 2] < S(0)) | (pn2 > S(2500))       # NaN compares false
    state["step"] = (state["step"] + 1).astype(np.int32)
    done = crash | (state["step"] >= max_steps)
    return rk4_obs(state), rew.astype(np.float32), done, crash


def rk4_reset(state, u, mask=None):
    """DroneEnv.reset for the rows in `mask` (all when None) given their rows
    of the (n,5) uniforms: oracle.cref.gym_reset's position, target and
    counters, q = (1, 0, 0, 0), v = omega = 0.  state also carries ep_num
    (n,) i64 and eps (n,) f64."""
    n = len(state["pos"])
    idx = np.arange(n) if mask is None else np.nonzero(mask)[0]
    if len(idx) == 0:
        return
    S = state["pos"].dtype.type
    m = len(idx)
    sub = {"pos": np.zeros((m, 3)), "vel": np.zeros((m, 3)), "euler": np.zeros((m, 3)),
           "omega": np.zeros((m, 3)), "target": np.zeros((m, 3)),
           "step": np.zeros(m, np.int32), "ep_num": state["ep_num"][idx].astype(np.int64),
           "eps": np.ascontiguousarray(state["eps"][idx], np.float64)}
    cref.gym_reset(sub, np.asarray(u, np.float64)[idx])
    state["pos"][idx] = sub["pos"].astype(S)
    state["target"][idx] = sub["target"].astype(S)
    state["vel"][idx] = 0
    state["omega"][idx] = 0
    state["quat"][idx] = np.array([1, 0, 0, 0], S)
    state["step"][idx] = 0
    state["ep_num"][idx] = sub["ep_num"]
    state["eps"][idx] = sub["eps"]


def rk4_env_step(state, action, u, dt=0.02, max_steps=200):
    """One auto-reset step (DummyVecEnv): the step, then a reset of the done
    rows from their rows of `u`.  Returns obs (post-reset), reward, done and
    the terminal obs (the pre-reset obs; meaningful on done rows)."""
    term, rew, done, _ = rk4_step(state, action, dt, max_steps)
    rk4_reset(state, u, done)
    return rk4_obs(state), rew, done, term


def random_unit_quat(rng, n, S=np.float64):
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return q.astype(S)
