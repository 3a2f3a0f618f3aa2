"""NumPy restatement of the gym env's airframe option (DESIGN.md section 19;
dr_set_airframe): the batched gym step of oracle/drone_np.py
(gym_step_batched), operation for operation, with the option's three changes
-- the motor gains on the command, the reciprocal mass scale on the three
accelerations, the reciprocal inertia scale on the three torques -- and the
per-episode draw through oracle.cref.philox_np.  f32 arithmetic is done in
np.float32, one numpy call per operation (no FMA)."""
import numpy as np

from philox_ref import blocks as _blocks, pm1 as _pm1
from oracle.drone_np import _FACTOR, DT, G, INERTIA, K_YAW, MAX_STEPS

TAG_AIRFRAME = 0x46000000


def airframe(seed, gids, ep, spreads):
    """(n,6) f32: mass scale m, inertia scale s, motor gains g0..g3 of envs
    `gids` in episodes `ep` under spreads (sigma_m, sigma_I, sigma_g)."""
    sm, si, sg = (np.float32(x) for x in spreads)
    one = np.float32(1.0)
    b0 = _pm1(_blocks(seed, gids, ep, TAG_AIRFRAME | 0))
    b1 = _pm1(_blocks(seed, gids, ep, TAG_AIRFRAME | 1))
    out = np.empty((len(b0), 6), np.float32)
    out[:, 0] = one + sm * b0[:, 0]
    out[:, 1] = one + si * b0[:, 1]
    for j in range(4):
        out[:, 2 + j] = one + sg * b1[:, j]
    return out


def airframe_step(state, action, fault=None):
    """One step for n envs.  `state`: gym_step_batched's dict plus "airframe"
    (n,6) f32, mutated in place (the airframe is read only).  Returns obs
    (n,15) f32, reward (n,) f64, done (n,) bool.

    `fault` selects a deliberately WRONG law, for the tests that show the
    checks can fail: "gravity" scales the gravity term by 1/m too, "yaw"
    leaves the yaw torque unscaled by 1/s, "f64_recip" forms 1/m in f64 where
    the law has the f32 divide."""
    s = state
    af = np.ascontiguousarray(s["airframe"], np.float32)
    a = np.asarray(action, dtype=np.float32)
    # 1. the gained command (f32 products)
    a0, a1, a2, a3 = (af[:, 2 + j] * a[:, j] for j in range(4))
    # 2. the reciprocals (f32 divides), then the cast to the state scalar
    im = (np.float32(1.0) / af[:, 0]).astype(np.float64)
    is_ = (np.float32(1.0) / af[:, 1]).astype(np.float64)
    if fault == "f64_recip":
        im = 1.0 / af[:, 0].astype(np.float64)
    thrust = ((a0 + a1) + a2) + a3                      # f32
    # 4. the torques scale by 1/s
    tau_phi = (_FACTOR * (((a0 + a1) - a2) - a3)) * is_         # f64
    tau_th = (_FACTOR * (((-a0 + a1) + a2) - a3)) * is_
    tau_psi = np.float32(K_YAW) * (((a0 - a1) + a2) - a3)       # f32
    tau_psi = tau_psi.astype(np.float64) * (1.0 if fault == "yaw" else is_)
    e = s["euler"]
    cph, sph = np.cos(e[:, 0]), np.sin(e[:, 0])
    cth, sth = np.cos(e[:, 1]), np.sin(e[:, 1])
    cps, sps = np.cos(e[:, 2]), np.sin(e[:, 2])
    T = thrust.astype(np.float64)
    # 3. the accelerations use the reciprocal mass scale
    acc = np.stack([0.0 + ((cps * sth * cph + sps * sph) * T) * im,
                    0.0 + ((sps * sth * cph - cps * sph) * T) * im,
                    -G * (im if fault == "gravity" else 1.0) + ((cth * cph) * T) * im], axis=1)
    s["vel"] += acc * DT
    s["pos"] += s["vel"] * DT
    w = s["omega"].copy()
    tth = np.tan(e[:, 1])
    ed = np.stack([w[:, 0] + (sph * tth) * w[:, 1] + (cph * tth) * w[:, 2],
                   0.0 * w[:, 0] + cph * w[:, 1] + (-sph) * w[:, 2],
                   0.0 * w[:, 0] + (sph / cth) * w[:, 1] + (cph / cth) * w[:, 2]],
                  axis=1)
    s["euler"] += ed * DT
    I = INERTIA
    wd = np.stack([(tau_phi - (I[1] - I[2]) * w[:, 1] * w[:, 2]) / I[0],
                   (tau_th - (I[2] - I[0]) * w[:, 0] * w[:, 2]) / I[1],
                   (tau_psi - (I[0] - I[1]) * w[:, 0] * w[:, 1]) / I[2]],
                  axis=1)
    s["omega"] += wd * DT
    dv = s["pos"] - s["target"]
    d = np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])
    rew = 0.01 * -d + np.where(d < 0.05, 1.0, 0.0)
    p = s["pos"]
    pn = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
    s["step"] = s["step"] + 1
    done = (p[:, 2] < 0) | (pn > 50) | (s["step"] >= MAX_STEPS)
    obs = np.concatenate([s["pos"], s["vel"], s["euler"], s["omega"],
                          s["target"] - s["pos"]], axis=1).astype(np.float32)
    return obs, rew, done
