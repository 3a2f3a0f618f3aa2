"""The "rk4" variant's step law without a GPU: the
NumPy restatement tests/rk4_ref.py is fourth order, agrees to first order
with the reference's Euler-angle dynamics, passes through gimbal lock, keeps
the quaternion on the unit sphere and resets as the gym env does; the Euler
<-> quaternion helpers round-trip; and the argument rules of the C ABI,
DroneBatch and PPOConfig that run before any device work."""
import ctypes
import os

import numpy as np
import pytest

import rk4_ref
from oracle import cref

HOVER = 9.81 / 4


def _tumbling(rng, n, S=np.float64, w_scale=3.0):
    return {"pos": (rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 5.0]).astype(S),
            "vel": rng.normal(0, 1, (n, 3)).astype(S),
            "quat": rk4_ref.random_unit_quat(rng, n, S),
            "omega": (w_scale * rng.normal(0, 1, (n, 3))).astype(S),
            "target": np.tile(np.array([0, 0, 1.0], S), (n, 1)),
            "step": np.zeros(n, np.int32)}


def _copy(s):
    return {k: v.copy() for k, v in s.items()}


def _run(s0, actions, dt, sub):
    """Every 20-ms action held over `sub` steps of dt / sub."""
    s = _copy(s0)
    for a in actions:
        for _ in range(sub):
            rk4_ref.integrate(s, a, dt / sub)
    return s


def _rms(a, b):
    return float(np.sqrt(np.mean((a - b) ** 2)))


def _quat_diff(a, b):
    """Difference of two attitudes as quaternions (q and -q are one attitude)."""
    sign = np.sign(np.sum(a * b, axis=1, keepdims=True))
    return a - sign * b


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_fourth_order(seed):
    """RMS error against the same law at dt / 32 falls by 2^4 per halving of
    dt, within [2^3.5, 2^4.5] (what separates order 4 from 3 and 5), for each
    of p, v, q, omega."""
    rng = np.random.default_rng(seed)
    n, steps = 1000, 8
    s0 = _tumbling(rng, n)
    acts = [(HOVER + rng.uniform(-1, 1, (n, 4))).astype(np.float32) for _ in range(steps)]
    ref = _run(s0, acts, 0.02, 32)
    err = {}
    for sub in (1, 2, 4):
        s = _run(s0, acts, 0.02, sub)
        err[sub] = {k: _rms(s[k], ref[k]) for k in ("pos", "vel", "quat", "omega")}
    for k in ("pos", "vel", "quat", "omega"):
        for a, b in ((1, 2), (2, 4)):
            ratio = err[a][k] / err[b][k]
            print(f"seed {seed} {k}: dt 0.02/{a} -> 0.02/{b} error ratio {ratio:.3f} "
                  f"({err[a][k]:.3e} -> {err[b][k]:.3e})")
            assert 2 ** 3.5 <= ratio <= 2 ** 4.5, (k, a, b, ratio)


def _gym_euler_law(s, action, dt):
    """The reference's step (drone.py:81-139: ZYX Euler angles, one forward-
    Euler step) restated with a dt argument, f64, in place."""
    thr, phi, theta, psi = rk4_ref.motor_mix(action)
    T = thr.astype(np.float64)
    tau = [rk4_ref.FACTOR * phi.astype(np.float64), rk4_ref.FACTOR * theta.astype(np.float64),
           (rk4_ref.K_YAW32 * psi).astype(np.float64)]
    e, w = s["euler"], s["omega"]
    sph, cph = np.sin(e[:, 0]), np.cos(e[:, 0])
    sth, cth = np.sin(e[:, 1]), np.cos(e[:, 1])
    sps, cps = np.sin(e[:, 2]), np.cos(e[:, 2])
    acc = np.stack([(cps * sth * cph + sps * sph) * T, (sps * sth * cph - cps * sph) * T,
                    -rk4_ref.G + cth * cph * T], 1)
    s["vel"] += acc * dt
    s["pos"] += s["vel"] * dt
    tth = sth / cth
    w0, w1, w2 = w[:, 0].copy(), w[:, 1].copy(), w[:, 2].copy()
    ed = np.stack([w0 + sph * tth * w1 + cph * tth * w2, cph * w1 - sph * w2,
                   sph / cth * w1 + cph / cth * w2], 1)
    s["euler"] = e + ed * dt
    wd = np.stack([(tau[0] - (rk4_ref.IYY - rk4_ref.IZZ) * w1 * w2) / rk4_ref.IXX,
                   (tau[1] - (rk4_ref.IZZ - rk4_ref.IXX) * w0 * w2) / rk4_ref.IYY,
                   (tau[2] - (rk4_ref.IXX - rk4_ref.IYY) * w0 * w1) / rk4_ref.IZZ], 1)
    s["omega"] = w + wd * dt


def test_first_order_agreement_with_the_reference_dynamics():
    """The Euler-angle law sub-stepped 100x and 1000x approaches the rk4
    result: one ODE, two parametrisations.  Its error falls 5-20x (first
    order: 10x) from 100 to 1000 sub-steps."""
    from drone_rl_amd.env import euler_to_quat
    rng = np.random.default_rng(4)
    n, steps = 200, 4
    euler = rng.uniform(-0.5, 0.5, (n, 3))
    base = {"pos": rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 5.0], "vel": rng.normal(0, 1, (n, 3)),
            "omega": rng.normal(0, 1, (n, 3)), "target": np.zeros((n, 3)),
            "step": np.zeros(n, np.int32)}
    acts = [(HOVER + rng.uniform(-0.3, 0.3, (n, 4))).astype(np.float32) for _ in range(steps)]
    r = _copy(base)
    r["quat"] = euler_to_quat(euler)
    for a in acts:
        rk4_ref.integrate(r, a, 0.02)
    err = {}
    for sub in (100, 1000):
        g = _copy(base)
        g["euler"] = euler.copy()
        for a in acts:
            for _ in range(sub):
                _gym_euler_law(g, a, 0.02 / sub)
        assert np.abs(g["euler"][:, 1]).max() < 1.2       # away from gimbal lock
        err[sub] = {"pos": np.abs(g["pos"] - r["pos"]).max(),
                    "quat": np.abs(_quat_diff(euler_to_quat(g["euler"]), r["quat"])).max(),
                    "omega": np.abs(g["omega"] - r["omega"]).max()}
    for k in ("pos", "quat", "omega"):
        ratio = err[100][k] / err[1000][k]
        print(f"{k}: error {err[100][k]:.3e} at 100, {err[1000][k]:.3e} at 1000 sub-steps, "
              f"ratio {ratio:.2f}")
        assert 5.0 <= ratio <= 20.0, (k, ratio)
    assert err[1000]["pos"] < 1e-3


def test_gimbal_lock_is_an_ordinary_state():
    """From pitch = pi/2 exactly (1 / cos(theta) of the Euler law is 1.6e16
    there) 8 steps stay finite and within 1e-4 of the dt / 32 solution."""
    from drone_rl_amd.env import euler_to_quat
    rng = np.random.default_rng(5)
    n, steps = 256, 8
    # body rates of about 1 rad/s, as in the first-order test: the subject is
    # the singularity, not fast tumbling (the step's error grows as
    # (|omega| dt)^5, which test_fourth_order covers at 3 rad/s)
    s0 = _tumbling(rng, n, w_scale=1.0)
    e = np.stack([rng.uniform(-1, 1, n), np.full(n, np.pi / 2), rng.uniform(-1, 1, n)], 1)
    s0["quat"] = euler_to_quat(e)
    acts = [(HOVER + rng.uniform(-1, 1, (n, 4))).astype(np.float32) for _ in range(steps)]
    a, b = _run(s0, acts, 0.02, 1), _run(s0, acts, 0.02, 32)
    worst = max(np.abs(a[k] - b[k]).max() for k in ("pos", "vel", "quat", "omega"))
    print(f"gimbal lock: max deviation from the dt/32 solution {worst:.3e}")
    assert all(np.isfinite(a[k]).all() for k in ("pos", "vel", "quat", "omega"))
    assert worst <= 1e-4


@pytest.mark.parametrize("S", [np.float64, np.float32])
def test_unit_norm_after_every_step(S):
    rng = np.random.default_rng(6)
    n = 1000
    s = _tumbling(rng, n, S, w_scale=10.0)
    ulp = np.finfo(S).eps
    worst = 0.0
    for t in range(20):
        a = rng.uniform(0, 7.3575, (n, 4)).astype(np.float32)
        rk4_ref.integrate(s, a, 0.02)
        q = s["quat"].astype(np.longdouble)
        dev = np.abs((q * q).sum(1) - 1).max()
        worst = max(worst, float(dev / ulp))
        assert dev <= 4 * ulp, (t, float(dev / ulp))
    print(f"{np.dtype(S).name}: | |q|^2 - 1 | <= {worst:.2f} ulp over 20 steps")


def test_euler_quaternion_helpers_round_trip():
    from drone_rl_amd.env import euler_to_quat, quat_to_euler
    rng = np.random.default_rng(7)
    e = np.stack([rng.uniform(-np.pi, np.pi, 2000), rng.uniform(-1.55, 1.55, 2000),
                  rng.uniform(-np.pi, np.pi, 2000)], 1)
    q = euler_to_quat(e)
    np.testing.assert_allclose((q * q).sum(1), 1.0, rtol=0, atol=1e-15)
    np.testing.assert_allclose(quat_to_euler(q), e, rtol=0, atol=1e-12)
    np.testing.assert_allclose(quat_to_euler(-q), e, rtol=0, atol=1e-12)
    np.testing.assert_array_equal(euler_to_quat(np.zeros(3)), [1, 0, 0, 0])
    np.testing.assert_array_equal(quat_to_euler(np.array([1.0, 0, 0, 0])), [0, 0, 0])
    # body z in the world frame is the gym's rotation-matrix column 2
    a, b, c, d = q.T
    sph, cph, sth, cth, sps, cps = (f(e[:, k]) for k in range(3) for f in (np.sin, np.cos))
    np.testing.assert_allclose(2 * (b * d + a * c), cps * sth * cph + sps * sph, atol=1e-14)
    np.testing.assert_allclose(2 * (c * d - a * b), sps * sth * cph - cps * sph, atol=1e-14)
    np.testing.assert_allclose(1 - 2 * (b * b + c * c), cth * cph, atol=1e-14)


@pytest.mark.parametrize("S", [np.float64, np.float32])
def test_reset_is_the_gyms_with_the_identity_attitude(S):
    rng = np.random.default_rng(8)
    n = 64
    s = _tumbling(rng, n, S)
    s["ep_num"] = rng.integers(1990, 2010, n).astype(np.int64)
    s["eps"] = rng.uniform(0, 1, n)
    g = {"pos": np.zeros((n, 3)), "vel": np.ones((n, 3)), "euler": np.ones((n, 3)),
         "omega": np.ones((n, 3)), "target": np.zeros((n, 3)), "step": np.full(n, 7, np.int32),
         "ep_num": s["ep_num"].copy(), "eps": s["eps"].copy()}
    u = rng.uniform(0, 1, (n, 5))
    mask = rng.uniform(size=n) < 0.5
    before = _copy(s)
    rk4_ref.rk4_reset(s, u, mask)
    cref.gym_reset(g, u)
    np.testing.assert_array_equal(s["quat"][mask], np.tile(np.array([1, 0, 0, 0], S), (mask.sum(), 1)))
    np.testing.assert_array_equal(s["pos"][mask], g["pos"][mask].astype(S))
    np.testing.assert_array_equal(s["target"][mask], g["target"][mask].astype(S))
    np.testing.assert_array_equal(s["ep_num"][mask], g["ep_num"][mask])
    np.testing.assert_array_equal(s["eps"][mask], g["eps"][mask])
    assert not s["vel"][mask].any() and not s["omega"][mask].any() and not s["step"][mask].any()
    for k in ("pos", "vel", "quat", "omega", "target", "ep_num", "eps"):
        np.testing.assert_array_equal(s[k][~mask], before[k][~mask])
    obs = rk4_ref.rk4_obs(s)
    assert obs.shape == (n, 16) and obs.dtype == np.float32
    np.testing.assert_array_equal(obs[mask, 6:10], np.tile(np.float32([1, 0, 0, 0]), (mask.sum(), 1)))


def test_step_counts_rewards_and_ends_as_the_gym():
    """Free fall from rest, level: the law's closed form (constant
    acceleration is integrated exactly by RK4 up to rounding), the reward
    form, the bonus radius, the crash rule and the step limit."""
    z0 = np.array([1.0, 0.001, 1.0, 1.0])
    s = {"pos": np.stack([np.zeros(4), np.zeros(4), z0], 1), "vel": np.zeros((4, 3)),
         "quat": np.tile([1.0, 0, 0, 0], (4, 1)), "omega": np.zeros((4, 3)),
         "target": np.array([[0, 0, 3.0], [0, 0, 3.0], [0, 0, 0.99], [0, 0, 3.0]]),
         "step": np.array([3, 3, 3, 199], np.int32)}
    obs, rew, done, crash = rk4_ref.rk4_step(s, np.zeros((4, 4), np.float32))
    np.testing.assert_allclose(s["pos"][:, 2], z0 - 0.5 * 9.81 * 0.02 ** 2, rtol=0, atol=1e-15)
    np.testing.assert_allclose(s["vel"][:, 2], -9.81 * 0.02, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(s["quat"], np.tile([1.0, 0, 0, 0], (4, 1)))
    np.testing.assert_array_equal(crash, [False, True, False, False])
    np.testing.assert_array_equal(done, [False, True, False, True])
    np.testing.assert_array_equal(s["step"], [4, 4, 4, 200])
    d = np.abs(s["pos"][:, 2] - s["target"][:, 2])
    assert d[2] < 0.05 < d[0]
    want = 0.01 * -d + np.array([0, 0, 1.0, 0])
    np.testing.assert_array_equal(rew, want.astype(np.float32))
    assert obs.shape == (4, 16) and obs.dtype == np.float32
    np.testing.assert_array_equal(obs[:, 13:], (s["target"] - s["pos"]).astype(np.float32))
    # NaN ends at the step limit, not before
    s["pos"][0, 0] = np.nan
    _, _, done, crash = rk4_ref.rk4_step(s, np.zeros((4, 4), np.float32))
    assert not done[0] and not crash[0]


# ---- argument rules (no device work) ---------------------------------------
def test_ids_and_tables():
    from drone_rl_amd import _lib
    from drone_rl_amd.env import OBS_DIM, RESET_UNIFORMS
    assert _lib.DR_VARIANT_RK4 == 5 and _lib.FIELDS["quat"] == 12
    assert _lib.ABI_VERSION == 16
    assert OBS_DIM["rk4"] == 16 and RESET_UNIFORMS["rk4"] == 5
    hdr = open(os.path.join(os.path.dirname(__file__), "..", "include", "dronerl.h")).read()
    assert "DR_VARIANT_RK4 = 5" in hdr and "DR_FIELD_QUAT = 12" in hdr
    assert "#define DR_ABI_VERSION 16" in hdr


def test_variant_and_field_rules_need_no_device():
    from drone_rl_amd import DroneBatch
    from drone_rl_amd.env import check_field, check_smoothing, check_tag
    from drone_rl_amd.ppo import PPOConfig
    with pytest.raises(ValueError, match="unknown variant"):
        DroneBatch(4, "rk5")
    with pytest.raises(ValueError, match="unknown variant"):
        PPOConfig(variant="rk5")
    assert PPOConfig(variant="rk4", num_envs=321).variant == "rk4"
    for variant in ("gym", "vectorized", "moving", "smooth", "tag"):
        with pytest.raises(ValueError, match="quat"):
            check_field(variant, "quat")
    check_field("rk4", "quat")
    check_field("rk4", "euler")
    # the smooth and tag parameters treat "rk4" like "gym"
    check_smoothing("rk4", 1.0, 0.0)
    assert check_tag("rk4", None, None, 321, 1) == check_tag("gym", None, None, 321, 1)
    for kw in (dict(motor_alpha=0.5), dict(rate_penalty=0.1), dict(tag_radius=0.3),
               dict(crash_penalty=0.1)):
        with pytest.raises(ValueError):
            DroneBatch(4, "rk4", **kw)
        with pytest.raises(ValueError):
            PPOConfig(variant="rk4", **kw)


def test_abi_refusals_before_any_device_call():
    from drone_rl_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 4)()
    for fn in (L.dr_get_state, L.dr_set_state):
        assert fn(None, _lib.FIELDS["quat"], buf, None) == _lib.DR_ERR_INVALID
        assert "null handle" in _lib.last_error()
    ids = (ctypes.c_int32 * 1)()
    assert L.dr_gather_state(None, _lib.FIELDS["quat"], ids, 1, buf, None) == _lib.DR_ERR_INVALID

    def create(variant, n=4):
        cfg = _lib.dr_config(num_envs=n, variant=variant, state_dtype=0, rng_mode=0,
                             auto_reset=1, device=0, max_steps=0, seed=1, env_id_offset=0,
                             dt=0.02)
        h = ctypes.c_void_p()
        rc = L.dr_create(ctypes.byref(cfg), ctypes.byref(h))
        # dr_last_error keeps the LAST error: after a call that succeeded it
        # still holds an earlier call's message, which is not this call's
        msg = _lib.last_error() if rc != _lib.DR_OK else ""
        if h.value:
            L.dr_destroy(h)
        return rc, msg
    rc, msg = create(6)
    assert rc == _lib.DR_ERR_INVALID and "unknown variant" in msg
    # the variant is known: accepted, or no device to run it on
    rc, msg = create(_lib.DR_VARIANT_RK4)
    assert rc in (_lib.DR_OK, _lib.DR_ERR_HIP) and "unknown variant" not in msg, (rc, msg)
    # an odd batch is fine here (only "tag" pairs envs)
    rc, msg = create(_lib.DR_VARIANT_RK4, 3)
    assert rc in (_lib.DR_OK, _lib.DR_ERR_HIP), (rc, msg)
