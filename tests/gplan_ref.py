"""NumPy restatement of the gradient planner (dr_gplan_*).

Every f64 and f32 operation below is one numpy call (one IEEE rounding, no
FMA), written in the order the kernel follows, so given the same sin / cos
values the device forms the same bits.  The forward step is the gym step in
physics_step_mixed's order with plain divisions; its sin / cos are libm's, the
device's are its own (<= 1 ulp apart), so the restated costs and gradients are
the law's, not the device's bits: the device's cost is pinned bit for bit
against dr_step, its gradient against this file within a bound measured here
(`ulps` moves every sin / cos result by whole ulps).

One plan step for env n, M = f32(3 * 9.81 / 4), clip as in mppi_ref:
    0. dones[n] set: nominal[n] <- hover, f32(9.81 / 4)
    1. start state, f64: p, v, euler, omega = obs[0:12]; target = obs[0:3] +
       obs[12:15]
    2. cost of U: H gym steps on a_h = clip(U[h]); after step h
       c += (((w_pos |p - tgt|^2 + w_vel |v|^2) + w_att |euler|^2) + w_rate |omega|^2)
            + w_effort |a_h - hover|^2
       and after the last one c += w_pos_final |p - tgt|^2 + w_vel_final |v|^2
    3. g = dc/dU by the adjoint (adjoint_step), the casts and the clip taken
       as the identity
    4. Adam from m = s = 0, it = 1 .. I:
       m = b1 m + (1 - b1) g; s = b2 s + (1 - b2) (g g);
       U <- clip(f32(f64(U) - (lr (m / (1 - b1^it))) / (sqrt(s / (1 - b2^it)) + eps)))
       with b^it the running product
    5. cost or a gradient entry of iteration 1 not finite: the nominal stays as
       step 0 left it, the action is clip(U[0])
    6. action = U[0]; nominal[h] <- U[h + 1] for h < H - 1, nominal[H - 1] <- U[H - 1]
"""
import numpy as np

from mppi_ref import HOVER, MOTOR_MAX, START_ROWS, _nominal, bits, clip  # noqa: F401

DT = 0.02
MASS, G = 1.0, 9.81
IXX, IYY, IZZ = 0.005, 0.005, 0.01
FACTOR = 0.5 / 1.4142135623730951
KYAW = np.float32(0.01)
KYAW64 = float(KYAW)
HOVER64 = float(HOVER)
C_YZ, C_ZX, C_XY = IYY - IZZ, IZZ - IXX, IXX - IYY
S_PHI = np.array([1.0, 1.0, -1.0, -1.0])
S_THETA = np.array([-1.0, 1.0, 1.0, -1.0])
S_PSI = np.array([1.0, -1.0, 1.0, -1.0])
FAULTS = (None, "no_lp_dt", "theta_sign", "no_bias_correction", "no_shift")
DEFAULTS = dict(horizon=16, iterations=10, lr=0.05, beta1=0.9, beta2=0.999, adam_eps=1e-8,
                w_pos=1.0, w_vel=0.05, w_att=0.05, w_rate=0.005, w_effort=0.0,
                w_pos_final=10.0, w_vel_final=1.0)


def powers(beta, iterations):
    """beta^1 .. beta^I as the running product: one f64 rounding per step."""
    p, out = 1.0, []
    for _ in range(iterations):
        p = p * float(beta)
        out.append(p)
    return out


def start_state(obs):
    o = np.asarray(obs, np.float32).astype(np.float64)
    return {"p": o[:, 0:3].copy(), "v": o[:, 3:6].copy(), "e": o[:, 6:9].copy(),
            "w": o[:, 9:12].copy(), "tgt": o[:, 0:3] + o[:, 12:15]}


def _sq3(d):
    return (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]


def forward_step(x, a, ulps=None):
    """One gym step on x (dict of (n, 3) f64, replaced, not mutated) with the
    f32 action a (n, 4).  Returns the new state and the tape (sin, cos of the
    old Euler angles, the old omega, T).  ulps (n, 6) moves sin (0:3) and cos
    (3:6) by that many ulps."""
    a = np.asarray(a, np.float32)
    a0, a1, a2, a3 = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    thr = ((a0 + a1) + a2) + a3
    tau_phi = FACTOR * (((a0 + a1) - a2) - a3).astype(np.float64)
    tau_th = FACTOR * (((-a0 + a1) + a2) - a3).astype(np.float64)
    tau_psi = (KYAW * (((a0 - a1) + a2) - a3)).astype(np.float64)
    e, w = x["e"], x["w"]
    sn, cs = np.sin(e), np.cos(e)
    if ulps is not None:
        sn = sn + ulps[:, 0:3] * np.spacing(sn)
        cs = cs + ulps[:, 3:6] * np.spacing(cs)
    sph, sth, sps = sn[:, 0], sn[:, 1], sn[:, 2]
    cph, cth, cps = cs[:, 0], cs[:, 1], cs[:, 2]
    r02 = cps * sth * cph + sps * sph
    r12 = sps * sth * cph - cps * sph
    r22 = cth * cph
    T = thr.astype(np.float64)
    acc = np.stack([0.0 + (r02 * T) / MASS, 0.0 + (r12 * T) / MASS, -G + (r22 * T) / MASS], 1)
    v = x["v"] + acc * DT
    p = x["p"] + v * DT
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    tth = sth / cth
    ed2 = (0.0 * w0 + (sph / cth) * w1) + (cph / cth) * w2
    ed0 = (1.0 * w0 + (sph * tth) * w1) + (cph * tth) * w2
    ed1 = (0.0 * w0 + cph * w1) + (-sph) * w2
    en = e + np.stack([ed0, ed1, ed2], 1) * DT
    wd = np.stack([(tau_phi - C_YZ * w1 * w2) / IXX, (tau_th - C_ZX * w0 * w2) / IYY,
                   (tau_psi - C_XY * w0 * w1) / IZZ], 1)
    wn = w + wd * DT
    return ({"p": p, "v": v, "e": en, "w": wn, "tgt": x["tgt"]},
            {"sn": sn, "cs": cs, "w": w, "T": T})


def adjoint_step(tape, lp, lv, le, lw, fault=None):
    """The adjoint of forward_step: from the adjoint (lp, lv, le, lw) of the
    new state, the step's direct cost gradient already added, the adjoint of
    the old state and (gT, nu): dc/da_j = gT + F (Sphi_j nu0 + Stheta_j nu1) +
    K Spsi_j nu2 without the effort term."""
    sn, cs, w, T = tape["sn"], tape["cs"], tape["w"], tape["T"]
    sph, sth, sps = sn[:, 0], sn[:, 1], sn[:, 2]
    cph, cth, cps = cs[:, 0], cs[:, 1], cs[:, 2]
    w0, w1, w2 = w[:, 0], w[:, 1], w[:, 2]
    sec = 1.0 / cth
    tth = sth * sec
    sg = sph * w1 + cph * w2
    ed1 = cph * w1 - sph * w2
    r02 = cps * sth * cph + sps * sph
    r12 = sps * sth * cph - cps * sph
    r22 = cth * cph
    lvt = lv if fault == "no_lp_dt" else lv + lp * DT
    q0, q1, q2 = lvt[:, 0] * DT, lvt[:, 1] * DT, lvt[:, 2] * DT
    gT = ((r02 * q0 + r12 * q1) + r22 * q2) / MASS
    Tm = T / MASS
    A0 = Tm * (((-cps * sth * sph + sps * cph) * q0 + (-sps * sth * sph - cps * cph) * q1)
               + (-cth * sph) * q2)
    A1 = Tm * (((cps * cth * cph) * q0 + (sps * cth * cph) * q1) + (-sth * cph) * q2)
    A2 = Tm * (-r12 * q0 + r02 * q1)
    mu0, mu1, mu2 = le[:, 0] * DT, le[:, 1] * DT, le[:, 2] * DT
    le0 = (le[:, 0] + A0) + ((mu0 * ed1 * tth - mu1 * sg) + mu2 * ed1 * sec)
    le1 = (le[:, 1] + A1) + (mu0 * sg * sec * sec + mu2 * sg * sec * tth)
    le2 = le[:, 2] + A2
    nu0, nu1, nu2 = lw[:, 0] * DT / IXX, lw[:, 1] * DT / IYY, lw[:, 2] * DT / IZZ
    lw0 = (lw[:, 0] + mu0) + (-C_ZX * w2 * nu1 - C_XY * w1 * nu2)
    lw1 = (lw[:, 1] + ((sph * tth * mu0 + cph * mu1) + sph * sec * mu2)) + \
        (-C_YZ * w2 * nu0 - C_XY * w0 * nu2)
    lw2 = (lw[:, 2] + ((cph * tth * mu0 - sph * mu1) + cph * sec * mu2)) + \
        (-C_YZ * w1 * nu0 - C_ZX * w0 * nu1)
    return (lp, lvt, np.stack([le0, le1, le2], 1), np.stack([lw0, lw1, lw2], 1),
            gT, (nu0, nu1, nu2))


class GplanRef:
    """`fault` selects a deliberately WRONG law, for the tests that show the
    checks can fail: "no_lp_dt" drops lp dt from lvt, "theta_sign" flips the
    sign of Stheta's first entry, "no_bias_correction" divides m and s by 1,
    "no_shift" keeps the new nominal unshifted."""

    def __init__(self, n, fault=None, **kw):
        assert fault in FAULTS and set(kw) <= set(DEFAULTS), kw
        self.n, self.fault = n, fault
        for k, v in DEFAULTS.items():
            setattr(self, k, type(v)(kw.get(k, v)))
        self.H, self.I = self.horizon, self.iterations
        self.s_theta = S_THETA.copy()
        if fault == "theta_sign":
            self.s_theta[0] = 1.0
        self.reset()

    def reset(self):
        self.nominal = np.full((self.n, self.H, 4), HOVER, np.float32)

    def stage_cost(self, x, a):
        d = x["p"] - x["tgt"]
        da = a.astype(np.float64) - HOVER64
        ae = ((da[:, 0] * da[:, 0] + da[:, 1] * da[:, 1]) + da[:, 2] * da[:, 2]) + \
            da[:, 3] * da[:, 3]
        return (((self.w_pos * _sq3(d) + self.w_vel * _sq3(x["v"])) + self.w_att * _sq3(x["e"]))
                + self.w_rate * _sq3(x["w"])) + self.w_effort * ae

    def final_cost(self, x):
        return self.w_pos_final * _sq3(x["p"] - x["tgt"]) + self.w_vel_final * _sq3(x["v"])

    def cost_grad(self, obs, U, ulps=None):
        """c (n,) and g = dc/dU (n, H, 4), f64.  ulps (n, H, 6), optional."""
        H = self.H
        x = start_state(obs)
        a = clip(U)
        c = np.zeros(len(a), np.float64)
        xs, tapes = [], []
        with np.errstate(all="ignore"):
            for h in range(H):
                x, tape = forward_step(x, a[:, h], None if ulps is None else ulps[:, h])
                xs.append(x)
                tapes.append(tape)
                c = c + self.stage_cost(x, a[:, h])
            c = c + self.final_cost(x)
            d = x["p"] - x["tgt"]
            lp = (2.0 * self.w_pos_final) * d
            lv = (2.0 * self.w_vel_final) * x["v"]
            le, lw = np.zeros_like(d), np.zeros_like(d)
            g = np.zeros((len(a), H, 4), np.float64)
            for h in range(H - 1, -1, -1):
                x = xs[h]
                lp = lp + (2.0 * self.w_pos) * (x["p"] - x["tgt"])
                lv = lv + (2.0 * self.w_vel) * x["v"]
                le = le + (2.0 * self.w_att) * x["e"]
                lw = lw + (2.0 * self.w_rate) * x["w"]
                lp, lv, le, lw, gT, nu = adjoint_step(tapes[h], lp, lv, le, lw, self.fault)
                for j in range(4):
                    da = a[:, h, j].astype(np.float64) - HOVER64
                    g[:, h, j] = ((gT + FACTOR * (S_PHI[j] * nu[0] + self.s_theta[j] * nu[1]))
                                  + KYAW64 * S_PSI[j] * nu[2]) + (2.0 * self.w_effort) * da
        return c, g

    def adam(self, U, g, m, s, p1, p2):
        """One Adam step on U (n, H, 4) f32; returns the new U, m, s."""
        m = self.beta1 * m + (1.0 - self.beta1) * g
        s = self.beta2 * s + (1.0 - self.beta2) * (g * g)
        if self.fault == "no_bias_correction":
            mh, sh = m / 1.0, s / 1.0
        else:
            mh, sh = m / (1.0 - p1), s / (1.0 - p2)
        with np.errstate(all="ignore"):
            up = U.astype(np.float64) - (self.lr * mh) / (np.sqrt(sh) + self.adam_eps)
        return clip(up.astype(np.float32)), m, s

    def plan(self, obs, dones=None, grad=None, ulps=None):
        """One plan step; `grad` (n, H, 4) f64 replaces iteration 1's gradient
        (the device's own grad_out); ulps (I, n, H, 6), optional.  Returns the
        actions (n, 4) f32."""
        if dones is not None:
            self.nominal[np.asarray(dones).astype(bool)] = HOVER
        U = self.nominal.copy()
        m, s = np.zeros(U.shape), np.zeros(U.shape)
        p1, p2 = powers(self.beta1, self.I), powers(self.beta2, self.I)
        for it in range(self.I):
            c, g = self.cost_grad(obs, U, None if ulps is None else ulps[it])
            if it == 0:
                self.last_cost, self.last_grad = c, g
                if grad is not None:
                    g = np.asarray(grad, np.float64)
                ok = np.isfinite(c) & np.isfinite(g).all((1, 2))
            U, m, s = self.adam(U, g, m, s, p1[it], p2[it])
        new = U.copy()
        if self.fault != "no_shift":
            new[:, :-1] = U[:, 1:]
        out = np.where(ok[:, None], U[:, 0], clip(self.nominal[:, 0]))
        self.nominal = np.where(ok[:, None, None], new, self.nominal).astype(np.float32)
        return out.astype(np.float32)


# ------------------------------------------------- the device tests' inputs
NS = (1, 3, 65)
HS = (1, 2, 16, 32)


def nan_index(n):
    """The env of a batch whose observation is NaN: the last lane of the first
    wave where there is one, so that env n - 1 sits alone in the next block."""
    return n - 2 if n >= 3 else None


def batches(n, horizon, nan_row=True):
    """mppi_ref's start rows, cycled, in batches of n that together hold every
    row: for each the obs (n, 15) f32, the nominal (n, H, 4) f32 and the
    index of the NaN row (None: the batch has none).  Repeats of a row are
    moved by a seeded 1 % so that no two envs of a batch agree."""
    k = len(START_ROWS)
    rng = np.random.default_rng(1234 + n)
    for c0 in range(0, k, n):
        rows = [START_ROWS[(c0 + i) % k] for i in range(n)]
        obs = np.stack([r[1] for r in rows]).astype(np.float32)
        nom = np.stack([_nominal(horizon, r[2]) for r in rows])
        if n > k:
            jit = (1 + 0.01 * rng.standard_normal(obs.shape)).astype(np.float32)
            jit[:k] = 1
            obs = (obs * jit).astype(np.float32)
        bad = nan_index(n) if nan_row and c0 == 0 else None
        if bad is not None:
            obs[bad] = np.nan
        yield obs, nom, bad


def random_ulps(seed, shape, k):
    """Seeded whole-ulp moves in {-k, ..., k} for forward_step."""
    return np.random.default_rng(seed).integers(-k, k + 1, shape).astype(np.float64)


def grad_ratio(g, ref):
    """max |g - ref| / max |ref| per env."""
    return np.abs(g - ref).max((1, 2)) / np.abs(ref).max((1, 2))


# (n, H, I) of the device's iterated comparison against the restatement
ITER_CASES = ((3, 16, 3), (3, 16, 10), (65, 16, 10))


def ulp_distance(a, b):
    """Entrywise distance in f32 ulps of two arrays of non-negative floats
    (a clipped nominal has no other)."""
    return np.abs(bits(np.asarray(a, np.float32)).astype(np.int64) -
                  bits(np.asarray(b, np.float32)).astype(np.int64))


def iterate(n, H, I, obs, nom, ulps=None):
    """The new nominal and the action of one plan step of I iterations from
    `nom`, as one (n, H + 1, 4) array: the action first."""
    ref = GplanRef(n, horizon=H, iterations=I)
    ref.nominal = nom.copy()
    out = ref.plan(obs, ulps=ulps)
    return np.concatenate([out[:, None], ref.nominal], 1)


def twin_differences(n, H, I, obs, nom, bad, seed):
    """(entries more than 1 f32 ulp apart, entries that differ, entries) between
    the restatement and its twin with sin / cos moved by seeded +-1 ulp, over
    the rows that are not NaN."""
    ok = np.arange(n) != (-1 if bad is None else bad)
    a = iterate(n, H, I, obs, nom)[ok]
    b = iterate(n, H, I, obs, nom, random_ulps(seed, (I, n, H, 6), 1))[ok]
    d = ulp_distance(a, b)
    return int((d > 1).sum()), int((d > 0).sum()), d.size


# ------------------------------------ shared references of the device tests
_CACHE = {}


def reference(n, H):
    """For every batch of (n, H): obs, nominal, the NaN row's index, the rows
    that are not NaN, and the restatement's cost and gradient of the nominal.
    Computed once; the tests leave it unchanged."""
    if (n, H) not in _CACHE:
        out = []
        for obs, nom, bad in batches(n, H):
            c, g = GplanRef(n, horizon=H).cost_grad(obs, nom)
            out.append((obs, nom, bad, np.arange(n) != (-1 if bad is None else bad), c, g))
        _CACHE[n, H] = out
    return _CACHE[n, H]


def gradient_bar(H, seeds=3, moved=2, allow=8.0):
    """The bar of the device's gradient against the restatement at horizon H,
    as max |dg| / max |g| per env.  Measured, not chosen: the restatement is
    run again with every sin / cos result moved by seeded whole ulps in
    [-moved, moved] (the device's sincos and libm's are each within 1 ulp of
    the correctly rounded value, so up to 2 apart), the worst ratio over every
    batch of every n and `seeds` seeds is taken, and `allow` times that is
    allowed: the device's moves point in some worst direction, the seeded ones
    in a random one.  Returns (bar, the measured worst ratio)."""
    key = ("bar", H, seeds, moved)
    if key not in _CACHE:
        worst = 0.0
        for n in NS:
            for obs, nom, bad, ok, c, g in reference(n, H):
                for seed in range(seeds):
                    g2 = GplanRef(n, horizon=H).cost_grad(
                        obs, nom, random_ulps(1000 * seed + n, (n, H, 6), moved))[1]
                    worst = max(worst, float(grad_ratio(g2[ok], g[ok]).max()))
        _CACHE[key] = worst
    return allow * _CACHE[key], _CACHE[key]
