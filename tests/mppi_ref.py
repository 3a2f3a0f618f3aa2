"""NumPy restatement of the MPPI planner (dr_mppi_*).

The Philox draws go through philox_ref and every f32 operation of the action
law is one numpy call (one IEEE rounding, no FMA), so the device must produce
every sample's action sequence bit for bit.  The model is the oracle's
gym_step_batched: its sin / cos are libm's, the device's are its own (<= 1 ulp
apart), so the restated returns are the law's, not the device's bits; the
device's returns are pinned bit for bit against dr_step (test_planner_gpu).

One plan step for env n (gid = env_id_offset + n), M = f32(3 * 9.81 / 4):
    0. dones[n] set: nominal[n] <- hover, f32(9.81 / 4)
    1. start state, f64: p, v, euler, omega = obs[0:12]; target = obs[0:3] +
       obs[12:15]
    2. sample s at step h: a = clip(U[h]) for s = 0, else
       clip(U[h] + sigma' * pm1(w)), w the block (calls, gid, TAG_PLAN | (s H + h))
       under the key seed; sigma' = f32(sigma sqrt 3); clip(x) = 0 where x < 0,
       M where x > M, else x
    3. H gym steps; while the sample has not crashed before step h
       J += disc[h] * (f64(f32(r)) - (crash ? crash_cost : 0)); disc[0] = 1,
       disc[h] = disc[h - 1] * gamma; a sample that never crashed ends with
       J -= terminal_weight * d, d the gym's distance on the final state
    4. Jmax = max of the J that are not NaN; w = exp((J - Jmax) / lambda), 0 for
       a NaN J; W = sum w.  Jmax not finite: the nominal stays as step 0 left
       it, the action is clip(U[0]), calls counts on
    5. U_new[h] = f32(sum_s w_s * f64(a_s[h]) / W)
    6. action = U_new[0]; nominal[h] <- U_new[h + 1] for h < H - 1;
       nominal[H - 1] <- U_new[H - 1]; calls += 1
"""
import math

import numpy as np

from oracle.drone_np import gym_step_batched
from philox_ref import blocks as _blocks, pm1 as _pm1

TAG_PLAN = 0x4D000000
HOVER = np.float32(9.81 / 4)
MOTOR_MAX = np.float32(3 * 1.0 * 9.81 / 4.0)
FAULTS = (None, "perturb_sample0", "no_shift", "crash_sign", "stale_calls")


def bits(x):
    x = np.ascontiguousarray(x)
    return x.view({4: np.uint32, 8: np.uint64}[x.dtype.itemsize])


def clip(x):
    x = np.asarray(x, np.float32)
    return np.where(x < 0, np.float32(0), np.where(x > MOTOR_MAX, MOTOR_MAX, x)).astype(np.float32)


def discounts(gamma, horizon):
    d, out = 1.0, []
    for _ in range(horizon):
        out.append(d)
        d = d * float(gamma)
    return np.array(out, np.float64)


def start_state(obs, samples):
    """The (n * samples)-row state dict of gym_step_batched the observation
    describes, every env's row repeated `samples` times."""
    o = np.asarray(obs, np.float32).astype(np.float64)
    rep = lambda a: np.repeat(a, samples, axis=0)
    return {"pos": rep(o[:, 0:3]), "vel": rep(o[:, 3:6]), "euler": rep(o[:, 6:9]),
            "omega": rep(o[:, 9:12]), "target": rep(o[:, 0:3] + o[:, 12:15]),
            "step": np.zeros(len(o) * samples, np.int32)}


def distance(pos, target):
    dv = pos - target
    return np.sqrt((dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1]) + dv[:, 2] * dv[:, 2])


class MppiRef:
    """`fault` selects a deliberately WRONG law, for the tests that show the
    checks can fail: "perturb_sample0" adds noise to sample 0 too, "no_shift"
    keeps the new nominal unshifted, "crash_sign" adds the crash cost instead
    of subtracting it, "stale_calls" never advances the call count."""

    def __init__(self, n, samples=256, horizon=16, sigma=0.3, temperature=0.05, gamma=1.0,
                 crash_cost=10.0, terminal_weight=1.0, seed=0, env_id_offset=0, fault=None):
        assert fault in FAULTS
        self.n, self.S, self.H, self.fault = n, samples, horizon, fault
        self.sig = np.float32(float(sigma) * math.sqrt(3.0))
        self.lam, self.cc, self.tw = float(temperature), float(crash_cost), float(terminal_weight)
        self.disc = discounts(gamma, horizon)
        self.seed = seed
        self.gids = env_id_offset + np.arange(n, dtype=np.int64)
        self.reset()

    def reset(self):
        self.nominal = np.full((self.n, self.H, 4), HOVER, np.float32)
        self.calls = np.zeros(self.n, np.uint32)

    def actions(self):
        """Every sample's action sequence on the current nominal and call
        counts: (n, S, H, 4) f32."""
        n, S, H = self.n, self.S, self.H
        idx = np.arange(S * H, dtype=np.int64)
        w = _blocks(self.seed, np.repeat(self.gids, S * H), np.repeat(self.calls, S * H),
                    np.tile(TAG_PLAN | idx, n))
        e = (self.sig * _pm1(w)).astype(np.float32).reshape(n, S, H, 4)
        u = np.broadcast_to(self.nominal[:, None], (n, S, H, 4))
        a = (u + e).astype(np.float32)
        if self.fault != "perturb_sample0":
            a[:, 0] = self.nominal
        return clip(a)

    def returns_from(self, rew, crash, final_d):
        """J (n, S) f64 from per-step f32 rewards (H, n * S), crash flags
        (H, n * S) and the final distance (n * S,), in the law's order."""
        J = np.zeros(rew.shape[1], np.float64)
        alive = np.ones(rew.shape[1], bool)
        for h in range(self.H):
            pay = np.where(crash[h], self.cc, 0.0)
            r = rew[h].astype(np.float32).astype(np.float64)
            term = self.disc[h] * ((r + pay) if self.fault == "crash_sign" else (r - pay))
            J = np.where(alive, J + term, J)
            alive &= ~crash[h].astype(bool)
        J = np.where(alive, J - self.tw * final_d, J)
        return J.reshape(self.n, self.S), alive.reshape(self.n, self.S)

    def returns(self, obs, acts):
        """J (n, S) and the survivors, on the oracle's step."""
        s = start_state(obs, self.S)
        rew, crash = [], []
        with np.errstate(all="ignore"):
            for h in range(self.H):
                _, r, d = gym_step_batched(s, acts[:, :, h].reshape(-1, 4))
                rew.append(r.astype(np.float32))
                crash.append(d)
            return self.returns_from(np.array(rew), np.array(crash),
                                     distance(s["pos"], s["target"]))

    def mean(self, J, acts):
        """U_new (n, H, 4) in f64, unrounded, and the envs that have one."""
        ok = ~np.isnan(J)
        with np.errstate(all="ignore"):
            jmax = np.where(ok, J, -np.inf).max(1)
            valid = np.isfinite(jmax)
            w = np.where(ok, np.exp((J - jmax[:, None]) / self.lam), 0.0)
            W = w.sum(1)
            u = (w[:, :, None, None] * acts.astype(np.float64)).sum(1) / W[:, None, None]
        return u, valid

    def plan(self, obs, dones=None, costs=None):
        """One plan step; `costs` (n, S) f64 replaces the oracle's returns
        (the device's own costs_out).  Returns the actions (n, 4) f32."""
        if dones is not None:
            self.nominal[np.asarray(dones).astype(bool)] = HOVER
        acts = self.actions()
        J = self.returns(obs, acts)[0] if costs is None else np.asarray(costs, np.float64)
        self.last_costs, self.last_actions = J, acts
        u64, valid = self.mean(J, acts)
        u = u64.astype(np.float32)
        out = np.where(valid[:, None], u[:, 0], clip(self.nominal[:, 0]))
        new = u.copy()
        if self.fault != "no_shift":
            new[:, :-1] = u[:, 1:]
        self.nominal = np.where(valid[:, None, None], new, self.nominal).astype(np.float32)
        if self.fault != "stale_calls":
            self.calls = self.calls + np.uint32(1)
        return out.astype(np.float32)


# ------------------------------------------------- the device tests' inputs
def _row(pos, vel=(0, 0, 0), euler=(0, 0, 0), omega=(0, 0, 0), target=(0, 0, 1)):
    s = np.array(list(pos) + list(vel) + list(euler) + list(omega), np.float64)
    return np.concatenate([s, np.array(target, np.float64) - s[:3]]).astype(np.float32)


def _nominal(horizon, pattern=None):
    u = np.full((horizon, 4), HOVER, np.float32)
    if pattern is not None:
        for h in range(horizon):
            u[h] = np.roll(np.array(pattern, np.float32), h)
    return u


# (name, obs row, nominal pattern rolled along the horizon or None for hover)
START_ROWS = (
    ("hover", _row((0.1, -0.2, 1.0), target=(0.3, 0.1, 1.4)), None),
    ("tilted", _row((0, 0, 2), (0.5, 0, -0.5), (0.6, -0.6, 0.3), (1.0, -2.0, 0.5)), None),
    # z = 0.01 descending slowly: the noise decides who crashes late in the horizon
    ("low", _row((0.2, 0.1, 0.01), (0, 0, -0.02), target=(0.2, 0.1, 1.0)), None),
    # a tenth of a millimetre up: the noise decides at the first step
    ("edge", _row((0, 0, 1e-4), (0, 0, -0.005)), None),
    ("far", _row((30, 39.99, 0.5), (0.15, 0.2, 0), target=(0, 0, 1)), None),
    ("bonus", _row((0.5, 0.5, 1.0), target=(0.51, 0.49, 1.02)), None),
    # a nominal that clips at 0 and at MOTOR_MAX, and sits within the noise of both
    ("clips", _row((0, 0, 1.5), target=(0.2, 0, 1.5)), (-0.5, 8.0, 0.1, 7.3)),
)
SHAPES = [(n, s, h, g) for n in (1, 3) for s in (64, 256) for h in (1, 5, 16) for g in (1.0, 0.97)]
CALLS0 = 3          # the call count the device tests start from
SEED = 11


def chunks(n, horizon):
    """The start rows in groups of n (the last group wraps round): for each
    group the names, obs (n, 15) f32 and nominal (n, H, 4) f32."""
    k = len(START_ROWS)
    for c0 in range(0, k, n):
        rows = [START_ROWS[(c0 + i) % k] for i in range(n)]
        yield ([r[0] for r in rows], np.stack([r[1] for r in rows]),
               np.stack([_nominal(horizon, r[2]) for r in rows]))


def make_ref(n, samples, horizon, gamma, nominal, fault=None, **kw):
    ref = MppiRef(n, samples, horizon, gamma=gamma, seed=SEED, fault=fault, **kw)
    ref.nominal = nominal.copy()
    ref.calls = np.full(n, CALLS0, np.uint32)
    return ref
