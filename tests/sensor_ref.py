"""NumPy restatement of the sensor model (dr_sensor_*):
the Philox draws through philox_ref, every f32 operation one numpy call (one
IEEE rounding, no FMA), so that the device must match it bit for bit.

Per env: ep (u32), s, d (i32), bias (od,) f32 and a ring of L = delay_hi + 1
clean rows.  An episode starts at reset() and, in step(), for an env whose
done is set (obs is then the new episode's first observation):
    ep <- 0 at reset, ep + 1 after a done;  s <- 0
    d  <- lo + ((uint64(w0) * (hi - lo + 1)) >> 32),  block TAG_SENSOR | 0
    bias_c <- beta_c * pm1(word c % 4 of block TAG_SENSOR | (1 + c // 4))
    every ring slot <- obs
The delivery at count s: x = ring[(s - d) mod L];
    e_c = bias_c + sigma'_c * pm1(word c % 4 of block
          ((0x60 + c // 4) << 24) | (s & 0xffffff)),   sigma' = f32(sigma sqrt 3)
    out_c = x_c + e_c, or x_c - e_m for a mirror of column m; a column whose
    sigma and beta (its source's, for a mirror) are both 0 is x_c unchanged.
step, not done: s <- s + 1, ring[s mod L] <- obs, deliver.  Done, with the
terminal pair: terminal_out is the old episode's delivery at s + 1 with the
terminal observation as that step's clean row; then the episode start."""
import math

import numpy as np

from philox_ref import blocks as _blocks, pm1 as _pm1

TAG_SENSOR = 0x53000000
NOISE_TOP = 0x60
FAULTS = (None, "leak", "mirror_plus", "stale_ep")


class SensorRef:
    """`fault` selects a deliberately WRONG law, for the tests that show the
    checks can fail: "leak" does not refill the ring at an episode start,
    "mirror_plus" adds the source's error on a mirror column instead of
    subtracting it, "stale_ep" draws the noise after a done from the old
    episode's ep."""

    def __init__(self, n, od, sigma, beta, mirror, delay=(0, 0), seed=0, env_id_offset=0,
                 fault=None):
        assert fault in FAULTS
        self.n, self.od, self.fault = n, od, fault
        self.sigma = np.asarray(sigma, np.float32)
        self.beta = np.asarray(beta, np.float32)
        self.mirror = np.asarray(mirror, np.int64)
        assert self.sigma.shape == self.beta.shape == self.mirror.shape == (od,)
        self.sig = np.array([np.float32(float(s) * math.sqrt(3.0)) for s in self.sigma],
                            np.float32)
        self.lo, self.hi = delay
        self.L = self.hi + 1
        self.seed = seed
        self.gids = env_id_offset + np.arange(n, dtype=np.int64)
        self.ep = np.zeros(n, np.uint32)
        self.s = np.zeros(n, np.int32)
        self.d = np.zeros(n, np.int32)
        self.bias = np.zeros((n, od), np.float32)
        self.ring = np.zeros((self.L, n, od), np.float32)
        src = np.where(self.mirror < 0, np.arange(od), self.mirror)
        self.passes = (self.sigma[src] == 0) & (self.beta[src] == 0)
        # the ep the noise is drawn from ("stale_ep" lets it lag)
        self._noise_ep = self.ep.copy()

    # ------------------------------------------------------------------ law
    def _words(self, ep, top_and_low):
        """(len(ep), od) u32: word c % 4 of block `top_and_low(q)` per quad q."""
        out = np.zeros((len(ep), self.od), np.uint32)
        for q in range((self.od + 3) // 4):
            w = _blocks(self.seed, self._g, ep, top_and_low(q))
            k = min(4, self.od - 4 * q)
            out[:, 4 * q:4 * q + k] = w[:, :k]
        return out

    def _start(self, idx, obs, first):
        """Episode start of envs `idx` on their rows of obs."""
        if len(idx) == 0:
            return
        self.ep[idx] = 0 if first else self.ep[idx] + np.uint32(1)
        if self.fault != "stale_ep" or first:
            self._noise_ep[idx] = self.ep[idx]
        self.s[idx] = 0
        self._g = self.gids[idx]
        w0 = _blocks(self.seed, self._g, self.ep[idx], TAG_SENSOR)[:, 0].astype(np.uint64)
        self.d[idx] = self.lo + ((w0 * np.uint64(self.hi - self.lo + 1)) >>
                                 np.uint64(32)).astype(np.int32)
        w = self._words(self.ep[idx], lambda q: TAG_SENSOR | (1 + q))
        self.bias[idx] = self.beta[None, :] * _pm1(w)
        if self.fault != "leak" or first:
            self.ring[:, idx] = obs[idx][None]
        else:
            self.ring[0, idx] = obs[idx]

    def _deliver(self, idx, s, x, ep):
        """The delivery of envs `idx` at counts `s` with clean rows x."""
        self._g = self.gids[idx]
        s = np.asarray(s, np.int64)
        w = self._words(ep, lambda q: ((NOISE_TOP + q) << 24) | (s & 0xffffff))
        e = self.bias[idx] + self.sig[None, :] * _pm1(w)
        em = e[:, np.maximum(self.mirror, 0)]
        mir = x + em if self.fault == "mirror_plus" else x - em
        out = np.where(self.mirror[None, :] < 0, x + e, mir).astype(np.float32)
        return np.where(self.passes[None, :], x, out)

    # ------------------------------------------------------------ interface
    def reset(self, obs):
        obs = np.ascontiguousarray(obs, np.float32)
        every = np.arange(self.n)
        self._start(every, obs, first=True)
        return self._deliver(every, self.s, obs, self._noise_ep)

    def step(self, obs, done, term_obs=None, term_out=None):
        """Returns out or, with term_obs, (out, term_out): term_out (a copy of
        the given one, or zeros) with the rows of done envs replaced."""
        obs = np.ascontiguousarray(obs, np.float32)
        done = np.asarray(done).astype(bool)
        live, dead = np.flatnonzero(~done), np.flatnonzero(done)
        to = None
        if term_obs is not None:
            to = np.zeros_like(obs) if term_out is None else np.array(term_out, np.float32)
            if len(dead):
                s1 = self.s[dead].astype(np.int64) + 1
                slot = np.mod(s1 - self.d[dead], self.L)
                x = np.where((self.d[dead] == 0)[:, None], np.asarray(term_obs, np.float32)[dead],
                             self.ring[slot, dead])
                to[dead] = self._deliver(dead, s1, x, self._noise_ep[dead])
        self.s[live] += 1
        self.ring[np.mod(self.s[live], self.L), live] = obs[live]
        self._start(dead, obs, first=False)
        every = np.arange(self.n)
        x = self.ring[np.mod(self.s.astype(np.int64) - self.d, self.L), every]
        out = self._deliver(every, self.s, x, self._noise_ep)
        return out if term_obs is None else (out, to)

    def state(self):
        """(3, n) int32 as the device keeps it: ep's bits, s, d."""
        return np.stack([self.ep.view(np.int32), self.s, self.d])


# ------------------------------------------------------------------ inputs
# The cases of the device comparison (tests/test_sensor_gpu.py), which the CPU
# tests also run the fault modes on: (n, od, delay, mirrors, terminal pair,
# done pattern).  Every n (wave and block tails), od (quad tails), delay pair,
# mirror / terminal choice and done pattern occurs; not their full product.
STEPS = 40
DONE_PATTERNS = ("none", "all", "first", "consecutive", "random")
CASES = (
    (1, 12, (0, 0), False, False, "none"),
    (63, 15, (3, 3), True, True, "random"),
    (257, 16, (0, 4), True, True, "consecutive"),
    (4099, 19, (15, 15), False, True, "first"),
    (4099, 15, (0, 4), True, True, "random"),
    (257, 19, (3, 3), True, False, "all"),
    (63, 16, (15, 15), True, True, "all"),
    (1, 15, (0, 4), True, True, "consecutive"),
    (257, 12, (0, 4), False, True, "random"),
    (63, 19, (0, 0), True, True, "first"),
)


def done_pattern(kind, steps, n, rng):
    """(steps, n) u8.  "first": every env on the first step; "consecutive":
    even envs (env 0 among them) on steps 5, 6 and 7; "random": p = 0.1."""
    d = np.zeros((steps, n), np.uint8)
    if kind == "all":
        d[:] = 1
    elif kind == "first":
        d[0] = 1
    elif kind == "consecutive":
        d[5:8, 0::2] = 1
    elif kind == "random":
        d[:] = rng.random((steps, n)) < 0.1
    else:
        assert kind == "none"
    return d


def case_inputs(case, seed=0):
    """The settings and the synthetic stream of a case: per-column sigma and
    beta in (0, 0.1) with column 4 left clean (sigma = beta = 0), the last
    three columns mirrors of the first three when asked, random normal
    observations and terminal observations."""
    n, od, delay, mirrors, terminal, pattern = case
    rng = np.random.default_rng([seed, n, od])
    sigma = rng.uniform(0.01, 0.1, od).astype(np.float32)
    beta = rng.uniform(0.01, 0.1, od).astype(np.float32)
    sigma[4] = beta[4] = 0.0
    mirror = np.full(od, -1, np.int64)
    if mirrors:
        mirror[od - 3:] = (0, 1, 2)
    return {"n": n, "od": od, "delay": delay, "sigma": sigma, "beta": beta, "mirror": mirror,
            "obs0": rng.standard_normal((n, od)).astype(np.float32),
            "obs": rng.standard_normal((STEPS, n, od)).astype(np.float32),
            "term": rng.standard_normal((STEPS, n, od)).astype(np.float32) if terminal else None,
            "dones": done_pattern(pattern, STEPS, n, rng)}


def make_ref(inp, seed=7, env_id_offset=0, fault=None):
    return SensorRef(inp["n"], inp["od"], inp["sigma"], inp["beta"], inp["mirror"], inp["delay"],
                     seed=seed, env_id_offset=env_id_offset, fault=fault)


def bits(a):
    """The bit patterns of an f32 array (NaN payloads and the sign of zero
    count in a bitwise comparison)."""
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
