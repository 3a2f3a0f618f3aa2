"""The env kernels on the designed state corpus of tests/env_states.py: the
out-of-range trig branch, the fast range's boundary, gimbal lock, the
termination and bonus thresholds at their edges, and non-finite state.

a. test_step_matches_oracle: one dr_step of every variant and dtype, and of
   the gym variant under each of its options (wind, waypoint courses,
   airframe randomisation), against the CPU oracle.
b. test_device_sincos_ulps: the device's sin / cos against mpmath, read
   through state words one or two roundings away.
c. test_step_forms_bitwise / test_rollout_*: every kernel form against the
   default step kernel, bit patterns compared (NaN rows count).

The float bound of (a).  Per entry |got - ref| <= gamma(c) x envelope, gamma(c)
= c u / (1 - c u), u = 2^-53 (f64 state) or 2^-24 (f32); the envelope is the
value's expression with every term replaced by its absolute value
(env_states.envelopes), so every rounding, being relative to a partial
result, is at most u x envelope.  c counts those roundings
(env_states.rounding_counts), per side of the comparison:

  S    one sin / cos.  Fast path: trig.h holds it to 1 ulp (f32: 2) from the
       correctly rounded value, i.e. 1.5 (2.5) ulp = 3u (5u) from the true
       one.  Library path (a row with |angle| >= 2^19): the OpenCL C bound of
       4 ulp = 8u that the device library is built to; unverified here.
       CPU oracle: glibc, 1 ulp = 2u.
  K    1 in f32 state, where the constants dt, g, the inertias and 0.01 are
       themselves rounded; 0 in f64.
  vel  three trig factors and two products, the sum (r02), x T, / m (exact),
       x dt (+K), + g term (K), + vel:                  3S + 6 + 2K
  pos  vel, x dt (+K), + pos:                           vel + 2 + K
  eul  tan as the corrected quotient of sth and cth (2S + 2; oracle: one
       library tan, 2), one more trig factor, two products, two sums, x dt
       (+K), + angle:                                   S + tan + 6 + K
       (the yaw row's two div_rcp quotients, 2S + 2 each, cost no more)
  omg  factor x mix (1 + K), inertia difference (K) x w x w (2), the
       difference (1), div_rcp (2, its divisor K), x dt (1 + K), + omega:
                                                        8 + 4K
  rew  pos, - target (1), squares and sums under the root (halved: 1.5 + 1),
       the root (1), x 0.01 (1 + K), + bonus (1):       pos + 7 + K
       then the f32 casts, 2^-24 |r| each, added outside gamma.

The gym options (kinds "wind", "waypoint", "airframe" of env_states.OPTIONS)
change these lines, on both sides of the comparison alike (the restatements
tests/wind_ref.py, waypoint_ref.py, airframe_ref.py are f64 and have the
kernel's operations):

  wind      the pre-step v' = v + ((k (w - v)) dt) stands where v does.  w =
            (S)(m + g') is the exact cast of an f32 sum and (S)k an exact
            cast; the difference (1), x k (1), x dt (1 + K), the sum (1):
                                                        vel + 4 + K
            pos and rew follow from vel.  Envelope: |v| + k (|w| + |v|) dt
            in place of |v|.  The gust g' = b g + c xi is f32 in both state
            dtypes and compared bitwise with wind_ref.gust_update.
  airframe  x (S)im replaces the exact / kMass:         vel + 1
            x (S)is on each of the three torques:       omg + 1
            im = 1.0f / m and is = 1.0f / s are f32 divides on both sides
            (equal inputs, no rounding counted); the gained command g_j a_j
            is f32 on both sides too.  Envelope: 1/m on the thrust terms (not
            on g), 1/s on the torques, up to 10 at the spreads' ends.
  waypoint  the physics and its counts are the gym's; reached = d < (S)R, the
            counters and the new target are exact (option_exact_failures).

c = kernel side + oracle side in f64 (15 + 12 = 27 for vel on the fast path,
30 + 12 = 42 on the library path); in f32 the f64 oracle's whole error is
below one f32 rounding: kernel side + 1.  None of this is taken from what the
kernel produces.  Measured worst |got - ref| / (u x envelope) on the MI355X
(c: f64 pos 31..46, vel 27..42, euler 27..42, omega 16; f32 pos 27..36, vel
24..33, euler 25..34, omega 13); rew as a fraction of its bound; flips = f32
`done` differing from the f64 oracle, all in block E, none in A-D:

  variant     dtype  pos   vel   euler  omega  rew    flips
  gym         f64    1.94  4.03  3.98   0.00   0.332  0
  gym         f32    2.73  4.33  4.14   3.28   0.027  142
  moving      f64    1.78  4.12  4.24   0.00   0.329  0
  moving      f32    1.84  3.63  3.95   3.34   0.027  128
  smooth      f64    1.97  3.70  5.17   0.00   0.000  0
  smooth      f32    2.68  3.25  4.10   3.14   0.068  156
  tag         f64    2.69  3.80  4.67   0.00   0.000  0
  tag         f32    2.98  4.22  3.47   3.36   0.030  136
  vectorized  f64    1.93  3.95  4.06   0.00   0.328  0
  vectorized  f32    2.13  3.68  3.76   3.31   0.022  128

(omega 0.00 in f64: div_rcp gave the IEEE quotient's bits on every row.)

The gym options, measured the same way (c: wind f64 pos 39..54, vel 35..50,
f32 pos 32..41, vel 29..38; airframe f64 pos 33..48, vel 29..44, omega 18, f32
pos 28..37, vel 25..34, omega 14; waypoint and every other count as gym's);
reach flips = f32 `reached` differing from the f64 restatement's, all in block
E:

  kind        dtype  pos   vel   euler  omega  rew    flips  reach flips
  wind        f64    2.11  3.57  5.08   0.00   0.333  0
  wind        f32    2.27  3.47  4.05   3.48   0.025  158
  waypoint    f64    1.81  3.83  5.34   0.00   0.331  0      0
  waypoint    f32    1.99  3.34  4.31   3.20   0.023  134    36
  airframe    f64    2.40  4.15  3.78   0.00   0.330  0
  airframe    f32    2.82  3.89  3.52   3.83   0.026  118

(waypoint: 506 reaches in f64, 465 of them in block E and 251 in a step that
also ends the episode; 369 rows of E miss by less than 1e-6.  wind f32: the
rows at the largest finite f32 wind reach |pos| = 6.8e34, where the f32
squares of the reward's distance overflow: the kernel's reward is -inf there,
as the f32 recomputation from its stored position has it, and the f64
restatement's is finite; those rows are compared with the recomputation only.)

`done` is exact: equal to the oracle on every row in f64, on blocks A-D in
f32 (tests/test_env_states_cpu.py shows those rows >= 1e-3 from every
threshold), and in both dtypes equal to the reference's own predicate
recomputed from the position the kernel stored."""
import os
import subprocess

import numpy as np
import pytest
import torch

import env_states as es
from env_states_worker import (K, actions_for, assert_same_run, check_rollout,
                               check_rollout_random, fields, new_batch, same_bits, step_run)
from subproc import run_worker

pytestmark = pytest.mark.gpu
VARIANTS = ("gym", "moving", "smooth", "tag", "vectorized")
KINDS = tuple(es.OPTIONS)               # the gym options: wind, waypoint, airframe
DTYPES = ("f64", "f32")
U32 = 2.0 ** -24


def _np(t):
    return t.detach().cpu().numpy()


def _moved_target(c, step_new):
    """The moving variant's target at the new step (oracle formula, numpy
    f32): within a few f32 ulps of the amplitude of the device's."""
    mp = c["motion"]
    t = step_new.astype(np.float32) * np.float32(es.DT)
    ang = mp[:, 3:6] * t[:, None] + mp[:, 6:9]
    return c["target"] + (mp[:, 0:3] * np.sin(ang)).astype(np.float64)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS + KINDS)
def test_step_matches_oracle(variant, dtype):
    c = es.corpus(dtype, variant)
    n, f, u = c["n"], es.ftype(dtype), es.unit_roundoff(dtype)
    b = new_batch(variant, dtype, c, False)
    obs, rew, done = b.step(torch.from_numpy(c["action"]).cuda())
    obs, rew, done = _np(obs), _np(rew), _np(done).astype(bool)
    got = {k: _np(b.get(k)) for k in ("pos", "vel", "euler", "omega")}
    step = _np(b.get("current_step"))
    tgt_new = _np(b.get("target")) if variant == "waypoint" else None
    ref, ro, rr, rd = es.oracle_step(variant, c)
    ad = es.rows_of(c, es.AD)

    # ---- done -----------------------------------------------------------
    flips = done != rd
    print(f"{variant} {dtype}: n {n}, done flips vs oracle {int(flips.sum())} "
          f"(blocks A-D: {int(flips[ad].sum())})")
    assert not flips[ad].any()
    if dtype == "f64":
        assert not flips.any(), np.flatnonzero(flips)[:10]
    assert np.array_equal(step, ref["step"])
    # ---- exact self-consistency ----------------------------------------------
    want_done, crash = es.done_predicate(variant, dtype, got["pos"], step, c["max_steps"])
    assert np.array_equal(done, want_done), np.flatnonzero(done != want_done)[:10]
    e = c["blocks"]["E"]
    assert want_done[e].sum() > 1000 and (~want_done[e]).sum() > 1000
    tgt = c["target"]
    exact_rows = np.ones(n, bool)
    if variant == "moving":
        exact_rows = (c["motion"][:, :3] == 0).all(1)      # target == centre exactly
    dev_sq = es.smooth_dev_sq(c) if variant == "smooth" else None
    want_rew = es.reward_exact(variant, dtype, got["pos"], tgt, crash, dev_sq)
    ok = es.same_bits_or_nan(rew, want_rew) | ((rew == 0) & (want_rew == 0))
    assert ok[exact_rows].all(), np.flatnonzero(~ok & exact_rows)[:10]
    bonus = np.abs(want_rew) > 0.4 if variant != "smooth" else want_rew > 0.4
    if variant != "smooth":
        assert (bonus & exact_rows)[e].sum() >= 20 and (~bonus & exact_rows)[e].sum() >= 20

    # ---- obs against the stored state, exact --------------------------------
    with np.errstate(all="ignore"):
        st12 = np.concatenate([got[k] for k in ("pos", "vel", "euler", "omega")], 1)
        assert es.same_bits_or_nan(obs[:, :12], st12.astype(np.float32)).all()
        ps = got["pos"].astype(f)
        if variant == "tag":
            sw = np.arange(n) ^ 1
            vs = got["vel"].astype(f)
            ext = np.concatenate([(ps[sw] - ps).astype(np.float32),
                                  (vs[sw] - vs).astype(np.float32)], 1)
            assert es.same_bits_or_nan(obs[:, 12:18], ext).all()
            assert np.array_equal(obs[:, 18], np.where(np.arange(n) % 2 == 0, 1, -1))
        elif variant != "vectorized":
            # waypoint: the stored target is the new one on the reach rows
            rel = ((tgt if tgt_new is None else tgt_new).astype(f) - ps).astype(np.float32)
            assert es.same_bits_or_nan(obs[exact_rows, 12:15], rel[exact_rows]).all()
        if variant == "smooth":
            al = np.float32(es.SMOOTH[0])
            lag = (np.float32(1.0) - al) * c["motor"] + al * c["action"]
            assert es.same_bits_or_nan(_np(b.get("motor")), lag).all()
            assert es.same_bits_or_nan(obs[:, 15:19], lag).all()
        if variant == "moving":
            aw = np.abs(c["motion"][:, 0:3] * c["motion"][:, 3:6]).astype(np.float64)
            fin = np.isfinite(ro[:, 15:18])
            assert (np.abs(obs[:, 15:18].astype(np.float64) - ro[:, 15:18])[fin]
                    <= (8 * U32 * aw)[fin]).all()

    # ---- non-finite entries ---------------------------------------------------
    for k in got:
        assert es.same_nonfinite(got[k], ref[k]), k
    # f32 squares overflow where |pos - target| passes 1.8e19 (the wind kind's
    # rows at the largest finite f32): there the kernel's distance is inf and
    # its reward -inf, as reward_exact has it above, and the f64 oracle's finite
    sq_over = np.zeros(n, bool)
    if dtype == "f32" and variant != "tag":
        with np.errstate(all="ignore"):
            d2 = ((ref["pos"] - tgt) ** 2).sum(1)
            sq_over = np.isfinite(d2) & (d2 > float(np.finfo(np.float32).max))
        assert sq_over.sum() == 0 if variant != "wind" else 6 <= sq_over.sum() <= 15
        assert (rew[sq_over] == -np.inf).all() and np.isfinite(rr[sq_over]).all()
    assert es.same_nonfinite(rew[~sq_over], rr[~sq_over])
    with np.errstate(over="ignore"):
        assert np.isinf(st12.astype(np.float32)).sum() == np.isinf(obs[:, :12]).sum()
    if dtype == "f64":
        assert np.isinf(obs[:, 6:9]).any()          # angles that overflow the f32 cast

    # ---- floats ---------------------------------------------------------------
    oor = (~(np.abs(c["euler"]) < es.FAST)).any(1)
    cnt = es.bound_counts(dtype, oor, variant=variant)
    tnew = None
    amp = np.zeros(n)
    if variant == "moving":
        tnew = np.abs(c["target"]) + np.abs(c["motion"][:, :3])
        amp = np.abs(c["motion"][:, :3]).max(1).astype(np.float64)
    env = es.envelopes(variant, c, tnew)
    line = []
    for k in ("pos", "vel", "euler", "omega"):
        units, rel = es.worst_ratio(got[k], ref[k], env[k], cnt[k], u)
        line.append(f"{k} {units:.2f} (c {cnt[k].min():.0f}..{cnt[k].max():.0f})")
        assert rel <= 1.0, (k, units, rel)
    # reward: the bonus is a step of height 1; where the oracle's distance is
    # within the bound of the edge the two may legitimately differ, and the
    # exact recomputation above has already pinned the kernel's choice
    with np.errstate(all="ignore"):
        if variant == "tag":
            dv = ref["pos"] - ref["pos"][c["pairs"]]
            edge = float(np.float32(es.TAG[0]))
        else:
            dv = ref["pos"] - (_moved_target(c, ref["step"]) if variant == "moving" else tgt)
            edge = es.bonus_edge(variant)
        d_ref = np.sqrt((dv ** 2).sum(1))
        d_tol = es.gamma(cnt["rew"], u) * env["rew"] / 0.01 + 8 * U32 * amp * np.sqrt(3.0)
        clear = ~(np.abs(d_ref - edge) <= d_tol)
        extra = 0.01 * 8 * U32 * amp * np.sqrt(3.0)      # device sinf against the oracle's
        if variant == "smooth":
            extra = extra + 3 * U32 * np.float64(es.SMOOTH[1]) * dev_sq
        if variant == "tag":
            extra = extra + 3 * U32 * es.TAG[1]
        fin = np.isfinite(rr) & clear & ~sq_over
        if variant == "tag":
            # the crash penalty is a step too: f32 may cross a threshold the
            # f64 oracle does not (block E only; never in f64)
            same_crash = crash == ref["crash"]
            assert same_crash[ad].all() and (dtype == "f32" or same_crash.all())
            fin &= same_crash
        err = np.abs(rew.astype(np.float64) - rr)
        lim = es.gamma(cnt["rew"], u) * (env["rew"] + 1.0) + 3 * U32 * np.abs(rr) + extra
        assert (err[fin] <= lim[fin]).all(), np.flatnonzero(fin & (err > lim))[:10]
        assert clear.mean() > 0.9
        line.append(f"rew {np.max(np.where(fin, err / lim, 0.0)):.3f} of its bound")
    print(f"{variant} {dtype}: worst |got - ref| / (u x envelope): " + ", ".join(line))

    # ---- the options' own words, exact -------------------------------------------
    if variant in KINDS:
        gx = {"pos": got["pos"], "target": _np(b.get("target")), variant: _np(b.get(variant))}
        assert es.option_exact_failures(variant, dtype, c, gx) == []
    if variant == "waypoint":
        reached = es.reached_exact(dtype, got["pos"], tgt)
        near = ~reached & (np.abs(ref["d"] - edge) < 1e-6)
        ended = reached & done
        print(f"waypoint {dtype}: reaches {int(reached.sum())} (block E {int(reached[e].sum())}, "
              f"in a step that ends {int(ended.sum())}), near misses in E {int(near[e].sum())}, "
              f"reach flips vs oracle {int((reached != ref['reached']).sum())}")
        assert reached[e].sum() >= 20 and near[e].sum() >= 20 and ended.sum() >= 40
        assert not (reached != ref["reached"])[ad].any()
        if dtype == "f64":
            assert np.array_equal(reached, ref["reached"])
    if variant == "airframe":
        # the rows at 1.0f in all six words are the gym kernel's rows
        ones = (c["airframe"] == 1).all(1)
        assert ones.sum() >= 500
        g = new_batch("gym", dtype, {k: v for k, v in c.items() if k != "airframe"}, False)
        go, gr, gd = g.step(torch.from_numpy(c["action"]).cuda())
        for name, x, y in [("obs", obs, _np(go)), ("rew", rew, _np(gr)),
                           ("done", done, _np(gd).astype(bool))] + \
                [(k, got[k], _np(g.get(k))) for k in got]:
            same = es.same_bits_or_nan(x, y) if x.dtype.kind == "f" else x == y
            assert same[ones].all(), name
            if name in ("vel", "omega"):
                assert not same[~ones].all(), name      # the option is live elsewhere
        g.close()
    b.close()


# ---------------------------------------------------------------------------
# b. device sin / cos in ulps
# ---------------------------------------------------------------------------
_SWEEP = {}


def _sweep(dtype):
    """Blocks A, C, D and 2^14 log-spaced magnitudes, both signs, with the
    mpmath sin / cos of each (cached per dtype)."""
    if dtype not in _SWEEP:
        f = es.ftype(dtype)
        fi = np.finfo(f)
        top = 1e300 if dtype == "f64" else 3e38
        lg = np.exp(np.linspace(np.log(float(fi.tiny)), np.log(top), 1 << 14))
        hi = np.exp(np.linspace(np.log(es.FAST), np.log(top), 256))
        _, xw = es.worst_cancellation(dtype, 128)
        base = es.rn(np.arange(-16, 17) * float(es.rn(np.pi / 2, dtype)), dtype)
        a = np.concatenate([es.ulp_steps(base, k, dtype) for k in range(-3, 4)])
        x = np.concatenate([lg, hi, xw, es.ulp_steps(xw, 1, dtype), es.ulp_steps(xw, -1, dtype),
                            a, [0.0, float(fi.smallest_subnormal), float(fi.tiny)]])
        x = es.rn(np.concatenate([x, -x, es.boundary_values(dtype)]), dtype)
        x = x[np.isfinite(x)]
        n = len(x) + (len(x) & 1)                      # even, ragged
        x = np.concatenate([x, np.full(n - len(x), 0.75)])
        _SWEEP[dtype] = (x, es.mp_sincos(x))
    return _SWEEP[dtype]


ROUTES = ("cos_phi", "sin_phi", "sin_theta", "cos_theta", "cos_psi", "sin_psi")
THETA0 = 0.5


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("route", ROUTES)
def test_device_sincos_ulps(route, dtype):
    """One angle x at a time ("gym" step, the other angles +0 unless said,
    vel = 0, pos = (0, 0, 2), target far); dt is the state dtype's RN(0.02).
    Each route, from physics_step_mixed (sincos(+0) = (+0, 1) exactly):

      cos_phi    omega = (0, 1, 0): ed1 = (0 w0 + cph 1) + (-sph) 0 = cph, so
                 euler[1] = 0 + RN(cph dt).
      sin_phi    omega = (0, 0, 1): ed1 = (0 + cph 0) + (-sph) 1 = -sph, so
                 euler[1] = RN(-sph dt).
      sin_theta  four actions of 0.25: thrust exactly 1, all torques 0; r02 =
                 (1 sth) 1 + 0 0 = sth, acc0 = 0 + (sth 1) / 1, so vel[0] =
                 RN(sth dt).
      cos_theta  omega = (0, 0, 1), phi = 0: ed2 = (0 + div_rcp(0, cth) 0) +
                 div_rcp(1, cth) 1 = q, q the corrected quotient 1 / cth
                 (<= 1 ulp), so euler[2] = RN(q dt).
      cos_psi    theta = RN(0.5), thrust 1: r02 = RN(cps sth0) 1 + sps 0, so
      sin_psi    vel[0] = RN(RN(cps sth0) dt); r12 = RN(sps sth0) 1 - cps 0,
                 so vel[1] = RN(RN(sps sth0) dt).  sth0 is the device's own
                 sin(0.5), another fast-path result.

    Bound, absolute, each ulp taken at the value it applies to: B ulp(f) x
    |d result / d f| for the function, B = 1.5 ulp (f32: 2.5) on the fast
    path -- trig.h's 1 (2) ulp from the correctly rounded value is 1.5 (2.5)
    from the true one -- and 4 ulp for |x| >= 2^19, the OpenCL C figure the
    device library is built to (unverified); plus 0.5 ulp of each further
    rounded intermediate (1 ulp for the corrected quotient) carried to the
    result.  The reference is mpmath on the exact input at 240 bits.
    Measured on the MI355X, worst error / bound, and in brackets the
    function's error in its own ulps (an upper estimate: it includes the
    route's roundings), fast path | library path:

      route      f64                          f32
      cos_phi    0.647 (1.44) | 0.267 (1.28)  0.514 (1.69) | 0.413 (1.98)
      sin_phi    0.614 (1.38) | 0.268 (1.28)  0.901 (1.75) | 0.380 (1.81)
      sin_theta  0.614 (1.38) | 0.268 (1.28)  0.901 (1.75) | 0.380 (1.81)
      cos_theta  0.560 (2.24) | 0.313 (2.12)  0.538 (2.84) | 0.349 (2.31)
      cos_psi    0.477 (2.10) | 0.277 (1.86)  0.435 (2.77) | 0.300 (2.26)
      sin_psi    0.500 (1.72) | 0.267 (1.81)  0.885 (2.23) | 0.314 (2.41)

    (0.901 / 0.885: x near 1.4e-38, where the result RN(sin x dt) is
    subnormal and its own last rounding is nearly the whole bound.)"""
    x, (sh, sl, ch, cl) = _sweep(dtype)
    n, f = len(x), es.ftype(dtype)
    dt = float(f(es.DT))
    c = {"n": n, "pos": np.tile([0.0, 0.0, 2.0], (n, 1)), "vel": np.zeros((n, 3)),
         "euler": np.zeros((n, 3)), "omega": np.zeros((n, 3)),
         "target": np.tile([5.0, 5.0, 5.0], (n, 1)), "step": np.zeros(n, np.int32),
         "action": np.zeros((n, 4), np.float32)}

    def ulp(v):
        return np.spacing(np.abs(np.asarray(v, np.float64)).astype(f)).astype(np.float64)
    lib = ~(np.abs(x) < es.FAST)
    B = np.where(lib, 4.0, 1.5 if dtype == "f64" else 2.5)
    sin_t, cos_t = sh + sl, ch + cl
    if route in ("cos_phi", "sin_phi"):
        c["euler"][:, 0] = x
        c["omega"][:, 1 if route == "cos_phi" else 2] = 1.0
        fv, (fh, fl) = (cos_t, (ch, cl)) if route == "cos_phi" else (-sin_t, (-sh, -sl))
        field, col = "euler", 1
        scale = dt
        lim = B * ulp(fv) * dt
    elif route == "sin_theta":
        c["euler"][:, 1] = x
        c["action"][:] = 0.25
        fv, (fh, fl) = sin_t, (sh, sl)
        field, col, scale = "vel", 0, dt
        lim = B * ulp(fv) * dt
    elif route == "cos_theta":
        c["euler"][:, 1] = x
        c["omega"][:, 2] = 1.0
        fv, (fh, fl) = cos_t, (ch, cl)
        field, col = "euler", 2
        with np.errstate(all="ignore"):
            scale = dt / (cos_t * cos_t)
            lim = B * ulp(fv) * scale + 1.0 * ulp(1.0 / cos_t) * dt
    else:
        c["euler"][:, 2] = x
        c["euler"][:, 1] = float(es.rn(THETA0, dtype))
        c["action"][:] = 0.25
        fv, (fh, fl) = (cos_t, (ch, cl)) if route == "cos_psi" else (sin_t, (sh, sl))
        field, col = "vel", 0 if route == "cos_psi" else 1
        s0h, s0l, _, _ = es.mp_sincos(np.array([float(es.rn(THETA0, dtype))]))
        s0 = float(s0h[0] + s0l[0])
        B0 = 1.5 if dtype == "f64" else 2.5
        scale = abs(s0) * dt
        lim = (B * ulp(fv) * abs(s0) + B0 * ulp(s0) * np.abs(fv) + 0.5 * ulp(fv * s0)) * dt
    # the true result in extended precision (np.longdouble carries 64 bits,
    # enough beside bounds of >= 1 ulp of 53)
    ld = np.longdouble
    if route == "cos_theta":
        with np.errstate(all="ignore"):
            true = ld(dt) / (ld(ch) + ld(cl))
    elif route in ("cos_psi", "sin_psi"):
        true = (ld(fh) + ld(fl)) * (ld(s0h[0]) + ld(s0l[0])) * ld(dt)
    else:
        true = (ld(fh) + ld(fl)) * ld(dt)
    b = new_batch("gym", dtype, c, False)
    b.step(torch.from_numpy(c["action"]).cuda())
    got = _np(b.get(field))[:, col]
    b.close()
    with np.errstate(all="ignore"):
        lim = lim + 0.5 * ulp(np.asarray(true, np.float64))     # the last rounding
        err = np.abs(np.asarray(ld(got) - true, np.float64))
        fin = np.isfinite(np.asarray(true, np.float64)) & np.isfinite(lim) & (lim > 0)
        ratio = np.where(fin, err / lim, 0.0)
        # the function's own error, where the result is a normal number
        den = ulp(fv) * np.abs(scale)
        normal = np.abs(np.asarray(true, np.float64)) >= float(np.finfo(f).tiny)
        f_ulps = np.where(fin & normal & (den > 0), err / den, 0.0)
    assert fin.sum() > 0.95 * n and np.isfinite(got[fin]).all()
    for name, m in (("fast", ~lib), ("library", lib)):
        i = np.argmax(np.where(m, ratio, -1.0))
        print(f"{route} {dtype} {name}: {int((m & fin).sum())} angles, worst error / bound "
              f"{ratio[i]:.3f} at x = {x[i]!r}; function error <= "
              f"{np.max(np.where(m, f_ulps, 0.0)):.2f} ulp")
    assert ratio.max() <= 1.0, (ratio.max(), x[ratio.argmax()])
    # exact zeros stay exact
    z = (np.asarray(true, np.float64) == 0) & np.isfinite(x)
    assert (got[z] == 0).all()


@pytest.fixture(scope="module")
def host_trig(tmp_path_factory):
    """tests/c/trig_host.cpp: trig.h's fast path as g++ compiles it."""
    import ctypes
    so = str(tmp_path_factory.mktemp("trig") / "libtrig.so")
    src = os.path.join(os.path.dirname(os.path.abspath(__file__)), "c", "trig_host.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared",
                    src, "-o", so], check=True)
    lib = ctypes.CDLL(so)

    def f(x, dtype):
        x = np.ascontiguousarray(x, es.ftype(dtype))
        s, c = np.empty_like(x), np.empty_like(x)
        p = lambda a: a.ctypes.data_as(ctypes.c_void_p)  # noqa: E731
        fn = lib.trig_sincos if dtype == "f64" else lib.trig_sincosf
        fn(ctypes.c_int64(len(x)), p(x), p(s), p(c))
        return s, c
    return f


@pytest.mark.parametrize("dtype", DTYPES)
def test_fast_path_is_the_host_build_and_the_library_branch_is_live(dtype, host_trig):
    """Inside the fast range the device's sincos is trig.h's, and trig.h is
    IEEE operations only (fma, rint, the int conversion, products and sums
    with contraction off), so the device must give the bits of the g++ build
    that tests/test_trig_host.py holds to mpmath: checked on every in-range
    angle of the sweep through the cos_phi and sin_phi routes, whose last
    step, RN(f dt), numpy restates exactly.  From |x| = 2^19 on the library
    takes over: over the 130 floats of block C at and above +-2^19 the device
    must NOT reproduce the fast path's bits throughout (two different
    algorithms that are each only mostly correctly rounded agree on 260
    results with negligible probability), or the out-of-range branch is not
    being taken at the boundary trig.h states.  Measured: every in-range
    angle equal in both dtypes; at the boundary 214 of 260 (f64) and 240 of
    264 (f32) library results equal to the fast path's."""
    x, _ = _sweep(dtype)
    n, f = len(x), es.ftype(dtype)
    near = np.abs(x) < 2.0 ** 21                    # the host build's int conversion is defined
    s, c = host_trig(np.where(near, x, 0.0), dtype)
    want = {"cos_phi": c * f(es.DT), "sin_phi": (-s) * f(es.DT)}
    inside = np.abs(x) < es.FAST
    edge = ~inside & np.isin(x, es.boundary_values(dtype))
    assert edge.sum() >= 130 and inside.sum() > 15000
    same_edge = 0
    for route, w in want.items():
        cc = {"n": n, "pos": np.tile([0.0, 0.0, 2.0], (n, 1)), "vel": np.zeros((n, 3)),
              "euler": np.zeros((n, 3)), "omega": np.zeros((n, 3)),
              "target": np.tile([5.0, 5.0, 5.0], (n, 1)), "step": np.zeros(n, np.int32),
              "action": np.zeros((n, 4), np.float32)}
        cc["euler"][:, 0] = x
        cc["omega"][:, 1 if route == "cos_phi" else 2] = 1.0
        b = new_batch("gym", dtype, cc, False)
        b.step(torch.from_numpy(cc["action"]).cuda())
        got = _np(b.get("euler"))[:, 1].astype(f)
        b.close()
        same = (got == w)                           # the sum 0 + v turns a -0 into +0
        assert same[inside].all(), (route, x[inside & ~same][:5], int((inside & ~same).sum()))
        same_edge += int(same[edge].sum())
    print(f"{dtype}: library results equal to the fast path's on {same_edge} of "
          f"{2 * int(edge.sum())} at the boundary")
    assert same_edge < 2 * int(edge.sum())


# ---------------------------------------------------------------------------
# c. every kernel form is bitwise the default step kernel
# ---------------------------------------------------------------------------
def _baseline(variant, dtype, monkeypatch):
    monkeypatch.setenv("DRONERL_ROWS_PER_WAVE", "64")
    monkeypatch.setenv("DRONERL_NT_LOADS", "0")
    c = es.corpus(dtype, variant)
    b = new_batch(variant, dtype, c, True)
    acts = actions_for(c)
    run = step_run(b, acts)
    out = (run, fields(b))
    b.close()
    return c, acts, out


@pytest.mark.parametrize("variant,dtype", [(v, "f64") for v in VARIANTS] + [("gym", "f32"),
                                                                           ("tag", "f32")] +
                         [(v, "f64") for v in KINDS] + [("waypoint", "f32")])
def test_step_forms_bitwise(variant, dtype, monkeypatch):
    """K = 4 dr_step launches with auto_reset from the corpus: 32 rows per
    wave and nontemporal state loads (the forms dr_create picks by batch
    size, forced by DRONERL_ROWS_PER_WAVE / DRONERL_NT_LOADS), the monitored
    kernel and the host-buffer step give the bit patterns of the 64-row plain
    form: obs, rew, done of every step and every state field."""
    c, acts, (run0, f0) = _baseline(variant, dtype, monkeypatch)
    d0 = _np(run0[2]).astype(bool)
    if variant != "vectorized":
        assert d0[0].sum() > 500 and d0[1].sum() > 500       # resets between the steps
    for rpw, ntl in (("32", "0"), ("64", "1"), ("32", "1")):
        monkeypatch.setenv("DRONERL_ROWS_PER_WAVE", rpw)
        monkeypatch.setenv("DRONERL_NT_LOADS", ntl)
        b = new_batch(variant, dtype, c, True)
        assert_same_run(step_run(b, acts), run0, fields(b), f0, (rpw, ntl))
        b.close()
    monkeypatch.setenv("DRONERL_ROWS_PER_WAVE", "64")
    monkeypatch.setenv("DRONERL_NT_LOADS", "0")
    b = new_batch(variant, dtype, c, True, monitor=True, keep_terminal_obs=True)
    trunc = torch.zeros(c["n"], dtype=torch.uint8, device="cuda")
    o, r, d = [], [], []
    for t in range(K):
        so, sr, sd = b.step(acts[t], trunc_out=trunc)
        o.append(so.clone()), r.append(sr.clone()), d.append(sd.clone())
        if t == 0 and variant != "vectorized":
            # crash and time limit in one step: not a truncation (block E holds
            # position; under wind it moves, to where the restatement has it:
            # at zero thrust no trig enters and the f64 kernel's position is
            # the restatement's bit for bit)
            pos1 = es.oracle_step(variant, c)[0]["pos"] if variant == "wind" else c["pos"]
            _, crash = es.done_predicate(variant, dtype, pos1, c["step"] + 1, c["max_steps"])
            e = es.rows_of(c, ("E",)) & np.isfinite(c["pos"]).all(1)
            if variant == "tag":
                crash = crash | crash[c["pairs"]]
            both = e & crash & (c["step"] + 1 >= c["max_steps"])
            only = e & ~crash & (c["step"] + 1 >= c["max_steps"])
            tr = _np(trunc).astype(bool)
            assert both.sum() >= 100 and only.sum() >= 100
            assert not tr[both].any() and tr[only].all()
    assert_same_run((torch.stack(o), torch.stack(r), torch.stack(d)), run0, fields(b), f0,
                    "monitor")
    b.close()
    b = new_batch(variant, dtype, c, True)
    for t in range(K):
        h = b.step_host(_np(acts[t]))
        for name, x, y in (("obs", h["obs"], run0[0][t]), ("rew", h["rew"], run0[1][t]),
                           ("done", h["done"], run0[2][t])):
            assert same_bits(torch.from_numpy(x.copy()), y), ("step_host", name, t)
    fb = fields(b)
    for k in f0:
        assert same_bits(fb[k], f0[k]), ("step_host", k)
    b.close()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS + KINDS)
def test_rollout_default_form_bitwise(variant, dtype):
    """dr_rollout in the form the size rule picks at the corpus' size (the
    split-physics kernel for gym, the warp-specialised one for moving and
    vectorized, the one-role kernel for smooth, tag and the gym options, whose
    words block F's resets redraw inside the launch) against K dr_step
    launches, resets from non-finite and out-of-range angles inside the
    launch: env_states_worker.check_rollout."""
    check_rollout(variant, dtype, "default form")


def test_rollout_random_default_form_bitwise():
    check_rollout_random("gym", "f64", "default form, in-kernel policy")


@pytest.mark.parametrize("variant,dtype,ws", [
    ("gym", "f64", "0"), ("gym", "f32", "0"), ("moving", "f64", "0"),
    ("vectorized", "f64", "0"), ("moving", "f32", "0"), ("gym", "f64", "1")])
def test_rollout_forced_form_bitwise(variant, dtype, ws):
    """The rollout form the size rule does not pick at this size
    (DRONERL_ROLLOUT_WS is read once per process, hence the subprocess), and
    with ws = 1 the in-kernel policy's warp-specialised gym kernel."""
    run_worker("env_states_worker.py", variant, dtype, ws, timeout=120, DRONERL_ROLLOUT_WS=ws)
