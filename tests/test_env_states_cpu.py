"""The env state corpus (tests/env_states.py) checked on the CPU alone: it is
what its docstring says, block E holds position on the oracle, blocks A-D
stay clear of every termination threshold (which is what lets the GPU tests
demand zero `done` flips there in both dtypes), and the two CPU oracles agree
over all of it inside the bound the GPU tests use."""
import numpy as np
import pytest

import env_states as es
from oracle import drone_np

VARIANTS = ("gym", "moving", "smooth", "tag", "vectorized")
DTYPES = ("f64", "f32")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_corpus_shape_and_determinism(variant, dtype):
    c = es.corpus(dtype, variant)
    n = c["n"]
    assert 8000 <= n <= 16000, n
    assert n % 64 and n % 256 and n % 2 == 0
    assert c["blocks"]["C_lanes"].start == 0 and c["blocks"]["C_lanes"].stop % 64 == 0
    for k in es.VEC:
        assert c[k].shape == (n, 3) and c[k].dtype == np.float64
        if dtype == "f32":
            with np.errstate(over="ignore"):
                back = c[k].astype(np.float32).astype(np.float64)
            assert es.same_bits_or_nan(back, c[k]).all(), k
    assert c["step"].dtype == np.int32 and c["action"].shape == (n, 4)
    assert ("motion" in c) == (variant == "moving") and ("motor" in c) == (variant == "smooth")
    assert ("pairs" in c) == (variant == "tag")
    for b in c["blocks"].values():
        assert (b.stop - b.start) % 2 == 0 and b.start % 2 == 0
    # a second build (cache dropped) gives the same bits
    es._CACHE.pop((dtype, variant))
    d = es.corpus(dtype, variant)
    for k in c:
        if isinstance(c[k], np.ndarray):
            assert es.same_bits_or_nan(c[k], d[k]).all() if c[k].dtype.kind == "f" \
                else np.array_equal(c[k], d[k]), k
    # what the blocks are for is in them
    e = c["euler"]
    out = np.abs(e) >= es.FAST
    lanes = out[c["blocks"]["C_lanes"]].any(1).reshape(-1, 64).sum(1)
    assert sorted(set(lanes.tolist())) == [1, 32, 64]
    assert np.isnan(e).any() and np.isinf(e).any() and out.any()
    assert np.isnan(c["pos"]).any() and np.isnan(c["vel"]).any() and np.isnan(c["omega"]).any()
    top = 1e299 if dtype == "f64" else 2.9e38
    assert (np.abs(e[np.isfinite(e)]) > top).any()


@pytest.mark.parametrize("dtype", DTYPES)
def test_worst_cancellations_cancel(dtype):
    """The chosen multiples leave a reduced argument far below an ulp of the
    argument: the reduction loses (almost) every bit of x there."""
    k, x = es.worst_cancellation(dtype, 128)
    import mpmath
    mpmath.mp.prec = 300
    r = np.array([abs(float(mpmath.mpf(float(xi)) - int(ki) * mpmath.pi / 2))
                  for ki, xi in zip(k, x)])
    f = es.ftype(dtype)
    ulp = np.spacing(np.abs(x).astype(f)).astype(np.float64)
    assert (r / ulp).max() < 2e-3 and (np.abs(x) < es.FAST).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_block_e_holds_position(variant, dtype):
    """f64: on the oracle itself.  f32: the oracle computes in f64, where
    RN32(g dt) does not cancel; there the kernel's z-velocity update is
    restated in np.float32 (one rounding per operation), and the oracle must
    stay within the velocity residual times dt."""
    c = es.corpus(dtype, variant)
    e = c["blocks"]["E"]
    f = es.ftype(dtype)
    v = f(es.hold_velocity(dtype))
    with np.errstate(all="ignore"):
        vz = v + (f(-es.G) + f(0)) * f(es.DT)
    assert vz == 0 and not np.signbit(vz)
    s, _, _, _ = es.oracle_step(variant, c)
    p0, p1 = c["pos"][e], s["pos"][e]
    ok = np.isfinite(p0).all(1)
    assert ok.sum() > 6000
    if dtype == "f64":
        assert np.array_equal(p0[ok], p1[ok])            # -0 == +0: the one bit that may change
        assert (s["vel"][e][ok] == 0).all()
    else:
        resid = abs(float(v) - es.G * es.DT) * es.DT
        # the residual, and the rounding of the oracle's position sum
        assert resid < 1e-9
        assert (np.abs(p1[ok] - p0[ok]) <= resid + np.spacing(np.abs(p0[ok]))).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS)
def test_blocks_a_to_d_clear_of_thresholds(variant, dtype):
    """Oracle post-position at least 1e-3 from pz = 0 and |p| = 50, the step
    counter two or more below the limit.  A NaN position compares false on
    both sides of any threshold and is clear of them all."""
    c = es.corpus(dtype, variant)
    m = es.rows_of(c, es.AD)
    s, _, _, done = es.oracle_step(variant, c)
    p = s["pos"][m]
    fin = np.isfinite(p).all(1)
    assert (p[fin][:, 2] >= 1e-3).all()
    assert (np.sqrt((p[fin] ** 2).sum(1)) <= 50 - 1e-3).all()
    assert (s["step"][m] <= c["max_steps"] - 2).all()
    assert not done[m].any()
    assert (~fin).sum() >= 8


@pytest.mark.parametrize("dtype", DTYPES)
def test_cpu_oracles_agree(dtype):
    """cref.gym_step (C, glibc) against drone_np.gym_step_batched (numpy) over
    the whole gym corpus: done exactly, non-finite patterns exactly, floats
    within gamma(c) x envelope with c = twice the reference-side count of
    env_states.rounding_counts (two f64 implementations of the same
    operations, each with 1 ulp library sin / cos / tan)."""
    c = es.corpus(dtype, "gym")
    s1, o1, r1, d1 = es.oracle_step("gym", c)
    s2 = {k: c[k].copy() for k in es.VEC}
    s2["step"] = c["step"].copy()
    with np.errstate(all="ignore"):
        o2, r2, d2 = drone_np.gym_step_batched(s2, c["action"])
    assert np.array_equal(d1, d2)
    oor = (~(np.abs(c["euler"]) < es.FAST)).any(1)
    cnt = es.bound_counts("f64", oor, both_cpu=True)
    env = es.envelopes("gym", c)
    u = es.unit_roundoff("f64")
    worst = {}
    for k in ("pos", "vel", "euler", "omega"):
        assert es.same_nonfinite(s2[k], s1[k]), k
        units, rel = es.worst_ratio(s2[k], s1[k], env[k], cnt[k], u)
        worst[k] = units
        assert rel <= 1.0, (k, units, rel)
    assert es.same_nonfinite(r2, r1) and es.same_nonfinite(o2, o1)
    units, rel = es.worst_ratio(r2, r1, env["rew"] + 1.0, cnt["rew"], u)
    assert rel <= 1.0, ("rew", units, rel)
    # the obs are the f32 casts of states that differ by the above
    fin = np.isfinite(o1)
    assert (np.abs(o2[fin].astype(np.float64) - o1[fin]) <=
            2.0 ** -23 * np.abs(o1[fin]) + 1e-44).all()
    print("worst |cref - drone_np| in u x envelope:", worst)


def test_checks_reject_wrong_results():
    """The shared checks are not vacuous: a kernel wrong in the 9th digit near
    gimbal lock, a flipped infinity and a wrong bonus all fail them."""
    c = es.corpus("f64", "gym")
    s, _, rew, _ = es.oracle_step("gym", c)
    env = es.envelopes("gym", c)
    oor = (~(np.abs(c["euler"]) < es.FAST)).any(1)
    cnt = es.bound_counts("f64", oor)
    bad = s["euler"].copy()
    b = c["blocks"]["B"]
    bad[b] *= 1 + 1e-9
    _, rel = es.worst_ratio(bad, s["euler"], env["euler"], cnt["euler"], 2.0 ** -53)
    assert rel > 1e3
    x = np.array([np.inf, 1.0, np.nan])
    assert es.same_nonfinite(x, x) and not es.same_nonfinite(-x, x)
    assert not es.same_nonfinite(np.array([1.0, 1.0, np.nan]), x)
    r = es.reward_exact("gym", "f64", s["pos"], c["target"])
    fin = np.isfinite(rew)
    assert np.abs(r[fin] - rew[fin]).max() < 1e-6
    assert ((r > 0.5) & fin).sum() >= 50 and ((r < 0.5) & fin).sum() >= 50
