"""The env state corpus (tests/env_states.py) checked on the CPU alone: it is
what its docstring says, block E holds position on the oracle, blocks A-D
stay clear of every termination threshold (which is what lets the GPU tests
demand zero `done` flips there in both dtypes), and the two CPU oracles agree
over all of it inside the bound the GPU tests use.  The gym options' kinds
(wind, waypoint, airframe) get the same, on their restatements: block E still
straddles its thresholds -- under wind because it is derived from the
restatement's vel_new dt -- and each restatement in a deliberately wrong form
fails the shared checks."""
import numpy as np
import pytest

import env_states as es
from oracle import drone_np

VARIANTS = ("gym", "moving", "smooth", "tag", "vectorized")
KINDS = tuple(es.OPTIONS)               # the gym options: wind, waypoint, airframe
DTYPES = ("f64", "f32")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("variant", VARIANTS + KINDS)
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
    for k in KINDS:
        assert (k in c) == (variant == k)
    assert ("eps" in c) == (variant == "waypoint") and ("ep_num" in c) == (variant in KINDS)
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
@pytest.mark.parametrize("variant", VARIANTS + ("waypoint", "airframe"))
def test_block_e_holds_position(variant, dtype):
    """f64: on the oracle itself.  f32: the oracle computes in f64, where
    RN32(g dt) does not cancel; there the kernel's z-velocity update is
    restated in np.float32 (one rounding per operation), and the oracle must
    stay within the velocity residual times dt.  Waypoints do not touch the
    physics, and at zero thrust the airframe's 1/m multiplies a zero; the wind
    kind does not hold position (test_wind_block_e_lands_where_designed)."""
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
@pytest.mark.parametrize("variant", VARIANTS + KINDS)
def test_blocks_a_to_d_clear_of_thresholds(variant, dtype):
    """Oracle post-position at least 1e-3 from pz = 0 and |p| = 50, the step
    counter two or more below the limit.  A NaN position compares false on
    both sides of any threshold and is clear of them all.  wind: block D's
    rows at the largest finite f32 and at inf are blown 1e34 m and further
    past the thresholds, as clear of them on the far side; they alone are
    done."""
    c = es.corpus(dtype, variant)
    m = es.rows_of(c, es.AD)
    s, _, _, done = es.oracle_step(variant, c)
    blown = np.zeros(c["n"], bool)
    if variant == "wind":
        with np.errstate(invalid="ignore"):
            blown = c["wind_special"] & (np.abs(c["wind"]) > 1e38).any(1)
        assert 20 <= blown.sum() <= 40 and not blown[~m].any()
        q = s["pos"][blown]
        nan = np.isnan(q).any(1)                    # inf - inf in the air's velocity
        assert (np.abs(q[~nan]).max(1) > 1e34).all()
        assert done[blown][~nan].all() and not done[blown][nan].any()
        assert np.isinf(q).any(1).sum() >= 6 and np.isfinite(q).all(1).sum() >= 6
    p = s["pos"][m & ~blown]
    fin = np.isfinite(p).all(1)
    assert (p[fin][:, 2] >= 1e-3).all()
    assert (np.sqrt((p[fin] ** 2).sum(1)) <= 50 - 1e-3).all()
    assert (s["step"][m] <= c["max_steps"] - 2).all()
    assert not done[m & ~blown].any()
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


@pytest.mark.parametrize("dtype", DTYPES)
def test_wind_block_e_lands_where_designed(dtype):
    """The wind kind's block E is derived from the restatement's vel_new dt:
    on the restatement the ground rows land within 3 ulp of -vel_new_z dt of
    pz = 0, on both sides and on it, and the axis rows of the bonus edge at the
    edge's distance exactly."""
    c = es.corpus(dtype, "wind")
    e = c["blocks"]["E"]
    assert np.isfinite(c["wind"][e]).all() and not c["wind_special"][e].any()
    s, _, _, _ = es.oracle_step("wind", c)
    third = (e.stop - e.start) // 3
    rows = e.start + np.array([t * third + r for t in range(3) for r in range(6)])
    pz = s["pos"][rows, 2]
    scale = np.spacing(np.abs(es.rn(s["vel"][rows, 2] * es.DT, dtype)).astype(es.ftype(dtype)))
    assert (np.abs(pz) <= 4.0 * scale).all()
    assert (pz < 0).sum() >= 3 and (pz >= 0).sum() >= 3
    if dtype == "f64":
        assert (pz == 0).sum() >= 6
        d = np.sqrt(((s["pos"] - c["target"])[e] ** 2).sum(1))
        for k in range(-3, 4):
            assert (d == es.ulp_steps(0.05, k, dtype)).sum() >= 3, k


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("kind", KINDS)
def test_option_block_e_straddles_its_thresholds(kind, dtype):
    """On the restatement alone: more than 1000 done and more than 1000
    not-done rows in block E, at least 20 finite rows on each side of the
    bonus / reach edge; waypoint: the reference's d is R itself and each of its
    1..3 ulp neighbours (state dtype) on some row, at least 20 rows reach in
    the step that crashes and 20 in the step that times out, and every (j,
    eps) pair of the designed values is among the reaches."""
    c = es.corpus(dtype, kind)
    e = es.rows_of(c, ("E",))
    s, _, rew, done = es.oracle_step(kind, c)
    assert (done & e).sum() > 1000 and (~done & e).sum() > 1000
    fin = np.isfinite(rew) & e
    assert (fin & (rew > 0.4)).sum() >= 20 and (fin & (rew < 0.4)).sum() >= 20
    if kind == "waypoint":
        R = es.bonus_edge("waypoint")
        assert R != 0.3 and R == float(np.float32(0.3))
        for k in range(-3, 4):
            on = e & (s["d"] == es.ulp_steps(R, k, dtype))
            assert on.sum() >= 3 and (s["reached"][on] == (k < 0)).all(), k
        _, crash = es.done_predicate("gym", "f64", s["pos"], s["step"], c["max_steps"])
        assert (e & s["reached"] & crash).sum() >= 20
        assert (e & s["reached"] & ~crash & (s["step"] >= c["max_steps"])).sum() >= 20
        assert (e & ~s["reached"] & (np.abs(s["d"] - R) < 1e-6)).sum() >= 20
        pairs = {(int(j), float(x)) for j, x in zip(c["waypoint"][s["reached"], 0],
                                                    c["eps"][s["reached"]])}
        assert len(pairs) == 15
        if dtype == "f64":
            assert (e & (s["d"] >= 0.3) & (s["d"] < R)).sum() >= 3      # literal vs (S)radius
    if kind == "airframe":
        af = c["airframe"]
        lo, hi = np.float32(1) - np.float32(0.9), np.float32(1) + np.float32(0.9)
        ad = es.rows_of(c, es.AD)
        for col, v in ((0, lo), (0, hi), (1, lo), (1, hi), (2, np.float32(0.5)),
                       (5, np.float32(1.5))):
            assert (ad & (af[:, col] == v)).sum() >= 100, (col, v)
        assert (ad & (af == 1).all(1)).sum() >= 100
        assert af[:, :2].min() >= lo and af[:, :2].max() <= hi
        assert af[:, 2:].min() >= 0.5 and af[:, 2:].max() <= 1.5
    if kind == "wind":
        w = c["wind"][c["wind_special"]]
        assert np.isnan(w).any() and np.isinf(w).any() and np.signbit(w[w == 0]).any()
        assert (np.abs(w) == np.finfo(np.float32).max).any()


def _check_failures(kind, c, got, rew, ref, rr):
    """The checks of test_step_matches_oracle that a CPU result (got, rew)
    fails against the restatement's (ref, rr), both f64: the float bound per
    field and on the reward, the reward recomputed from the stored position,
    and the option's exact predicates."""
    u = es.unit_roundoff("f64")
    oor = (~(np.abs(c["euler"]) < es.FAST)).any(1)
    cnt = es.bound_counts("f64", oor, both_cpu=True, variant=kind)
    env = es.envelopes(kind, c)
    bad = []
    for k in ("pos", "vel", "euler", "omega"):
        _, rel = es.worst_ratio(got[k], ref[k], env[k], cnt[k], u)
        if rel > 1.0 or not es.same_nonfinite(got[k], ref[k]):
            bad.append(k)
    _, rel = es.worst_ratio(rew, rr, env["rew"] + 1.0, cnt["rew"], u)
    if rel > 1.0:
        bad.append("rew")
    with np.errstate(all="ignore"):
        want = es.reward_exact(kind, "f64", got["pos"], c["target"])
        if not es.same_bits_or_nan(np.asarray(rew, np.float64).astype(np.float32), want).all():
            bad.append("reward_exact")
    return bad + es.option_exact_failures(kind, "f64", c, got)


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
    # the options' restatements in their deliberately wrong forms: each breaks
    # the float bound or an exact predicate somewhere on its corpus, and the
    # right form breaks none
    expect = {("airframe", "gravity"): "vel", ("airframe", "yaw"): "omega",
              ("airframe", "f64_recip"): "vel", ("wind", "no_gust"): "vel",
              ("wind", "drag_after"): "vel", ("waypoint", "reach_le"): "counters",
              ("waypoint", "reward_new"): "reward_exact"}
    for kind in KINDS:
        c = es.corpus("f64", kind)
        ref, ro, rr, _ = es.oracle_step(kind, c)
        assert _check_failures(kind, c, ref, rr, ref, rr) == []
        for (k, fault), name in expect.items():
            if k != kind:
                continue
            got, go, gr, _ = es.oracle_step(kind, c, fault=fault)
            bad = _check_failures(kind, c, got, gr, ref, rr)
            print(kind, fault, "fails", bad)
            assert name in bad, (kind, fault, bad)
            if fault == "f64_recip":
                # ... which the 1e-5 bar on the obs lets through
                fin = np.isfinite(ro) & np.isfinite(go)
                with np.errstate(invalid="ignore"):
                    err = np.abs(go.astype(np.float64) - ro) / np.maximum(np.abs(ro), 1.0)
                assert err[fin].max() <= 1e-5
