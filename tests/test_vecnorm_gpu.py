"""dr_vecnorm_* on the device against the NumPy f64 restatement
(tests/vecnorm_ref.py).

Bounds, from the issue that introduced the kernels: after every step
|mean - mean_ref| <= 1e-12 sqrt(var_ref + eps), |var - var_ref| <= 1e-12
(var_ref + eps), equal counts, outputs within 1 f32 ulp and at most 1e-3 of
the output elements different at all.  (An f64 emulation of a blocked Chan
reduction differed from np.mean / np.var by <= 2e-14 on such inputs: the bound
leaves ~50x for another merge tree.)

Sizes: N in {1, 2, 257, 4099} and N_LEVELS = 20001, which crosses every
reduction level of the implementation: 79 row tiles of 256 (the last one of
33 rows), so the slice walk, the slice merge and the 256-leaf returns tree see
a full and a partial tile, the finish's lanes 0..14 merge two partials each
(the strided loop) and all 64 lanes enter the shuffle tree.
"""
import numpy as np
import pytest
import torch

from vecnorm_ref import SENTINEL, VecNormalizeRef, make_sequence, ulp_diff

pytestmark = pytest.mark.gpu

N_LEVELS = 20001
EPS = 1e-8
SHAPES = [(n, d) for n in (1, 2, 257, 4099, N_LEVELS) for d in (12, 15, 16, 18, 19)]


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _vn(n, d, **kw):
    from drone_rl_amd import ppo_kernels as K
    return K.VecNormalize(n, d, torch.device("cuda", 0), gamma=0.99, clip_obs=10.0,
                          clip_reward=10.0, epsilon=EPS, **kw)


_SEQ = {}


def sequence(n, d):
    """Inputs and the restatement's results, computed once per shape and
    never modified."""
    if (n, d) not in _SEQ:
        seq = make_sequence(n, d, seed=1000 * d + n % 997)
        ref = VecNormalizeRef(n, d, epsilon=EPS)
        out = {"reset": (ref.reset(seq["reset"]), ref.stats(), ref.returns.copy()), "steps": []}
        for s in seq["steps"]:
            sent = np.full((n, d), SENTINEL, np.float32)
            res = ref.step(s["obs"], s["rew"], s["done"], s["term"], sent)
            out["steps"].append((res, ref.stats(), ref.returns.copy()))
        _SEQ[(n, d)] = (seq, out)
    return _SEQ[(n, d)]


def check_stats(vn, ref_stats, d, where):
    o_ref, r_ref = ref_stats
    o, r = vn.obs_rms.cpu().numpy(), vn.ret_rms.cpu().numpy()
    assert o[0] == o_ref[0] and r[0] == r_ref[0], f"{where}: counts"
    mean, var = o[1:1 + d], o[1 + d:]
    mean_ref, var_ref = o_ref[1:1 + d], o_ref[1 + d:]
    em = np.abs(mean - mean_ref) / np.sqrt(var_ref + EPS)
    ev = np.abs(var - var_ref) / (var_ref + EPS)
    er = max(abs(r[1] - r_ref[1]) / np.sqrt(r_ref[2] + EPS), abs(r[2] - r_ref[2]) / (r_ref[2] + EPS))
    print(f"{where}: mean err {em.max():.3e} var err {ev.max():.3e} ret err {er:.3e}")
    assert em.max() <= 1e-12, f"{where}: obs mean"
    assert ev.max() <= 1e-12, f"{where}: obs var"
    assert er <= 1e-12, f"{where}: ret_rms"


def check_out(got, ref, where, counter):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and np.isfinite(ref).all()
    u = ulp_diff(got, ref)
    counter[0] += int((u != 0).sum())
    counter[1] += u.size
    assert u.max() <= 1, f"{where}: {u.max()} ulp"


@pytest.mark.parametrize("n,d", SHAPES)
def test_reset_and_six_steps_follow_the_restatement(n, d):
    seq, ref = sequence(n, d)
    vn = _vn(n, d)
    diff = [0, 0]
    o = vn.reset(_dev(seq["reset"]))
    check_stats(vn, ref["reset"][1], d, "reset")
    check_out(o, ref["reset"][0], "reset obs", diff)
    assert torch.equal(vn.returns, torch.zeros_like(vn.returns))
    lo = hi = rlo = rhi = False
    for k, (s, (res, stats, returns)) in enumerate(zip(seq["steps"], ref["steps"])):
        term_out = torch.full((n, d), float(SENTINEL), device="cuda")
        o, r, t = vn.step(_dev(s["obs"]), _dev(s["rew"]), _dev(s["done"]), _dev(s["term"]),
                          term_out=term_out)
        check_stats(vn, stats, d, f"step {k}")
        check_out(o, res[0], f"step {k} obs", diff)
        check_out(r, res[1], f"step {k} rew", diff)
        check_out(t, res[2], f"step {k} term", diff)
        done = s["done"].astype(bool)
        # rows of envs that are not done keep the sentinel, bit for bit
        assert np.all(t.cpu().numpy()[~done] == SENTINEL)
        got_ret = vn.returns.cpu().numpy()
        assert np.all(got_ret[done] == 0.0)
        assert np.all(np.abs(got_ret - returns) <= 1e-12 * np.maximum(np.abs(returns), 1.0))
        lo |= bool((res[0] == -10.0).any())
        hi |= bool((res[0] == 10.0).any())
        rlo |= bool((res[1] == -10.0).any())
        rhi |= bool((res[1] == 10.0).any())
    if n >= 257:
        # both clip ends engage, on the restatement (a z-score above 10 needs
        # more than 100 samples: (k - 1) / sqrt(k) bounds it, so N = 1 and 2
        # with their 7 and 14 samples per column cannot reach the clip)
        assert lo and hi and rlo and rhi
    print(f"N={n} D={d}: {diff[0]} of {diff[1]} output elements differ")
    assert diff[0] <= 1e-3 * diff[1]


def test_sequence_has_the_required_done_patterns_and_constant_column():
    seq, _ = sequence(257, 16)
    dones = [s["done"] for s in seq["steps"]]
    assert not dones[1].any() and dones[3].all()
    assert any(0 < x.sum() < x.size for x in dones)
    c = seq["steps"][2]["obs"][:, 8]
    assert np.all(c == c[0])


def _run(n, d, steps=4, **kw):
    """reset + steps on a fresh normaliser; every output and the final state."""
    seq, _ = sequence(n, d)
    vn = _vn(n, d, **kw)
    outs = [vn.reset(_dev(seq["reset"]))]
    for s in seq["steps"][:steps]:
        outs += list(vn.step(_dev(s["obs"]), _dev(s["rew"]), _dev(s["done"]), _dev(s["term"]),
                             term_out=torch.full((n, d), float(SENTINEL), device="cuda")))
    return vn, outs


def test_two_runs_are_bitwise_equal():
    a, oa = _run(N_LEVELS, 19)
    b, ob = _run(N_LEVELS, 19)
    for x, y in zip(oa, ob):
        assert torch.equal(x, y)
    for k in ("obs_rms", "ret_rms", "returns"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k


def test_frozen_statistics_are_bitwise_unchanged():
    n, d = 4099, 15
    seq, _ = sequence(n, d)
    vn, _ = _run(n, d, steps=2)
    ref = VecNormalizeRef(n, d, epsilon=EPS)
    ref.reset(seq["reset"])
    for s in seq["steps"][:2]:
        ref.step(s["obs"], s["rew"], s["done"])
    before = (vn.obs_rms.clone(), vn.ret_rms.clone(), vn.returns.clone())
    # the restatement continues from the DEVICE's statistics (frozen from here)
    ref.obs_rms.count = float(before[0][0])
    ref.obs_rms.mean = before[0][1:1 + d].cpu().numpy()
    ref.obs_rms.var = before[0][1 + d:].cpu().numpy()
    ref.ret_rms.var = float(before[1][2])
    ref.returns = before[2].cpu().numpy().copy()
    vn.training = ref.training = False
    s = seq["steps"][2]
    o, r = vn.step(_dev(s["obs"]), _dev(s["rew"]), _dev(s["done"]))
    ro, rr = ref.step(s["obs"], s["rew"], s["done"])
    assert torch.equal(vn.obs_rms, before[0]) and torch.equal(vn.ret_rms, before[1])
    # returns: not advanced, zeroed where done
    exp = before[2].clone()
    exp[_dev(s["done"]).bool()] = 0.0
    assert torch.equal(vn.returns, exp)
    assert ulp_diff(o.cpu().numpy(), ro).max() <= 1 and ulp_diff(r.cpu().numpy(), rr).max() <= 1
    vn.reset(_dev(seq["reset"]))
    assert torch.equal(vn.obs_rms, before[0]) and not vn.returns.any()


@pytest.mark.parametrize("norm_obs,norm_reward", [(True, False), (False, True)])
def test_single_flag(norm_obs, norm_reward):
    n, d = 4099, 18
    seq, _ = sequence(n, d)
    kw = dict(norm_obs=norm_obs, norm_reward=norm_reward)
    vn = _vn(n, d, **kw)
    ref = VecNormalizeRef(n, d, epsilon=EPS, **kw)
    init_obs, init_ret = vn.obs_rms.clone(), vn.ret_rms.clone()
    raw0 = _dev(seq["reset"])
    o = vn.reset(raw0)
    ro = ref.reset(seq["reset"])
    assert ulp_diff(o.cpu().numpy(), ro).max() <= 1
    for k, s in enumerate(seq["steps"][:3]):
        raw, rew = _dev(s["obs"]), _dev(s["rew"])
        term_out = torch.full((n, d), float(SENTINEL), device="cuda")
        o, r, t = vn.step(raw, rew, _dev(s["done"]), _dev(s["term"]), term_out=term_out)
        ro, rr, rt = ref.step(s["obs"], s["rew"], s["done"], s["term"],
                              np.full((n, d), SENTINEL, np.float32))
        check_stats(vn, ref.stats(), d, f"step {k}")
        for got, want in ((o, ro), (r, rr), (t, rt)):
            assert ulp_diff(got.cpu().numpy(), want).max() <= 1
        if not norm_obs:
            # a plain copy, the terminal rows of done envs included
            assert torch.equal(o, raw)
            assert np.array_equal(t.cpu().numpy(), rt)
        if not norm_reward:
            assert torch.equal(r, rew)
    if not norm_obs:
        assert torch.equal(vn.obs_rms, init_obs)
    if not norm_reward:
        # the stated deviation from SB3: ret_rms untouched, returns never advance
        assert torch.equal(vn.ret_rms, init_ret) and not vn.returns.any()


def test_in_place_equals_out_of_place():
    n, d = 4099, 15
    seq, _ = sequence(n, d)
    a, oa = _run(n, d, steps=3)
    vn = _vn(n, d)
    x = _dev(seq["reset"])
    assert vn.reset(x, out=x) is x
    outs = [x]
    for s in seq["steps"][:3]:
        obs, rew = _dev(s["obs"]), _dev(s["rew"])
        term_out = torch.full((n, d), float(SENTINEL), device="cuda")
        vn.step(obs, rew, _dev(s["done"]), _dev(s["term"]), obs_out=obs, rew_out=rew,
                term_out=term_out)
        outs += [obs, rew, term_out]
    for p, q in zip(oa, outs):
        assert torch.equal(p, q)
    for k in ("obs_rms", "ret_rms", "returns"):
        assert torch.equal(getattr(a, k), getattr(vn, k)), k


def test_graph_replay_equals_eager_bitwise():
    n, d = N_LEVELS, 16
    seq, _ = sequence(n, d)
    steps = seq["steps"][:3]
    eager, oe = _run(n, d, steps=3)

    vn = _vn(n, d)
    ins = [(_dev(s["obs"]), _dev(s["rew"]), _dev(s["done"]), _dev(s["term"])) for s in steps]
    outs = [(torch.empty(n, d, device="cuda"), torch.empty(n, device="cuda"),
             torch.empty(n, d, device="cuda")) for _ in steps]
    vn.reset(_dev(seq["reset"]))
    state0 = (vn.obs_rms.clone(), vn.ret_rms.clone(), vn.returns.clone())
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs), torch.cuda.graph(g, stream=cs):
        for (o, r, dn, t), (oo, ro, to) in zip(ins, outs):
            vn.step(o, r, dn, t, obs_out=oo, rew_out=ro, term_out=to)
    torch.cuda.current_stream().wait_stream(cs)
    for _ in range(2):              # the second replay starts from the same state
        vn.obs_rms.copy_(state0[0])
        vn.ret_rms.copy_(state0[1])
        vn.returns.copy_(state0[2])
        for _, _, to in outs:
            to.fill_(float(SENTINEL))
        g.replay()
        torch.cuda.synchronize()
        flat = [x for trio in outs for x in trio]
        for p, q in zip(oe[1:], flat):
            assert torch.equal(p, q)
        for k in ("obs_rms", "ret_rms", "returns"):
            assert torch.equal(getattr(eager, k), getattr(vn, k)), k


@pytest.mark.parametrize("m", [1, 300, 5000])
def test_normalize_obs_at_another_row_count(m):
    n, d = 257, 19
    seq, _ = sequence(n, d)
    vn, _ = _run(n, d, steps=2)
    ref = VecNormalizeRef(n, d, epsilon=EPS)
    o = vn.obs_rms.cpu().numpy()
    ref.obs_rms.mean, ref.obs_rms.var = o[1:1 + d], o[1 + d:]
    before = vn.obs_rms.clone()
    x = np.resize(np.concatenate([s["obs"] for s in seq["steps"]]), (m, d)).astype(np.float32)
    got = vn.normalize_obs(_dev(x))
    want = ref.normalize_obs(x).astype(np.float32)
    assert ulp_diff(got.cpu().numpy(), want).max() <= 1
    assert (ulp_diff(got.cpu().numpy(), want) != 0).mean() <= 1e-3
    assert torch.equal(vn.obs_rms, before)
    # and back, where the clip did not engage
    back = vn.unnormalize_obs(got).cpu().numpy()
    inside = np.abs(want) < 10.0
    sd = np.sqrt(ref.obs_rms.var + EPS)
    assert np.all(np.abs(back - x)[inside] <= (2e-6 * (np.abs(x) + 10.0 * sd))[inside])


def test_state_dict_and_npz_round_trip(tmp_path):
    n, d = 257, 12
    a, _ = _run(n, d, steps=2)
    b = _vn(n, d, norm_reward=False)
    b.load_state_dict(a.state_dict())
    for k in ("obs_rms", "ret_rms", "returns"):
        assert torch.equal(getattr(a, k), getattr(b, k)), k
    assert b.norm_reward and b.flags() == a.flags()
    p = str(tmp_path / "vn.npz")
    a.save_npz(p)
    with np.load(p) as z:
        assert set(a.NPZ_KEYS) <= set(z.files)
        assert z["obs_mean"].shape == (d,) and z["obs_var"].dtype == np.float64
    c = _vn(n, d)
    c.load_npz(p)
    assert torch.equal(a.obs_rms, c.obs_rms) and torch.equal(a.ret_rms, c.ret_rms)
    assert not c.returns.any()
