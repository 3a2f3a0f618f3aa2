"""GPU checks of the PPO HIP kernels against the CPU restatement of SB3's
PPO arithmetic (oracle/ppo_ref.py, oracle/ppo_ref.c).  SB3 itself is not
available, so these are "parity unpinned" w.r.t. the reference; they pin the
kernels to the restatement: GAE bit-exact, Philox-derived streams bit-exact,
float loss/gradients within 1e-5 (f32 reduction-order differences)."""
import numpy as np
import pytest
import torch

from oracle import cref, ppo_ref

pytestmark = pytest.mark.gpu


def test_gae_bitexact_vs_oracle():
    from drone_rl_amd import ppo_kernels as K
    rng = np.random.default_rng(0)
    T, N = 32, 50_000
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T, N)).astype(np.float32)
    st = (rng.random((T, N)) < 0.05).astype(np.uint8)
    lv = rng.normal(size=N).astype(np.float32)
    ld = (rng.random(N) < 0.05).astype(np.uint8)
    cu = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    adv, ret = K.gae(cu(r), cu(v), cu(st), cu(lv), cu(ld), 0.99, 0.95)
    ra, rr = cref.gae(r, v, st, lv, ld, 0.99, 0.95)
    np.testing.assert_array_equal(adv.cpu().numpy(), ra)
    np.testing.assert_array_equal(ret.cpu().numpy(), rr)


def test_policy_sample_distribution_and_logp():
    from drone_rl_amd import ppo_kernels as K
    n = 1 << 20
    mean = torch.randn(n, 4, device="cuda")
    log_std = torch.tensor([0.0, -0.5, 0.3, -1.0], device="cuda")
    raw = torch.empty_like(mean)
    clip = torch.empty_like(mean)
    logp = torch.empty(n, device="cuda")
    K.policy_sample(mean, log_std, seed=5, counter=17, lo=0.0, hi=7.3575,
                    actions_raw=raw, actions_clipped=clip, logp=logp)
    z = (raw - mean) / log_std.exp()
    assert abs(z.mean().item()) < 5e-3 and abs(z.std().item() - 1) < 5e-3
    assert abs(((z.abs() < 1).float().mean() - 0.6827).item()) < 3e-3
    d = torch.distributions.Normal(mean, log_std.exp())
    ref = d.log_prob(raw).sum(1)
    assert torch.allclose(logp, ref, rtol=1e-5, atol=1e-5)
    assert torch.equal(clip, raw.clamp(0.0, 7.3575))
    # same (seed, counter) -> same draws; different counter -> different
    raw2 = torch.empty_like(mean)
    K.policy_sample(mean, log_std, 5, 17, 0.0, 7.3575, actions_raw=raw2)
    assert torch.equal(raw, raw2)
    K.policy_sample(mean, log_std, 5, 18, 0.0, 7.3575, actions_raw=raw2)
    assert not torch.equal(raw, raw2)


def test_permutation_valid_and_matches_philox_sort():
    from drone_rl_amd import ppo_kernels as K
    n = 5000
    perm = K.Permuter(n, "cuda")(seed=9, counter=3).cpu().numpy()
    assert np.array_equal(np.sort(perm), np.arange(n))
    keys = np.zeros(n, np.uint64)
    for i in range(n):
        r = cref.philox([i, 0, 3, 0x50000000], [9, 0])
        keys[i] = (np.uint64(r[0]) << np.uint64(32)) | np.uint64(r[1])
    np.testing.assert_array_equal(perm, np.argsort(keys, kind="stable"))
    big = K.Permuter(1 << 21, "cuda")(seed=1, counter=0)
    assert torch.equal(torch.sort(big.long()).values,
                       torch.arange(1 << 21, device="cuda"))


@pytest.mark.parametrize("n", [1, 2, 1000, 1025, 4097, 70001, 1 << 21])
def test_permutation_is_the_stable_key_argsort(n):
    """Bucket pass + per-bucket bitonic sorts == the stable argsort of the
    64-bit Philox keys (oracle/cref.permutation_np), at ragged sizes and at
    configs[2]'s 32 x 65,536 rollout rows; bitwise deterministic."""
    from drone_rl_amd import ppo_kernels as K
    p = K.Permuter(n, "cuda")
    got = p(seed=0x1234567890, counter=(7 << 32) + 5).cpu().numpy()
    np.testing.assert_array_equal(got, cref.permutation_np(n, 0x1234567890, (7 << 32) + 5))
    again = p(seed=0x1234567890, counter=(7 << 32) + 5, out=torch.empty_like(p.out))
    assert np.array_equal(again.cpu().numpy(), got)


def test_permutation_global_scratch_path(monkeypatch):
    """Buckets above the LDS capacity sort in global scratch (forced here by
    DRONERL_PERM_LDS_CAP; unreachable in practice at a mean of <= 1024)."""
    from drone_rl_amd import ppo_kernels as K
    for cap in ("0", "700"):
        monkeypatch.setenv("DRONERL_PERM_LDS_CAP", cap)
        n = 9000
        got = K.Permuter(n, "cuda")(seed=3, counter=11).cpu().numpy()
        np.testing.assert_array_equal(got, cref.permutation_np(n, 3, 11))


def test_permutation_graph_replays_are_fresh():
    """The permutation captured into a hipGraph (counter base on the device)
    replays to the eager permutation of each new counter, at configs[2]'s
    2,097,152 rows and 10 epochs per graph (rocPRIM's radix sort faulted on
    the second replay of such a graph; the bucket sort keeps no state)."""
    from drone_rl_amd import ppo_kernels as K
    n, E = 1 << 21, 10
    p = K.Permuter(n, "cuda")
    ctr = torch.zeros(1, dtype=torch.int64, device="cuda")
    outs = torch.zeros(E, n, dtype=torch.int32, device="cuda")

    def body():
        for e in range(E):
            p.dev(seed=7, counter_base=ctr, counter_offset=e, out=outs[e])
    body()
    torch.cuda.synchronize()
    cs = torch.cuda.Stream()
    cs.wait_stream(torch.cuda.current_stream())
    g = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs), torch.cuda.graph(g, stream=cs):
        body()
    torch.cuda.current_stream().wait_stream(cs)
    for it in range(3):
        ctr.fill_(it * E)
        g.replay()
        torch.cuda.synchronize()
        for e in (0, E - 1):
            ref = p(seed=7, counter=it * E + e, out=torch.empty_like(p.out))
            assert torch.equal(ref, outs[e]), (it, e)


def test_gather_rows_exact():
    from drone_rl_amd import ppo_kernels as K
    src = torch.randn(100_000, 15, device="cuda")
    idx = torch.randint(0, 100_000, (4096,), device="cuda", dtype=torch.int32)
    assert torch.equal(K.gather_rows(idx, src), src[idx.long()])


@pytest.mark.parametrize("normalize", [True, False])
def test_ppo_loss_vs_torch_autograd(normalize):
    from drone_rl_amd import ppo_kernels as K
    rng = np.random.default_rng(1)
    m = 65536
    mean = rng.normal(2.0, 1.0, (m, 4)).astype(np.float32)
    log_std = np.array([0.1, -0.3, 0.0, 0.2], np.float32)
    actions = (mean + np.exp(log_std) * rng.normal(size=(m, 4))).astype(np.float32)
    old_logp = (rng.normal(-5.0, 1.0, m)).astype(np.float32)
    # make the ratio land on both sides of the clip interval
    d = torch.distributions.Normal(torch.from_numpy(mean), torch.from_numpy(np.exp(log_std)))
    lp = d.log_prob(torch.from_numpy(actions)).sum(1).numpy()
    old_logp = (lp - rng.normal(0, 0.2, m)).astype(np.float32)
    adv = rng.normal(0.3, 2.0, m).astype(np.float32)
    returns = rng.normal(size=m).astype(np.float32)
    values = rng.normal(size=m).astype(np.float32)
    stats, gm, gls, gv = ppo_ref.ppo_loss_torch(mean, log_std, values, actions, old_logp,
                                                adv, returns, 0.2, 0.01, 0.5, normalize)
    L = K.PPOLoss(m, "cuda", 0.2, 0.01, 0.5, normalize)
    cu = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    g_mean, g_ls, g_v, st = L(cu(mean), cu(log_std), cu(values), cu(actions), cu(old_logp),
                              cu(adv), cu(returns))
    st = st.cpu().numpy()
    names = ["loss", "policy_loss", "value_loss", "entropy_loss", "clip_fraction", "approx_kl"]
    for k, name in enumerate(names):
        assert abs(st[k] - stats[name]) <= 1e-5 * max(1.0, abs(stats[name])), name
    assert 0.05 < stats["clip_fraction"] < 0.95
    scale = np.abs(gm).max()
    np.testing.assert_allclose(g_mean.cpu().numpy(), gm, rtol=0, atol=1e-4 * scale)
    np.testing.assert_allclose(g_v.cpu().numpy(), gv, rtol=0, atol=1e-6)
    np.testing.assert_allclose(g_ls.cpu().numpy(), gls, rtol=1e-4, atol=1e-5)
    # the interleaved (m,3) aux form (the trainer's gathered rollout rows)
    # reads the same numbers: identical outputs
    keep = [t.clone() for t in (g_mean, g_ls, g_v, L.stats)]
    aux = cu(np.stack([old_logp, adv, returns], 1).copy())
    out = L(cu(mean), cu(log_std), cu(values), cu(actions), aux=aux)
    for a, b in zip(keep, out):
        assert torch.equal(a, b)


def test_clip_adam_vs_torch():
    from drone_rl_amd import ppo_kernels as K
    rng = np.random.default_rng(2)
    n = 141_065
    p = rng.normal(size=n).astype(np.float32)
    for gscale, step in ((10.0, 1), (1e-4, 7)):   # clipped, and not clipped
        g = (rng.normal(size=n) * gscale / np.sqrt(n)).astype(np.float32)
        m = (rng.normal(size=n) * 1e-3).astype(np.float32)
        v = (rng.random(n) * 1e-6).astype(np.float32)
        rp, rm, rv, rg, rnorm = ppo_ref.clip_adam_torch(p, g, m, v, step)
        opt = K.ClipAdam(torch.from_numpy(p.copy()).cuda())
        opt.m.copy_(torch.from_numpy(m))
        opt.v.copy_(torch.from_numpy(v))
        opt.t = step - 1
        gd = torch.from_numpy(g.copy()).cuda()
        norm = opt.step(gd).item()
        assert abs(norm - rnorm) <= 1e-5 * rnorm
        # f32 norms summed in a different order -> clip coefficients agree to
        # ~1e-6 relative; element tolerances are relative to each array's scale
        def close(a, b, rel):
            np.testing.assert_allclose(a, b, rtol=rel, atol=rel * np.abs(b).max())
        close(gd.cpu().numpy(), rg, 1e-5)
        close(opt.m.cpu().numpy(), rm, 1e-5)
        close(opt.v.cpu().numpy(), rv, 1e-5)
        close(opt.p.cpu().numpy() - p, rp - p, 1e-4)   # the update itself
        np.testing.assert_allclose(opt.p.cpu().numpy(), rp, rtol=1e-6, atol=1e-7)


def test_tanh_backward_fused_bias_grad():
    from drone_rl_amd import ppo_kernels as K
    for m, n in ((65536, 256), (1000, 64), (777, 12)):
        h = torch.tanh(torch.randn(m, n, device="cuda"))
        g = torch.randn(m, n, device="cuda")
        gz = torch.empty_like(h)
        gb = torch.empty(n, device="cuda")
        ws = torch.empty(K.tanh_backward_workspace_bytes(m, n) // 4 + 1, device="cuda")
        K.tanh_backward(g, h, gz, gb, ws)
        ref = g * (1 - h * h)
        assert torch.allclose(gz, ref, rtol=0, atol=0)
        assert torch.allclose(gb, ref.sum(0), rtol=1e-4, atol=1e-3)


def test_fused_train_step_matches_autograd():
    """The hand-written backward (fused tanh/bias kernel, split-K weight
    gradients) equals torch autograd through the same MLP."""
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep
    torch.manual_seed(0)
    pol = ActorCritic(15, 4, (256, 256), device="cuda", seed=3)
    m = 65536
    obs = torch.randn(m, 15, device="cuda")
    g_mean = torch.randn(m, 4, device="cuda") * 1e-3
    g_v = torch.randn(m, device="cuda") * 1e-3
    g_ls = torch.randn(4, device="cuda")
    fs = FusedTrainStep(pol, m)
    mean, value, cache = fs.forward(obs)
    grad = fs.backward(obs, cache, g_mean, g_v, g_ls).clone()
    pol.flat.grad = None
    mean2, value2 = pol(obs)
    assert torch.allclose(mean, mean2, atol=1e-5) and torch.allclose(value, value2, atol=1e-5)
    torch.autograd.backward([mean2, value2], [g_mean, g_v])
    ref = pol.flat.grad.clone()
    a, b, _ = pol.offsets["log_std"]
    ref[a:b] = g_ls
    for name, _, _ in pol.layout:
        lo, hi, _ = pol.offsets[name]
        scale = ref[lo:hi].abs().max().item() + 1e-12
        assert (grad[lo:hi] - ref[lo:hi]).abs().max().item() <= 1e-4 * scale, name


@pytest.mark.parametrize("k,n", [(15, 256), (12, 64), (18, 128)])
def test_linear_tanh_matches_torch(k, n):
    from drone_rl_amd import ppo_kernels as K
    m = 5001
    x = torch.randn(m, k, device="cuda")
    w = torch.randn(n, k, device="cuda") * 0.4
    b = torch.randn(n, device="cuda") * 0.1
    h = torch.empty(m, n, device="cuda")
    K.linear_tanh(x, w, b, h)
    ref = torch.tanh(torch.addmm(b, x, w.t()))
    assert (h - ref).abs().max().item() <= 2e-6


def test_policy_heads_match_torch():
    from drone_rl_amd import ppo_kernels as K
    m, hd = 3001, 256
    hp = torch.tanh(torch.randn(m, hd, device="cuda"))
    hv = torch.tanh(torch.randn(m, hd, device="cuda"))
    wa, ba = torch.randn(4, hd, device="cuda") * 0.1, torch.randn(4, device="cuda")
    wv, bv = torch.randn(1, hd, device="cuda") * 0.1, torch.randn(1, device="cuda")
    mean = torch.empty(m, 4, device="cuda")
    value = torch.empty(m, device="cuda")
    K.policy_heads(hp, hv, wa, ba, wv, bv, mean, value)
    assert (mean - torch.addmm(ba, hp, wa.t())).abs().max().item() <= 1e-5
    assert (value - torch.addmm(bv, hv, wv.t()).squeeze(1)).abs().max().item() <= 1e-5
    # pre-activation inputs: the layer's tanh is applied on load
    z = torch.randn(m, hd, device="cuda") * 2
    K.policy_heads(z, z, wa, ba, wv, bv, mean, value, preact=True)
    t = torch.tanh(z)
    assert (mean - torch.addmm(ba, t, wa.t())).abs().max().item() <= 1e-5
    assert (value - torch.addmm(bv, t, wv.t()).squeeze(1)).abs().max().item() <= 1e-5
    # top-layer biases added on load (the batched top GEMM leaves them out)
    zp, zv = torch.randn(hd, device="cuda"), torch.randn(hd, device="cuda")
    K.policy_heads(z, z, wa, ba, wv, bv, mean, value, preact=True, zb_pi=zp, zb_vf=zv)
    tp, tv = torch.tanh(z + zp), torch.tanh(z + zv)
    assert (mean - torch.addmm(ba, tp, wa.t())).abs().max().item() <= 1e-5
    assert (value - torch.addmm(bv, tv, wv.t()).squeeze(1)).abs().max().item() <= 1e-5


@pytest.mark.parametrize("arch,m", [((256, 256), 65536), ((64, 64), 64), ((64, 128), 1000)])
def test_fused_step_matches_unfused_path(arch, m):
    """FusedTrainStep.step (first-layer linear+tanh kernel, heads + loss +
    head backward kernel) == forward -> dr_ppo_loss -> hand backward, to f32
    summation-order noise; two runs are bitwise identical."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep
    torch.manual_seed(1)
    pol = ActorCritic(15, 4, arch, device="cuda", seed=4)
    with torch.no_grad():
        pol.flat.mul_(3.0)              # non-trivial heads / log_std
    obs = torch.randn(m, 15, device="cuda")
    fs = FusedTrainStep(pol, m)
    with torch.no_grad():
        mean, value, cache = fs.forward(obs)
        d = torch.distributions.Normal(mean, pol.log_std.exp())
        act = d.sample()
        aux = torch.stack([d.log_prob(act).sum(1) + 0.1 * torch.randn(m, device="cuda"),
                           torch.randn(m, device="cuda"), torch.randn(m, device="cuda")], 1)
    L = K.PPOLoss(m, "cuda", 0.2, 0.01, 0.5, True)
    g_mean, g_ls, g_v, st = L(mean, pol.log_std.detach(), value, act, aux=aux)
    ref = fs.backward(obs, cache, g_mean, g_v, g_ls).clone()
    st_ref = st.clone()
    head = K.HeadLossBackward(m, arch[-1], "cuda", 0.2, 0.01, 0.5, True)
    grad, st2 = fs.step(obs, act, aux, head)
    grad = grad.clone()
    for name, _, _ in pol.layout:
        lo, hi, _ = pol.offsets[name]
        scale = ref[lo:hi].abs().max().item() + 1e-12
        # + an absolute floor for sums that cancel (e.g. the value bias: 65k
        # terms of ~3e-5 summing to ~2e-5 in a different order)
        assert (grad[lo:hi] - ref[lo:hi]).abs().max().item() <= 2e-4 * scale + 1e-7, name
    assert torch.allclose(st2, st_ref, rtol=1e-4, atol=1e-6)
    grad2, _ = fs.step(obs, act, aux, head)
    assert torch.equal(grad, grad2)


@pytest.mark.parametrize("k,n,m", [(15, 256, 65536), (12, 64, 1001), (18, 128, 77)])
def test_first_layer_backward_matches_torch(k, n, m):
    from drone_rl_amd import ppo_kernels as K
    x = torch.randn(m, k, device="cuda")
    h = torch.tanh(torch.randn(m, n, device="cuda"))
    g = torch.randn(m, n, device="cuda")
    gw = torch.empty(n, k, device="cuda")
    gb = torch.empty(n, device="cuda")
    K.FirstLayerBackward(m, k, n, "cuda")(g, h, x, gw, gb)
    gz = (g.double() * (1 - h.double() ** 2))
    ref_w = gz.t() @ x.double()
    ref_b = gz.sum(0)
    tol = 1e-5 * (gz.abs().t() @ x.double().abs()).max().item()
    assert (gw.double() - ref_w).abs().max().item() <= tol
    assert (gb.double() - ref_b).abs().max().item() <= 1e-5 * gz.abs().sum(0).max().item()


def test_fused_step_rows_in_place_equals_gathered():
    """Reading the minibatch through the permutation (rows=) inside the
    kernels is bitwise the same as gathering it first."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep
    torch.manual_seed(2)
    pol = ActorCritic(15, 4, (256, 256), device="cuda", seed=5)
    total, m = 3 * 4096, 4096
    obs = torch.randn(total, 15, device="cuda")
    act = torch.rand(total, 4, device="cuda") * 7.3575
    aux = torch.randn(total, 3, device="cuda")
    rows = torch.randperm(total, device="cuda")[:m].to(torch.int32)
    fs = FusedTrainStep(pol, m)
    head = K.HeadLossBackward(m, 256, "cuda")
    g1, s1 = fs.step(obs, act, aux, head, rows=rows)
    g1, s1 = g1.clone(), s1.clone()
    r = rows.long()
    g2, s2 = fs.step(obs[r].contiguous(), act[r].contiguous(), aux[r].contiguous(), head)
    assert torch.equal(g1, g2) and torch.equal(s1, s2)


@pytest.mark.parametrize("k,n,m", [(15, 256, 65536), (18, 128, 1001), (12, 64, 77)])
def test_paired_first_layer_kernels_equal_single(k, n, m):
    """dr_linear_tanh2 / dr_first_layer_backward2 (both MLPs in one launch)
    are bitwise the single-net kernels, with and without rows=."""
    from drone_rl_amd import ppo_kernels as K
    g = torch.Generator(device="cuda").manual_seed(k * n + m)
    total = m + 13
    x = torch.randn(total, k, device="cuda", generator=g)
    rows = torch.randperm(total, device="cuda", generator=g)[:m].to(torch.int32)
    w = [torch.randn(n, k, device="cuda", generator=g) * 0.4 for _ in range(2)]
    b = [torch.randn(n, device="cuda", generator=g) * 0.1 for _ in range(2)]
    gh = [torch.randn(m, n, device="cuda", generator=g) for _ in range(2)]
    for r in (None, rows):
        xs = x[:m] if r is None else x
        h1 = [torch.empty(m, n, device="cuda") for _ in range(2)]
        for j in range(2):
            K.linear_tanh(xs, w[j], b[j], h1[j], r)
        h2 = [torch.empty(m, n, device="cuda") for _ in range(2)]
        K.linear_tanh2(xs, w[0], b[0], h2[0], w[1], b[1], h2[1], r)
        assert torch.equal(h1[0], h2[0]) and torch.equal(h1[1], h2[1])
        single = K.FirstLayerBackward(m, k, n, "cuda")
        ref = []
        for j in range(2):
            gw, gb = torch.empty(n, k, device="cuda"), torch.empty(n, device="cuda")
            single(gh[j], h1[j], xs, gw, gb, r)
            ref += [gw, gb]
        out = [torch.full((n, k), float("nan"), device="cuda"),
               torch.full((n,), float("nan"), device="cuda")] * 2
        out = [t.clone() for t in out]
        K.FirstLayerBackward2(m, k, n, "cuda")(xs, gh[0], h1[0], out[0], out[1],
                                               gh[1], h1[1], out[2], out[3], r)
        for a, c in zip(ref, out):
            assert torch.equal(a, c)


@pytest.mark.parametrize("m,d", [(65536, 15), (1000, 18), (300, 12)])
def test_gather_minibatch_equals_gathers_and_adv_pass(m, d):
    """dr_gather_minibatch == three dr_gather_rows, and the head step fed
    its advantage partials (normalize_advantage = 2) is bitwise the head
    step that computes them itself."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep
    g = torch.Generator(device="cuda").manual_seed(m + d)
    total = 2 * m + 5
    obs = torch.randn(total, d, device="cuda", generator=g)
    act = torch.rand(total, 4, device="cuda", generator=g) * 7.3575
    aux = torch.randn(total, 3, device="cuda", generator=g)
    idx = torch.randperm(total, device="cuda", generator=g)[:m].to(torch.int32)
    o, a, x = (torch.empty(m, w, device="cuda") for w in (d, 4, 3))
    head = K.HeadLossBackward(m, 256, "cuda", 0.2, 0.0, 0.5, True)
    K.gather_minibatch(idx, obs, act, aux, o, a, x, adv_part=head.adv_part)
    r = idx.long()
    assert torch.equal(o, obs[r]) and torch.equal(a, act[r]) and torch.equal(x, aux[r])
    pol = ActorCritic(d, 4, (256, 256), device="cuda", seed=6)
    fs = FusedTrainStep(pol, m)
    st_out = torch.empty(8, device="cuda")
    g1, s1 = fs.step(o, a, x, head, adv_ready=True, stats_out=st_out)
    assert s1.data_ptr() == st_out.data_ptr()
    g1, s1 = g1.clone(), s1.clone()
    g2, s2 = fs.step(o, a, x, head)          # the head's own advantage pass
    assert torch.equal(g1, g2) and torch.equal(s1, s2)


@pytest.mark.parametrize("m,d", [(1, 7), (1025, 5), (4099, 15), (70001, 12)])
def test_gather_minibatch_ragged_and_runtime_widths(m, d):
    """dr_gather_minibatch at ragged row counts (partial last block of every
    section) and at obs widths without a compiled-in constant (the runtime
    divisor path): the rows of obs / actions / aux exactly."""
    from drone_rl_amd import ppo_kernels as K
    g = torch.Generator(device="cuda").manual_seed(m * 31 + d)
    total = 3 * m + 2
    obs = torch.randn(total, d, device="cuda", generator=g)
    act = torch.randn(total, 4, device="cuda", generator=g)
    aux = torch.randn(total, 3, device="cuda", generator=g)
    idx = torch.randperm(total, device="cuda", generator=g)[:m].to(torch.int32)
    o, a, x = (torch.full((m, w), float("nan"), device="cuda") for w in (d, 4, 3))
    K.gather_minibatch(idx, obs, act, aux, o, a, x)
    r = idx.long()
    assert torch.equal(o, obs[r]) and torch.equal(a, act[r]) and torch.equal(x, aux[r])


@pytest.mark.parametrize("m,d", [(65536, 15), (1, 15), (1025, 12), (4099, 5), (70001, 18),
                                 (300, 24)])
def test_gather_records_is_gather_minibatch(m, d):
    """The one-line record path (round 6): dr_pack_rollout_records once, then
    dr_gather_records writes exactly dr_gather_minibatch's bytes -- obs,
    action and aux rows and the advantage (count, mean, M2) partials -- at
    full size, ragged row counts and other obs widths; the records hold
    each row's values at their documented offsets."""
    from drone_rl_amd import ppo_kernels as K
    g = torch.Generator(device="cuda").manual_seed(m * 7 + d)
    total = 2 * m + 3
    obs = torch.randn(total, d, device="cuda", generator=g)
    act = torch.rand(total, 4, device="cuda", generator=g) * 7.3575
    lp, adv, ret = (torch.randn(total, device="cuda", generator=g) for _ in range(3))
    aux = torch.stack([lp, adv, ret], dim=1)
    rec = torch.full((total, K.RECORD_FLOATS), float("nan"), device="cuda")
    K.pack_rollout_records(obs, act, lp, adv, ret, rec)
    ao = 4 * ((d + 3) // 4)
    assert torch.equal(rec[:, :d], obs) and torch.equal(rec[:, ao:ao + 4], act)
    assert torch.equal(rec[:, ao + 4:ao + 7], aux)
    assert (rec[:, d:ao] == 0).all() and (rec[:, ao + 7:] == 0).all()
    idx = torch.randperm(total, device="cuda", generator=g)[:m].to(torch.int32)
    nb = (m + 255) // 256
    outs = []
    for use_rec in (False, True):
        o, a, x = (torch.full((m, w), float("nan"), device="cuda") for w in (d, 4, 3))
        part = torch.full((3 * nb,), float("nan"), device="cuda")
        if use_rec:
            K.gather_records(idx, rec, d, o, a, x, adv_part=part)
        else:
            K.gather_minibatch(idx, obs, act, aux, o, a, x, adv_part=part)
        outs.append((o, a, x, part))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    r = idx.long()
    assert torch.equal(outs[1][0], obs[r]) and torch.equal(outs[1][2], aux[r])


@pytest.mark.parametrize("arch,m", [((256, 256), 65536), ((64, 64), 1000), ((64, 128), 4096)])
def test_deferred_finish_equals_separate_finishes(arch, m):
    """FusedTrainStep.step(defer_finish=True) + ClipAdam.step_finish (the
    head / first-layer / split-K reductions and the norm in one launch) ==
    the separate finish launches + ClipAdam.step: stats bitwise, clipped
    gradient and updated parameters to f32 summation-order noise; reruns
    bitwise."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep
    g = torch.Generator(device="cuda").manual_seed(m)
    obs = torch.randn(m, 15, device="cuda", generator=g)
    act = torch.rand(m, 4, device="cuda", generator=g) * 7.3575
    aux = torch.randn(m, 3, device="cuda", generator=g)

    def run(defer):
        pol = ActorCritic(15, 4, arch, device="cuda", seed=9)
        with torch.no_grad():
            pol.flat.mul_(2.0)
        fs = FusedTrainStep(pol, m)
        head = K.HeadLossBackward(m, arch[-1], "cuda", 0.2, 0.01, 0.5, True)
        opt = K.ClipAdam(pol.flat.data, 3e-4, eps=1e-5, max_grad_norm=0.5)
        st = torch.full((8,), float("nan"), device="cuda")
        outs = []
        for _ in range(2):                     # two optimizer steps
            grad, s = fs.step(obs, act, aux, head, stats_out=st, defer_finish=defer)
            if defer:
                norm = opt.step_finish(grad, fs.finish)
            else:
                norm = opt.step(grad)
            outs.append((grad.clone(), s.clone(), norm.clone()))
        torch.cuda.synchronize()
        return outs, pol.flat.detach().clone()

    (a, pa), (b, pb), (c, pc) = run(False), run(True), run(True)
    for (ga, sa, na), (gb, sb, nb) in zip(a, b):
        assert torch.equal(sa, sb)
        assert abs(na.item() - nb.item()) <= 1e-5 * na.item()
        scale = ga.abs().max().item()
        assert (ga - gb).abs().max().item() <= 1e-5 * scale
    assert (pa - pb).abs().max().item() <= 1e-5
    assert torch.equal(pb, pc) and all(torch.equal(x[0], y[0]) for x, y in zip(b, c))


# ------------------------------------------------- dr_ppo_loss rows against f64
U = 2.0 ** -24          # fp32 unit roundoff; one ulp is at most 2 U relative
LOG_SQRT_2PI = 0.5 * np.log(2 * np.pi)


def _adv_stats_bound(adv32):
    """Error bounds of dr_ppo_loss's advantage statistics (adv_stats_kernel's
    per-block (count, mean, M2), merged in double by Chan's formula), from
    the f32 inputs alone: (|d mean|, relative |d std|).

    Block b (<= 256 rows): its sum is a tree of depth 9 (6 wave shuffles, 3
    adds across the 4 waves), |d sum| <= gamma_9 sum|a|, and the division by
    the count is one more operation (<= 1 ulp = 2 U), so the block mean is off
    by |eps_b| <= e_b = (gamma_9 + 2 U) mean_b|a|.  The merged mean is the
    count-weighted mean of the block means (double: exact here), off by at
    most ebar = sum_b n_b e_b / N, plus its rounding to f32.

    M2.  The block's M2 is taken about its COMPUTED mean: sum (a_i - m_b -
    eps_b)^2 = M2_b + n_b eps_b^2 exactly (the first-order term vanishes,
    sum (a_i - m_b) = 0), and Chan's merge adds n_b (m_b + eps_b - mu -
    epsbar)^2.  A block-mean error common to all blocks cancels in eps_b -
    epsbar, so it enters at second order only; the blocks' differing errors
    enter as 2 n_b (m_b - mu)(eps_b - epsbar), first order but scaled by the
    block means' spread (sigma / 16 for 256-row blocks).  Hence
      |d M2| <= sum_b n_b [2 |m_b - mu| (e_b + ebar) + (e_b + ebar)^2 + e_b^2]
                + gamma_13 M2
    (gamma_13: each fl(a_i - m_b)^2 carries 3 roundings, the tree 9, the f32
    partial 1).  std = sqrtf(M2 / (N - 1)): the f32 rounding of M2, the
    division and the square root (<= 1 ulp each) add 0.5 (U + 2 U) + 2 U."""
    a = np.asarray(adv32, np.float64)
    N = len(a)
    mu = a.mean()
    M2 = ((a - mu) ** 2).sum()
    g9, g13 = 9 * U / (1 - 9 * U), 13 * U / (1 - 13 * U)
    nb, mb, eb = [], [], []
    for s in range(0, N, 256):
        blk = a[s:s + 256]
        nb.append(len(blk))
        mb.append(blk.mean())
        eb.append((g9 + 2 * U) * np.abs(blk).mean())
    nb, mb, eb = map(np.array, (nb, mb, eb))
    ebar = (nb * eb).sum() / N
    d_mu = ebar + U * abs(mu)
    d_m2 = (nb * (2 * np.abs(mb - mu) * (eb + ebar) + (eb + ebar) ** 2 + eb ** 2)).sum() + g13 * M2
    return d_mu, 0.5 * (d_m2 / M2 + 3 * U) + 2 * U


def _loss_rows_f64(mean, log_std, values, act, old_logp, adv, ret, clip, ent, vf, normalize):
    """torch f64 autograd of SB3's minibatch loss w.r.t. (mean, log_std,
    values), and the per-row quantities the bounds are built from."""
    t = lambda x: torch.as_tensor(x).double()      # noqa: E731
    mu = t(mean).clone().requires_grad_(True)
    ls = t(log_std).clone().requires_grad_(True)
    v = t(values).clone().requires_grad_(True)
    a, olp, A_raw, R = t(act), t(old_logp), t(adv), t(ret)
    m = mu.shape[0]
    z = (a - mu) / ls.exp()
    lp = (-0.5 * z ** 2 - ls - LOG_SQRT_2PI).sum(1)
    A = (A_raw - A_raw.mean()) / (A_raw.std() + 1e-8) if (normalize and m > 1) else A_raw
    logr = lp - olp
    r = logr.exp()
    surr = torch.min(A * r, A * r.clamp(1 - clip, 1 + clip))
    H = (0.5 + LOG_SQRT_2PI + ls).sum()
    verr = (R - v) ** 2
    loss = -surr.mean() - ent * H + vf * verr.mean()
    loss.backward()
    with torch.no_grad():
        kl = (r - 1) - logr
        return dict(g_mean=mu.grad.numpy(), g_ls=ls.grad.numpy(), g_v=v.grad.numpy(),
                    z=z.numpy(), q=(0.5 * z ** 2).numpy(), A=A.numpy(), A_raw=A_raw.numpy(),
                    r=r.numpy(), logr=logr.numpy(), surr=surr.numpy(), verr=verr.numpy(),
                    kl=kl.numpy(), H=H.item(), sd=ls.exp().detach().numpy(),
                    ls=ls.detach().numpy(),
                    clip_count=int(((r - 1).abs() > clip).sum()),
                    stats=[loss.item(), -surr.mean().item(), verr.mean().item(), -H.item(),
                           ((r - 1).abs() > clip).double().mean().item(), kl.mean().item()])


def _loss_row_bounds(ref, m, clip, ent, vf, normalize):
    """fp32 error bounds of dr_ppo_loss's outputs from ppo_row's operation
    chain (U = 2^-24; a correctly rounded operation costs U relative, a
    device-library function -- expf, logf, sqrtf, the reciprocals -- <= 1 ulp
    = 2 U; -ffp-contract=off: every product and sum is rounded separately):

      sd = expf(ls) 2U; var = sd sd 5U; inv_var, inv_2var 7U
      d = a - mu U; zz = d inv_var 9U; q = (d d) inv_2var 11U; y = (d d) inv_var 11U
      logsd = logf(sd): 2U |ls| + 2U absolute (the 2U of sd moves the log by 2U)
      lp: 4 x (q - logsd - c): E_lp = 11 sum q + 2 sum(|ls| + 1) + 4 c  (terms)
                                     + 12 S, S = sum(q + |ls| + c)       (12 adds)
      logr = lp - old: d_logr = U (E_lp + |logr|) absolute
      r = expf(logr): rho_r = d_logr + 2U relative
      A = (A - mean) inv_astd: d_A = (U |A - mean| + d_mean) / std
                                     + |A| (rho_std + 4U)   (_adv_stats_bound;
                                     inv_astd = 1 / (std + 1e-8): 3U, product U)
      dr = -(..A..) inv_m: the branch weights are exact (0, 1/2, 1; a tie is
           A/2 + A/2), inv_m 2U, product U;  dlp = dr r: + rho_r + U
      g_mean_j = dlp zz_j: |g| (rho_r + 14U) + (r |zz_j| / m) d_A
      g_value = vf (2 (v - R)) inv_m: 6U relative
      g_log_std_j = sum_i t_i - ent, t = dlp (y - 1):
           sum_i [|t| (rho_r + 5U) + (r |y - 1| / m) d_A + |dlp| (11U y + U |y - 1|)]
           + gamma_m sum|t| (a sum of m terms in any grouping) + U |result|
      policy_loss = sum(-min(A r, A rc)) inv_m, rc = r or 1 -+ clip (<= 2U):
           mean[|l| (rho_r + 3U) + r d_A] + (gamma_m + 3U) mean|l|
      value_loss = sum((R - v)^2) inv_m: (gamma_m + 6U) relative (positive terms)
      approx_kl = sum((r - 1) - logr) inv_m:
           mean[r rho_r + U |r - 1| + d_logr + U |t|] + (gamma_m + 3U) mean|t|
      entropy_loss = -sum_j(0.5 + c + ls_j): 12 adds of partial sums <= E_H =
           sum(0.5 + c + |ls_j|): 12U E_H + 4U c
      loss = pl + ent el + vf vl: the three bounds + 4U (|pl| + |ent el| + |vf vl|)
    """
    gm = lambda n: n * U / (1 - n * U)             # noqa: E731
    q, ls, r, A = ref["q"], ref["ls"], ref["r"], ref["A"]
    S = (q + np.abs(ls) + LOG_SQRT_2PI).sum(1)
    E_lp = 11 * q.sum(1) + 2 * (np.abs(ls) + 1).sum() + 4 * LOG_SQRT_2PI + 12 * S
    d_logr = U * (E_lp + np.abs(ref["logr"]))
    rho_r = d_logr + 2 * U
    if normalize and m > 1:
        d_mu, rho_sd = _adv_stats_bound(ref["A_raw"].astype(np.float32))
        std = ref["A_raw"].std(ddof=1)
        d_A = (U * np.abs(ref["A_raw"] - ref["A_raw"].mean()) + d_mu) / std + \
            np.abs(A) * (rho_sd + 4 * U)
    else:
        d_A = np.zeros(m)
    zz = np.abs(ref["z"]) / ref["sd"]
    b = {}
    b["g_mean"] = np.abs(ref["g_mean"]) * (rho_r + 14 * U)[:, None] + \
        (r[:, None] * zz / m) * d_A[:, None]
    b["g_v"] = 6 * U * np.abs(ref["g_v"])
    y = 2 * q
    # |dlp| = |A| r / m on the rows whose unclipped branch carries the gradient;
    # bounding every row by it only loosens the bound where the gradient is 0
    dlp = (np.abs(A) * r / m)[:, None]
    t = dlp * np.abs(y - 1)
    b["g_ls"] = (t * (rho_r + 5 * U)[:, None] + (r[:, None] * np.abs(y - 1) / m) * d_A[:, None] +
                 dlp * (11 * U * y + U * np.abs(y - 1))).sum(0) + gm(m) * t.sum(0) + \
        U * np.abs(ref["g_ls"])
    l = np.abs(ref["surr"])
    pl = (l * (rho_r + 3 * U) + np.maximum(r, 1 + clip) * d_A).mean() + (gm(m) + 3 * U) * l.mean()
    vl = (gm(m) + 6 * U) * ref["verr"].mean()
    kl = (r * rho_r + U * np.abs(r - 1) + d_logr + U * np.abs(ref["kl"])).mean() + \
        (gm(m) + 3 * U) * np.abs(ref["kl"]).mean()
    E_H = (0.5 + LOG_SQRT_2PI + np.abs(ls)).sum()
    el = 12 * U * E_H + 4 * U * LOG_SQRT_2PI
    st = ref["stats"]
    tot = pl + abs(ent) * el + vf * vl + 4 * U * (abs(st[1]) + abs(ent * st[3]) + abs(vf * st[2]))
    b["stats"] = [tot, pl, vl, el, 0.0, kl]
    return b


def _loss_inputs(m):
    """PPOLoss inputs on the in-distribution fixture: the f64 forward's mean
    and values rounded to f32."""
    from ppo_f64 import midtraining_minibatch
    mb = midtraining_minibatch(15, (64, 64), m, seed=3)
    return dict(mean=mb["mean64"].float().numpy(), log_std=mb["sd"]["log_std"].numpy(),
                values=mb["value64"].float().numpy(), act=mb["act"].numpy(),
                old_logp=mb["old_logp"].numpy(), adv=mb["adv"].numpy(), ret=mb["ret"].numpy())


def _run_loss(x, m, clip, ent, vf, normalize):
    from drone_rl_amd import ppo_kernels as K
    cu = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()  # noqa: E731
    L = K.PPOLoss(m, "cuda", clip, ent, vf, normalize)
    gm, gls, gv, st = L(cu(x["mean"]), cu(x["log_std"]), cu(x["values"]), cu(x["act"]),
                        cu(x["old_logp"]), cu(x["adv"]), cu(x["ret"]))
    torch.cuda.synchronize()
    return (gm.cpu().numpy().astype(np.float64), gls.cpu().numpy().astype(np.float64),
            gv.cpu().numpy().astype(np.float64), st.cpu().numpy().astype(np.float64))


@pytest.mark.parametrize("normalize", [True, False])
@pytest.mark.parametrize("m", [1, 255, 257, 4099])
def test_ppo_loss_rows_match_f64_entrywise(m, normalize):
    """dr_ppo_loss on a minibatch that engages the clip, at one row, one block
    less one row, one block plus one row and 17 blocks: grad_mean and
    grad_values entrywise, grad_log_std and the stats, against torch f64
    autograd of the same expression, within the bounds of ppo_row's operation
    chain (_loss_row_bounds, _adv_stats_bound: the derivation).  The
    clip count is exact.  At m = 1 normalize_advantage changes nothing (SB3
    normalises only when len(advantages) > 1).
    Measured on an MI355X, worst error / bound over the eight cases:
    grad_mean 0.128, grad_values 0.467, grad_log_std 0.075, loss 0.056,
    policy_loss 0.064, value_loss 0.179, entropy_loss 0.013, approx_kl 0.001
    (the sums' worst cases at m = 1, where the bound has no slack from
    rounding errors cancelling across rows)."""
    clip, ent, vf = 0.2, 0.01, 0.5
    x = _loss_inputs(m)
    ref = _loss_rows_f64(x["mean"], x["log_std"], x["values"], x["act"], x["old_logp"],
                         x["adv"], x["ret"], clip, ent, vf, normalize)
    b = _loss_row_bounds(ref, m, clip, ent, vf, normalize)
    gm, gls, gv, st = _run_loss(x, m, clip, ent, vf, normalize)
    tiny = 1e-37                       # below the smallest normal f32: underflow
    ratios = {
        "grad_mean": (np.abs(gm - ref["g_mean"]) / (b["g_mean"] + tiny)).max(),
        "grad_values": (np.abs(gv - ref["g_v"]) / (b["g_v"] + tiny)).max(),
        "grad_log_std": (np.abs(gls - ref["g_ls"]) / (b["g_ls"] + tiny)).max(),
    }
    for i, name in ((0, "loss"), (1, "policy_loss"), (2, "value_loss"), (3, "entropy_loss"),
                    (5, "approx_kl")):
        ratios[name] = abs(st[i] - ref["stats"][i]) / (b["stats"][i] + tiny)
    print(f"m {m} normalize {normalize}: " +
          ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
          f"; clip count {round(st[4] * m)} / {ref['clip_count']}")
    for k, v in ratios.items():
        assert v <= 1.0, f"{k}: error {v:.3f} x its fp32 bound"
    assert round(st[4] * m) == ref["clip_count"]
    assert abs(st[4] - ref["clip_count"] / m) <= 3 * U * ref["clip_count"] / m
    if m > 1:
        assert 0.2 * m <= ref["clip_count"] <= 0.7 * m
    if not normalize:
        assert st[6] == 0.0 and st[7] == 1.0
    if m == 1 and normalize:
        raw = _run_loss(x, m, clip, ent, vf, False)
        for u, v in zip((gm, gls, gv, st), raw):
            assert np.array_equal(u, v)


@pytest.mark.parametrize("offset", [0.0, 100.0, 1e4])
@pytest.mark.parametrize("m", [257, 4099])
def test_ppo_loss_advantage_statistics_match_f64(m, offset):
    """stats[6] / stats[7] (the minibatch advantage mean and unbiased std the
    normalisation uses) against the f64 mean and std of the same f32 inputs,
    unit spread around 0, 100 and 10,000 -- where a one-pass sum of squares
    would lose the variance -- within _adv_stats_bound (the derivation).
    Measured on an MI355X, worst error / bound (mean, std):
    0.105, 0.059 (bounds at m = 4099: |d mean| 5.2e-7 / 7.2e-5 / 7.2e-3 and
    relative |d std| 6.5e-7 / 8.0e-6 / 8.5e-4 at offsets 0 / 100 / 10,000)."""
    x = _loss_inputs(m)
    g = torch.Generator().manual_seed(m)
    x["adv"] = (offset + torch.randn(m, generator=g, dtype=torch.float64)).float().numpy()
    _, _, _, st = _run_loss(x, m, 0.2, 0.0, 0.5, True)
    a = x["adv"].astype(np.float64)
    d_mu, rho_sd = _adv_stats_bound(x["adv"])
    r_mu = abs(st[6] - a.mean()) / d_mu
    r_sd = abs(st[7] - a.std(ddof=1)) / (rho_sd * a.std(ddof=1))
    print(f"m {m} offset {offset:g}: mean error / bound {r_mu:.3f} (bound {d_mu:.3g}), "
          f"std error / bound {r_sd:.3f} (relative bound {rho_sd:.3g})")
    assert r_mu <= 1.0 and r_sd <= 1.0


# --------------------------------------------- policy_sample against the oracle
SAMPLE_SEED, SAMPLE_COUNTER = 0x1234567890, (7 << 32) + 5
LO, HI = 0.0, 7.3575


def _sample(n, mean, log_std, seed=SAMPLE_SEED, counter=SAMPLE_COUNTER, want=(1, 1, 1),
            dev=None):
    from drone_rl_amd import ppo_kernels as K
    raw = torch.full((n, 4), float("nan"), device="cuda") if want[0] else None
    clip = torch.full((n, 4), float("nan"), device="cuda") if want[1] else None
    logp = torch.full((n,), float("nan"), device="cuda") if want[2] else None
    if dev is None:
        K.policy_sample(mean, log_std, seed, counter, LO, HI, raw, clip, logp)
    else:
        base = torch.tensor([dev[0]], dtype=torch.int64, device="cuda")
        K.policy_sample_dev(mean, log_std, seed, base, dev[1], LO, HI, raw, clip, logp)
    torch.cuda.synchronize()
    return raw, clip, logp


@pytest.mark.parametrize("log_std", [[0.0, -0.5, 0.3, -1.0], [-5.0, -1.0, 0.0, 2.0]])
@pytest.mark.parametrize("n", [1, 255, 257, 4099])
def test_policy_sample_matches_philox_oracle(n, log_std):
    """dr_policy_sample per element against oracle/cref.policy_noise_np, with
    both high words of the seed and of the counter live.

    Noise.  z = r cos(theta) (or sin), r = sqrtf(-2 logf(u1)); u1, u2 and
    theta are formed exactly as the oracle forms them.  With the device
    library's documented bounds (logf, sqrtf, sincosf, expf: <= 1 ulp =
    2^-23 relative each; the HIP math API's table -- not available on the
    build machine, so taken as stated there): logf's 2^-23 is halved by the
    square root, sqrtf adds 2^-23, cos / sin 2^-23, the product 2^-24:
    |dz| <= 3 * 2^-23 r (|cos|, |sin| <= 1).  The test reads z back as
    (raw - mean) / exp(log_std) in f64: raw = fl(mean + fl(sd z)) adds 2^-24
    |z| + 2^-24 |raw| / sd, and sd = expf(log_std) (<= 1 ulp) 2^-23 |z|; the
    f64 subtraction and division add 2^-52 (|raw| + |mean|) / sd.
    Log-prob, from the kernel's own raw, against f64: four terms -(d d)
    inv_2var - logf(sd) - c; q = (d d) inv_2var carries 11 roundings (d 1, d d
    2 + 1, inv_2var 2 x 2 + 1 + 2, product 1), logf(sd) 2^-23 (|ls| + 1), the
    constant 2^-24 c, and the 12 additions 2^-24 S each, S = sum(q + |ls| + c):
    |d logp| <= 2^-24 (11 sum q + 2 sum(|ls| + 1) + 4 c + 12 S).
    Clipped actions: clamp(raw, lo, hi) exactly.
    Measured on an MI355X, worst error / bound (noise, log-prob):
    0.970, 0.126.  Against 3 * 2^-23 r alone the read-back noise is off by up
    to 43 x (log_std >= -1) and 1,490 x (log_std = -5): that is the rounding
    of mean + sd z divided by sd, which the bound carries, not the draw."""
    g = torch.Generator().manual_seed(n)
    mean = (2.0 + 2.0 * torch.randn(n, 4, generator=g)).cuda()
    ls = torch.tensor(log_std, device="cuda")
    raw, clip, logp = _sample(n, mean, ls)
    z_ref, rad = cref.policy_noise_np(n, SAMPLE_SEED, SAMPLE_COUNTER)
    mu = mean.cpu().numpy().astype(np.float64)
    a = raw.cpu().numpy().astype(np.float64)
    lsd = np.array(log_std, np.float32).astype(np.float64)
    sd = np.exp(lsd)
    z = (a - mu) / sd
    tol = 3 * 2.0 ** -23 * rad + (2.0 ** -23 + 2.0 ** -24) * np.abs(z_ref) + \
        2.0 ** -24 * np.abs(a) / sd + 2.0 ** -52 * (np.abs(a) + np.abs(mu)) / sd
    r_z = (np.abs(z - z_ref) / tol).max()
    # the share of the bound that is the draw's own (c 2^-23 r), for the record
    r_draw = (np.abs(z - z_ref) / (3 * 2.0 ** -23 * rad + 1e-300)).max()
    q = 0.5 * z ** 2
    lp_ref = (-q - lsd - LOG_SQRT_2PI).sum(1)
    S = (q + np.abs(lsd) + LOG_SQRT_2PI).sum(1)
    lp_tol = U * (11 * q.sum(1) + 2 * (np.abs(lsd) + 1).sum() + 4 * LOG_SQRT_2PI + 12 * S)
    r_lp = (np.abs(logp.cpu().numpy().astype(np.float64) - lp_ref) / lp_tol).max()
    print(f"n {n} log_std {log_std}: noise error / bound {r_z:.3f} "
          f"(against 3 * 2^-23 r alone: {r_draw:.3f}), log-prob error / bound {r_lp:.3f}")
    assert r_z <= 1.0 and r_lp <= 1.0
    assert torch.equal(clip, raw.clamp(LO, HI))
    if n == 4099:                      # both ends of the clamp are engaged
        assert (raw < LO).any() and (raw > HI).any()


def test_policy_sample_device_counter_optional_outputs_and_streams():
    """dr_policy_sample_dev reads counter_base + counter_offset on the device:
    bitwise dr_policy_sample at the sum, with a carry from the low word into
    the high one.  Any subset of the three outputs may be null and the others
    keep their bytes.  The high seed word, the high counter word and the row
    index each select a different stream."""
    n = 4099
    g = torch.Generator().manual_seed(7)
    mean = torch.randn(n, 4, generator=g).cuda()
    ls = torch.tensor([0.0, -0.5, 0.3, -1.0], device="cuda")
    full = _sample(n, mean, ls)
    # device counter, no carry and a carry out of the low word
    for c0, c1 in (((7 << 32), 5), ((6 << 32) + 0xfffffffe, 7), (5, (7 << 32))):
        assert c0 + c1 == SAMPLE_COUNTER
        got = _sample(n, mean, ls, dev=(c0, c1))
        for u, v in zip(full, got):
            assert torch.equal(u, v), (c0, c1)
    # optional outputs
    for want in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (0, 0, 0)):
        for dev in (None, ((6 << 32) + 0xfffffffe, 7)):
            got = _sample(n, mean, ls, want=want, dev=dev)
            for w, u, v in zip(want, full, got):
                assert (v is None) if not w else torch.equal(u, v), (want, dev)
    # stream separation: only the high seed word / only the high counter word
    raw = full[0]
    for seed, counter in ((SAMPLE_SEED ^ (1 << 36), SAMPLE_COUNTER),
                          (SAMPLE_SEED, SAMPLE_COUNTER ^ (1 << 35)),
                          (SAMPLE_SEED ^ 1, SAMPLE_COUNTER), (SAMPLE_SEED, SAMPLE_COUNTER ^ 1)):
        other = _sample(n, mean, ls, seed=seed, counter=counter, want=(1, 0, 0))[0]
        assert (other != raw).float().mean().item() > 0.99, (hex(seed), hex(counter))
    # only i: rows with the same mean draw different noise, and the four
    # dimensions of a row are four different draws
    same = _sample(n, torch.zeros(n, 4, device="cuda"), torch.zeros(4, device="cuda"),
                   want=(1, 0, 0))[0].cpu().numpy()
    assert len(np.unique(same, axis=0)) == n
    assert len(np.unique(same.ravel())) > 0.999 * 4 * n
    c = np.corrcoef(same.T)
    assert np.abs(c - np.eye(4)).max() < 5 / np.sqrt(n)


# ------------------------------------- small shapes and loops no test had reached
@pytest.mark.parametrize("T,N", [(1, 1), (1, 257), (5, 255), (33, 256), (7, 1000)])
def test_gae_bitexact_small_shapes_and_edges(T, N):
    """dr_gae == the C oracle bit for bit at one env, one step, ragged and
    whole blocks; episode_starts all zero, all one and random; last_dones
    random and all one; the default (gamma, lambda), (1, 1) and lambda = 0."""
    from drone_rl_amd import ppo_kernels as K
    rng = np.random.default_rng(T * 1000 + N)
    r = rng.normal(size=(T, N)).astype(np.float32)
    v = rng.normal(size=(T, N)).astype(np.float32)
    lv = rng.normal(size=N).astype(np.float32)
    cu = lambda x: torch.from_numpy(x).cuda()  # noqa: E731
    starts = {"zero": np.zeros((T, N), np.uint8), "one": np.ones((T, N), np.uint8),
              "random": (rng.random((T, N)) < 0.3).astype(np.uint8)}
    dones = {"random": (rng.random(N) < 0.3).astype(np.uint8), "one": np.ones(N, np.uint8)}
    for sname, st in starts.items():
        for dname, ld in dones.items():
            for gamma, lam in ((0.99, 0.95), (1.0, 1.0), (0.9, 0.0)):
                adv, ret = K.gae(cu(r), cu(v), cu(st), cu(lv), cu(ld), gamma, lam)
                ra, rr = cref.gae(r, v, st, lv, ld, gamma, lam)
                what = f"starts {sname}, last_dones {dname}, gamma {gamma}, lambda {lam}"
                np.testing.assert_array_equal(adv.cpu().numpy(), ra, err_msg=what)
                np.testing.assert_array_equal(ret.cpu().numpy(), rr, err_msg=what)


def _clip_adam_f64(p, g, m, v, step, lr=3e-4, b1=0.9, b2=0.999, eps=1e-5, max_norm=0.5):
    """clip_grad_norm_ + torch.optim.Adam (oracle/ppo_ref.clip_adam_torch's
    math) restated in f64: (params, exp_avg, exp_avg_sq, clipped grad, norm)."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    norm = np.sqrt((g * g).sum())
    c = min(1.0, max_norm / (norm + 1e-6))
    gc = g * c
    m1 = m + (1 - b1) * (gc - m)
    v1 = b2 * v + (1 - b2) * gc * gc
    bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
    p1 = p - (lr / bc1) * (m1 / (np.sqrt(v1) / np.sqrt(bc2) + eps))
    return p1, m1, v1, gc, norm


def _close_to_f64(opt, gd, p0, ref):
    """test_clip_adam_vs_torch's element tolerances.  They cover the fp32
    rounding of the ten or so elementwise operations of clip + Adam (each
    2^-24 relative: 1e-5 leaves a factor ten) and the norm's reduction order
    in the clip factor; the floor relative to each array's largest entry
    covers entries that cancel (exp_avg + w (g - exp_avg) near zero).  The
    update is read back as p_new - p_old, and p_new = fl(p_old - step) is
    itself rounded to f32: 2^-24 |p_new| more, which at 141,065 elements hides
    below the floor (some update is always large) and at a few hundred
    elements does not."""
    rp, rm, rv, rg, rnorm = ref
    norm = opt.grad_norm.item()
    assert abs(norm - rnorm) <= 1e-5 * rnorm

    def close(a, b, rel):
        np.testing.assert_allclose(a, b, rtol=rel, atol=rel * np.abs(b).max())
    close(gd.cpu().numpy(), rg, 1e-5)
    close(opt.m.cpu().numpy(), rm, 1e-5)
    close(opt.v.cpu().numpy(), rv, 1e-5)
    upd, rupd = opt.p.cpu().numpy().astype(np.float64) - p0, rp - p0
    assert (np.abs(upd - rupd) <= 1e-4 * np.abs(rupd) + 1e-4 * np.abs(rupd).max() +
            2.0 ** -24 * np.abs(rp)).all()
    np.testing.assert_allclose(opt.p.cpu().numpy(), rp, rtol=1e-6, atol=1e-7)


def _adam_state(n, gscale, seed):
    rng = np.random.default_rng(seed)
    p = rng.normal(size=n).astype(np.float32)
    g = (rng.normal(size=n) * gscale / np.sqrt(n)).astype(np.float32)
    m = (rng.normal(size=n) * 1e-3).astype(np.float32)
    v = (rng.random(n) * 1e-6).astype(np.float32)
    return p, g, m, v


def _adam_opt(p, m, v, step):
    from drone_rl_amd import ppo_kernels as K
    opt = K.ClipAdam(torch.from_numpy(p.copy()).cuda())
    opt.m.copy_(torch.from_numpy(m))
    opt.v.copy_(torch.from_numpy(v))
    opt.t = step - 1
    return opt


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 257])
def test_clip_adam_matches_f64_at_small_sizes_and_in_the_grid_stride_loops(n):
    """dr_clip_adam against the f64 restatement at one element, a ragged
    block, a block plus one, and 2048 x 256 + 257 elements -- above the
    2048-block cap of the launch, so sumsq_kernel's and clip_adam_kernel's
    grid-stride loops run a second trip (for 257 elements only); clipped and
    unclipped gradients; an all-zero gradient (norm 0, nothing NaN, Adam's
    update from the old moments)."""
    for gscale, step in ((10.0, 1), (1e-4, 7), (0.0, 3)):
        p, g, m, v = _adam_state(n, gscale, n + step)
        opt = _adam_opt(p, m, v, step)
        gd = torch.from_numpy(g.copy()).cuda()
        opt.step(gd)
        torch.cuda.synchronize()
        if gscale == 0.0:
            assert opt.grad_norm.item() == 0.0
            assert torch.equal(gd, torch.zeros_like(gd))
            for t in (opt.p, opt.m, opt.v):
                assert torch.isfinite(t).all()
            rp, rm, rv, _, _ = _clip_adam_f64(p, g, m, v, step)
            np.testing.assert_allclose(opt.m.cpu().numpy(), rm, rtol=1e-6)
            np.testing.assert_allclose(opt.v.cpu().numpy(), rv, rtol=1e-6)
            upd = opt.p.cpu().numpy().astype(np.float64) - p
            assert (np.abs(upd - (rp - p)) <= 1e-4 * np.abs(rp - p) +
                    1e-4 * np.abs(rp - p).max() + 2.0 ** -24 * np.abs(rp)).all()
            continue
        _close_to_f64(opt, gd, p, _clip_adam_f64(p, g, m, v, step))
        # (an element the loops skipped, or visited twice, misses the update
        # tolerance above: its error is the whole update)
        if n > 1000:
            assert (opt.p.cpu().numpy() != p).mean() > 0.99


@pytest.mark.parametrize("n", [257, 2048 * 256 + 257])
def test_clip_adam_sched_and_grad_scale(n):
    """dr_clip_adam_sched (the data-parallel step's optimizer): with
    grad_scale 1 bitwise dr_clip_adam of the same step count; with grad_scale
    0.5 bitwise dr_clip_adam of 0.5 g (a power of two is exact through the
    norm and the clip); with grad_scale 1/3 within the element tolerances of
    the f64 restatement on g / 3."""
    step = 4
    for gscale in (10.0, 1e-4):
        p, g, m, v = _adam_state(n, gscale, n + 11)

        def run(grad, scale):
            opt = _adam_opt(p, m, v, step)
            gd = torch.from_numpy(grad.copy()).cuda()
            if scale is None:
                opt.step(gd)
            else:
                sched = opt.schedule(step, 1)[0].contiguous().cuda()
                opt.step_sched(gd, sched, scale)
            torch.cuda.synchronize()
            return opt, gd

        base, gb = run(g, None)
        one, g1 = run(g, 1.0)
        for a, b in ((base.p, one.p), (base.m, one.m), (base.v, one.v), (gb, g1),
                     (base.grad_norm, one.grad_norm)):
            assert torch.equal(a, b)
        half_ref, gh = run((0.5 * g).astype(np.float32), None)
        half, g2 = run(g, 0.5)
        for a, b in ((half_ref.p, half.p), (half_ref.m, half.m), (half_ref.v, half.v),
                     (gh, g2), (half_ref.grad_norm, half.grad_norm)):
            assert torch.equal(a, b)
        assert not torch.equal(half.p, base.p)
        third, g3 = run(g, 1.0 / 3.0)
        _close_to_f64(third, g3, p, _clip_adam_f64(p, g.astype(np.float64) / 3.0, m, v, step))
