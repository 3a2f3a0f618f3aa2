"""SB3 PPO.train's minibatch loss, gradient and fp32 error envelope in f64
(SURVEY.md Appendix C restatement; SB3 is absent, so "parity unpinned" with
respect to SB3 itself).  Test infrastructure shared by the flagship-size
parity test and the data-parallel union-gradient check
(tests/test_ppo_flagship_parity_gpu.py, tests/dp_train_worker.py)."""
import functools

import numpy as np
import torch

U = 2.0 ** -24
# the network's tanh on the GPU (common.h tanh_rat): <= 6 ulp from the
# correctly rounded tanh, against torch's <= 1-2; its derivative factor
# 1 - h^2 then carries an absolute error <= 2 |h| 6 u |h| + u <= 13 u.
# Measured on an MI355X against f64 over 2.1 M inputs (every normal result,
# tests/test_tanh_device_gpu.py): worst 4.703 ulp
TANH_ULP = 6


def gamma(n: int) -> float:
    """Higham's gamma_n = n u / (1 - n u) for n dependent fp32 roundings."""
    return n * U / (1 - n * U)


def _chain_base(obs_dim: int, arch) -> int:
    """What every gradient entry's chain of dependent fp32 roundings holds
    besides the sum over rows, counted as the flagship parity test counts it:

      forward dots    obs_dim + sum(arch)      each layer's K, the head's K
      backward dots   4 + sum(arch[1:])        head -> top hidden (K = 4), then
                                               grad_h = grad_z W per layer
      elementwise     448                      the flagship's allowance for the
                                               loss row, the normalisation and
                                               the tanh derivative products
      tanh            4 * TANH_ULP             each tanh / derivative factor as
                                               TANH_ULP roundings (2 layers x 2)
    """
    arch = tuple(arch)
    return obs_dim + sum(arch) + 4 + sum(arch[1:]) + 448 + 4 * TANH_ULP


def chain_length(obs_dim: int, arch, m: int) -> int:
    """The chain behind a gradient entry whose sum over the m rows runs in an
    order that is not known (a library GEMM, torch's CPU autograd): the base
    (_chain_base) + m, since a sum of m terms obeys gamma_{m-1} in every
    order (Higham, eq. 4.4).  The project's own kernels have a known launch
    geometry and a shorter chain: step_chain_lengths."""
    return _chain_base(obs_dim, arch) + m


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def head_row_chain(m: int):
    """(gradient, scalar) row terms of ppo_head_kernel and its finish, rows
    per partial + number of partials as the flagship test counts them.
    Launch: nb = min(ceil(m / 8), 1024) blocks; each of a role's 2 waves per
    block takes 4-row tiles with stride 2 nb, t = ceil(ceil(m / 4) / (2 nb))
    tiles.  A lane's weight / bias accumulators (sw, sb) add 4 t rows; a
    loss term or head-bias entry (u[k]) adds one row per tile (t), then the
    64-lane butterfly (6 levels).  The block adds its 4 wave slots (3 adds)
    and the nb per-block rows are summed by the finish (grouped or direct:
    the same two-level order), counted as nb."""
    nb = min(_cdiv(m, 8), 1024)
    t = _cdiv(_cdiv(m, 4), 2 * nb)
    return max(4 * t, t + 6) + 3 + nb, t + 6 + 3 + nb


def first_row_chain(m: int) -> int:
    """Row term of first_layer_bwd_kernel + finish: nb = min(ceil(m / 16),
    256) blocks per net, each of the 4 nb waves t = ceil(ceil(m / 4) / (4 nb))
    tiles of 4 rows accumulated per lane (4 t), two adds combine the block's
    four waves, nb per-block rows are summed by the finish."""
    nb = min(_cdiv(m, 16), 256)
    t = _cdiv(_cdiv(m, 4), 4 * nb)
    return 4 * t + 2 + nb


def fused_first_row_chain(m: int, n_cu: int) -> int:
    """Row term of dr_gemm_x6_bwd_first (gemm_x6_fl16_kernel) + finish: per
    net `per` = min(2 (m / 32), n_cu rounded down to even) / 2 blocks, each R =
    ceil((m / 32) / per) row steps of 32 rows accumulated in its MFMA
    accumulator (32 R), then `per` per-block rows summed by the finish."""
    steps = m // 32
    grid = min(2 * steps, n_cu)
    per = (grid - grid % 2) // 2
    return 32 * _cdiv(steps, per) + per


def split_k_row_chain(m: int, chunks: int = 64) -> int:
    """Row term of the hidden layers' weight gradient (FusedTrainStep._wgrad2
    / _wgrad): C = 64 chunks of m / 64 rows, each a GEMM (dr_gemm_x6_wgrad or
    the library's: m / C accumulated rows) and a sum of the C chunks, when 64
    divides m; otherwise ONE library GEMM over all m rows, whose order is
    not known: m."""
    return m // chunks + chunks if m % chunks == 0 else m


def step_chain_lengths(obs_dim: int, arch, m: int, fused_first: bool = False,
                       n_cu: int = 256) -> dict:
    """The longest chain of dependent fp32 roundings behind each gradient
    tensor (SB3 names) of FusedTrainStep.step on an m-row minibatch: the base
    (_chain_base) + the row term of the kernel that reduces that tensor over
    the rows, from its launch geometry --

      heads, log_std, the top layer's biases   head_row_chain(m)[0]
      the top layer's weights (depth 2)        split_k_row_chain(m)
      the first layer (depth 2)                fused_first_row_chain(m, n_cu)
                                               with the fused
                                               dr_gemm_x6_bwd_first
                                               (fused_first), else
                                               first_row_chain(m)
      the only layer's weights (depth 1)       split_k_row_chain(m)
    """
    arch = tuple(arch)
    if len(arch) not in (1, 2):
        raise ValueError("step_chain_lengths: depth 1 or 2")
    base = _chain_base(obs_dim, arch)
    head = base + head_row_chain(m)[0]
    top = base + split_k_row_chain(m)
    first = base + (fused_first_row_chain(m, n_cu) if fused_first else first_row_chain(m))
    n = {"log_std": head}
    for net, hd in (("policy_net", "action_net"), ("value_net", "value_net")):
        n[f"{hd}.weight"] = n[f"{hd}.bias"] = head
        k = 2 * (len(arch) - 1)
        n[f"mlp_extractor.{net}.{k}.bias"] = head
        n[f"mlp_extractor.{net}.{k}.weight"] = top
        if len(arch) == 2:
            n[f"mlp_extractor.{net}.0.weight"] = n[f"mlp_extractor.{net}.0.bias"] = first
    return n


def stats_chain_length(m: int) -> int:
    """The chain of the sum over rows behind a loss statistic of
    FusedTrainStep.step (a mean over the m rows): head_row_chain(m)'s scalar
    term + 4 for the finish's product with the fp32 1 / m and the weighted
    sum that forms `loss`."""
    return head_row_chain(m)[1] + 4


def grad_bound(env, env_act, n):
    """Per-entry fp32 bound of a gradient: gamma(n) x the envelope + the tanh
    derivative factor's absolute error x the activation envelope (the
    flagship parity test's two terms).  n: one chain length, or one per
    tensor (a dict by the envelope's names)."""
    nk = (lambda k: n[k]) if isinstance(n, dict) else (lambda k: n)
    return {k: gamma(nk(k)) * env[k] + (2 * TANH_ULP + 1) * U * env_act[k] for k in env}


def forward64(sd, arch, obs):
    """(mean (m, 4), value (m,)) of the SB3-named state dict in f64."""
    x = torch.as_tensor(obs).double()
    out = []
    for net, head in (("policy_net", "action_net"), ("value_net", "value_net")):
        h = x
        for k in range(len(arch)):
            h = torch.tanh(h @ sd[f"mlp_extractor.{net}.{2 * k}.weight"].double().T +
                           sd[f"mlp_extractor.{net}.{2 * k}.bias"].double())
        out.append(h @ sd[f"{head}.weight"].double().T + sd[f"{head}.bias"].double())
    return out[0], out[1].flatten()


def logp64(mean, log_std, act):
    """Diagonal-Gaussian log-prob of act (m, 4), all in f64."""
    z = (torch.as_tensor(act).double() - mean) / log_std.double().exp()
    return (-0.5 * z ** 2 - log_std.double() - 0.5 * np.log(2 * np.pi)).sum(1)


def midtraining_minibatch(obs_dim, arch, m, seed, clip=0.2, adv_offset=0.0):
    """A minibatch as PPO sees it in the middle of training: the policy has
    moved since the rollout, so the ratio spreads around 1 and both clip
    edges, both branches of min(l1, l2) and the clamp's zero gradient are
    engaged, with the gradient's weight spread over many rows.  Built on the
    CPU from one torch.Generator; every property asserted below comes from
    the f64 reference alone.

    Rows whose f64 ratio lies within 1e-4 (relative) of 1 - clip or 1 + clip
    get old_logp += 0.01 (at most three passes): that close to an edge an
    fp32 evaluation may take the other branch, a discontinuity that no
    rounding bound covers, and old_logp is a free input.

    Asserted here at every m: the guard band is empty and at most 1 % of the
    rows were moved.  Asserted only at m >= 100: 10-35 % of the rows beyond
    each clip edge and >= m / 4 effective rows behind the policy gradient --
    these are statistics of the draw, which a handful of rows (m = 1 in the
    dr_ppo_loss row tests) cannot carry; below 100 rows the minibatch keeps
    the recipe and the empty guard band, nothing more.

    Returns a dict: sd (SB3-named f32 state dict), arch, obs (m, obs_dim),
    act (m, 4), old_logp, adv, ret (m,), all f32 tensors; mean64, value64,
    ratio64, adv_norm64 (f64); moved (rows nudged), frac_below, frac_above,
    eff_rows."""
    from drone_rl_amd.policy import ActorCritic
    arch = tuple(arch)
    g = torch.Generator().manual_seed(seed)
    pol = ActorCritic(obs_dim, 4, arch, seed=seed, device="cpu")
    with torch.no_grad():
        pol.flat.mul_(1.5)
        pol.log_std.copy_(torch.tensor([-0.7, 0.1, -0.3, 0.4]))
    sd = pol.state_dict()
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    obs = (1.5 * rn(m, obs_dim)).float()
    mean, value = forward64(sd, arch, obs)
    std = sd["log_std"].double().exp()
    act = (mean + std * rn(m, 4)).float()
    lp = logp64(mean, sd["log_std"], act)
    old_logp = (lp - 0.25 * rn(m)).float()
    adv = (adv_offset + 0.3 + 2.0 * rn(m)).float()
    ret = (value + rn(m)).float()
    lo, hi = 1.0 - clip, 1.0 + clip
    moved = torch.zeros(m, dtype=torch.bool)
    for _ in range(3):
        ratio = torch.exp(lp - old_logp.double())
        band = ((ratio / lo - 1).abs() <= 1e-4) | ((ratio / hi - 1).abs() <= 1e-4)
        if not band.any():
            break
        old_logp = torch.where(band, old_logp + 0.01, old_logp)
        moved |= band
    ratio = torch.exp(lp - old_logp.double())
    band = ((ratio / lo - 1).abs() <= 1e-4) | ((ratio / hi - 1).abs() <= 1e-4)
    assert not band.any(), "rows left in the clip edges' guard band"
    n_moved = int(moved.sum())
    assert n_moved <= 0.01 * m, f"{n_moved} of {m} rows moved off the clip edges"
    A = adv.double()
    A = (A - A.mean()) / (A.std() + 1e-8) if m > 1 else A
    below = (ratio < lo).double().mean().item()
    above = (ratio > hi).double().mean().item()
    # rows whose unclipped branch carries the gradient: not (A > 0 and r above)
    # and not (A < 0 and r below)
    active = ~(((A > 0) & (ratio > hi)) | ((A < 0) & (ratio < lo)))
    w = (A.abs() * ratio) * active
    w = w / w.sum()
    eff = 1.0 / (w ** 2).sum().item()
    if m >= 100:          # the fractions are statistics: asserted where m carries them
        assert 0.10 <= below <= 0.35 and 0.10 <= above <= 0.35, (below, above)
        assert eff >= m / 4, (eff, m)
    return dict(sd=sd, arch=arch, obs=obs, act=act, old_logp=old_logp, adv=adv, ret=ret,
                mean64=mean, value64=value, ratio64=ratio, adv_norm64=A, moved=n_moved,
                frac_below=below, frac_above=above, eff_rows=eff)


def f64_reference(sd, arch, obs, act, old_logp, adv, ret, clip, vf_coef, normalize,
                  device="cpu", with_act=False, ent_coef=0.0, with_stats=False):
    """SB3 PPO.train's minibatch loss in f64 with its gradient (SB3 names)
    and the absolute-value envelope of every gradient entry.  with_stats:
    also (last) a dict of the eight SB3 stats in f64, name -> (value,
    envelope), the envelope of a mean being the mean of |terms|.  with_act: also
    the activation envelope, the same backward with the tanh derivative
    factor |1 - h^2| replaced by 1 -- times 13 u it bounds, to first order,
    what the derivative factor's absolute error (TANH_ULP) adds to an entry,
    which the relative envelope misses where tanh saturates."""
    d = lambda x: torch.as_tensor(np.asarray(x) if not torch.is_tensor(x) else x,  # noqa: E731
                                  dtype=torch.float64, device=device)
    W = {k: d(v).clone().requires_grad_(True) for k, v in sd.items()}
    x = d(obs)
    hs = {}
    outs = {}
    for net, head in (("policy_net", "action_net"), ("value_net", "value_net")):
        h = x
        lay = []
        for k in range(len(arch)):
            z = h @ W[f"mlp_extractor.{net}.{2 * k}.weight"].T + \
                W[f"mlp_extractor.{net}.{2 * k}.bias"]
            lay.append((h, z))
            h = torch.tanh(z)
            z.retain_grad()
        hs[net] = (lay, h)
        o = h @ W[f"{head}.weight"].T + W[f"{head}.bias"]
        o.retain_grad()
        outs[net] = o
    mean, value = outs["policy_net"], outs["value_net"].flatten()
    log_std = W["log_std"]
    a = d(act)
    z_std = (a - mean) / log_std.exp()
    lp_dim = -0.5 * z_std ** 2 - log_std - 0.5 * np.log(2 * np.pi)
    lp_dim.retain_grad()
    log_prob = lp_dim.sum(1)
    A = d(adv)
    A_raw = A
    if normalize and A.numel() > 1:              # SB3: len(advantages) > 1
        A = (A - A.mean()) / (A.std() + 1e-8)
    logr = log_prob - d(old_logp)
    ratio = torch.exp(logr)
    surr = torch.min(A * ratio, A * torch.clamp(ratio, 1 - clip, 1 + clip))
    pol = -surr.mean()
    verr = (d(ret) - value) ** 2
    vloss = torch.mean(verr)
    # the diagonal Gaussian's entropy is row-independent; entropy_loss = -H
    ent_terms = 0.5 + 0.5 * np.log(2 * np.pi) + log_std
    eloss = -ent_terms.sum()
    loss = pol + ent_coef * eloss + vf_coef * vloss
    loss.backward()
    g = {k: v.grad.detach().clone() for k, v in W.items()}
    # envelope: the backward with |.| products
    env, env_act = {}, {}
    for net, head in (("policy_net", "action_net"), ("value_net", "value_net")):
        lay, htop = hs[net]
        dout = outs[net].grad.detach().abs()                 # (M, 4) or (M, 1)
        Wh = W[f"{head}.weight"].detach().abs()
        env[f"{head}.weight"] = dout.T @ htop.detach().abs()
        env[f"{head}.bias"] = dout.sum(0)
        env_act[f"{head}.weight"] = torch.zeros_like(env[f"{head}.weight"])
        env_act[f"{head}.bias"] = torch.zeros_like(env[f"{head}.bias"])
        dh = dout @ Wh                                       # |dL/dh| envelope
        dh_a = dh
        for k in reversed(range(len(arch))):
            h_in, z = lay[k]
            th = torch.tanh(z.detach())
            dz = dh * (1 - th ** 2).abs()
            env[f"mlp_extractor.{net}.{2 * k}.weight"] = dz.T @ h_in.detach().abs()
            env[f"mlp_extractor.{net}.{2 * k}.bias"] = dz.sum(0)
            if with_act:
                env_act[f"mlp_extractor.{net}.{2 * k}.weight"] = dh_a.T @ h_in.detach().abs()
                env_act[f"mlp_extractor.{net}.{2 * k}.bias"] = dh_a.sum(0)
            dh = dz @ W[f"mlp_extractor.{net}.{2 * k}.weight"].detach().abs()
            dh_a = dh_a @ W[f"mlp_extractor.{net}.{2 * k}.weight"].detach().abs()
    # log_std: d lp_dim / d log_std = z^2 - 1 per row and dimension
    env["log_std"] = (lp_dim.grad.detach() * (z_std.detach() ** 2 - 1)).abs().sum(0) + \
        (lp_dim.grad.detach()).abs().sum(0) + abs(ent_coef)
    out = [g, env]
    if with_act:
        env_act["log_std"] = torch.zeros_like(env["log_std"])
        out.append(env_act)
    if with_stats:
        with torch.no_grad():
            kl = (ratio - 1) - logr
            pe, ve = surr.abs().mean().item(), verr.mean().item()
            ee = ent_terms.abs().sum().item()
            many = A_raw.numel() > 1
            out.append({
                "loss": (loss.item(), pe + abs(ent_coef) * ee + vf_coef * ve),
                "policy_loss": (pol.item(), pe),
                "value_loss": (vloss.item(), ve),
                "entropy_loss": (eloss.item(), ee),
                "clip_fraction": (((ratio - 1).abs() > clip).double().mean().item(), 1.0),
                "clip_count": int(((ratio - 1).abs() > clip).sum().item()),
                "approx_kl": (kl.mean().item(), kl.abs().mean().item()),
                "adv_mean": (A_raw.mean().item(), A_raw.abs().mean().item()),
                "adv_std": (A_raw.std().item() if many else float("nan"),
                            A_raw.std().item() if many else float("nan")),
            })
    return tuple(out)


# --------------------------------------------------------------------------
# The rollout-side forward (PolicyInference, ActorCritic.forward): f64 with a
# running fp32 bound, a plain fp32 restatement, the fixtures and the two-tier
# check shared by tests/test_policy_forward_bound_cpu.py and
# tests/test_policy_inference_f64_gpu.py.  Nothing here comes from the kernels.

SHARP = 4.0     # margin of the sharp check: test_policy_forward_bound_cpu (b)


def _net_layers(sd, arch, net, head):
    """[(W, b)] of one MLP in f64: its hidden layers, then its head."""
    names = [f"mlp_extractor.{net}.{2 * k}" for k in range(len(arch))] + [head]
    return [(sd[f"{n}.weight"].double(), sd[f"{n}.bias"].double()) for n in names]


_NETS = (("policy_net", "action_net"), ("value_net", "value_net"))


def ulp32(x):
    """Spacing of the f32 grid at |x| (f64 tensor in, f64 out; the normal
    range's smallest spacing below it)."""
    _, e = torch.frexp(torch.as_tensor(x, dtype=torch.float64).abs())
    return torch.ldexp(torch.ones_like(e, dtype=torch.float64), (e - 24).clamp(min=-149))


def forward_bound64(sd, arch, obs):
    """(mean64 (m, 4), dmean, value64 (m,), dvalue): the f64 forward and, per
    output entry, a bound on what ANY fp32 evaluation (every summation order,
    fused or unfused multiply-adds, a tanh within TANH_ULP ulp) can differ
    from it.  Per layer with input h, input error dh, K inputs and envelope
    env = |h| |W|^T + |b|:

        dz  = dh |W|^T + gamma(K + 2) (env + dh |W|^T)
              the propagated input error, and K products + K - 1 sums + the
              bias add (+ 1 spare) on the inputs as computed, |h^| <= |h| + dh
        dh' = dz + 2 TANH_ULP u max(|tanh z|, 2^-126)
              tanh is 1-Lipschitz; ulp(t) <= 2 u |t|

    The x6 GEMM counts as an fp32 dot (tests/test_gemm_x6_gpu.py)."""
    x = torch.as_tensor(obs).double()
    out = []
    for net, head in _NETS:
        layers = _net_layers(sd, arch, net, head)
        h, dh = x, torch.zeros_like(x)
        for k, (W, b) in enumerate(layers):
            aW = W.abs().T
            prop = dh @ aW
            dz = prop + gamma(W.shape[1] + 2) * (h.abs() @ aW + b.abs() + prop)
            z = h @ W.T + b
            if k == len(layers) - 1:
                out += [z, dz]
                break
            h = torch.tanh(z)
            dh = dz + 2 * TANH_ULP * U * h.abs().clamp(min=2.0 ** -126)
    return out[0], out[1], out[2].flatten(), out[3].flatten()


def forward32_cpu(sd, arch, obs, tanh_ulps=0, bf16_layer=None, generator=None):
    """(mean (m, 4), value (m,)) by the plain fp32 restatement: torch's CPU
    fp32 `@`, the bias added in fp32, tanh taken in f64 and rounded to f32.
    Two deliberate defects for the margin / rejection tests: tanh_ulps moves
    every tanh result by a uniform draw in +-tanh_ulps ulp (from `generator`);
    bf16_layer rounds that layer's operands (its input and its weights;
    hidden layers count from 0, the head is layer len(arch)) to bf16."""
    x = torch.as_tensor(obs).float()
    out = []
    for net, head in _NETS:
        layers = _net_layers(sd, arch, net, head)
        h = x
        for k, (W, b) in enumerate(layers):
            W32 = W.float()
            if bf16_layer == k:
                h, W32 = h.bfloat16().float(), W32.bfloat16().float()
            z = h @ W32.T + b.float()
            if k == len(layers) - 1:
                out.append(z)
                break
            h = torch.tanh(z.double()).float()
            if tanh_ulps:
                r = 2 * torch.rand(h.shape, generator=generator, dtype=torch.float64) - 1
                h = (h.double() + tanh_ulps * r * ulp32(h.double())).float()
    return out[0], out[1].flatten()


def inference_fixture(obs_dim, arch, m, seed, scale):
    """A policy and m observations for the rollout-side forward, all from one
    torch.Generator: ActorCritic's init with flat *= scale, then flat += 0.05
    randn -- every bias non-zero (action.b, value.b and the top layer's
    included), outputs of rms 0.5-2 instead of a fresh init's 0.04; obs = 1.5
    randn (f32) with row 0 all zeros and, when m >= 3, row 1 all 50.0 (the
    position limit: the first layer saturates).  The parameters are drawn
    before the observations, so m does not change the policy.
    Returns dict(sd, arch, obs)."""
    from drone_rl_amd.policy import ActorCritic
    arch = tuple(arch)
    g = torch.Generator().manual_seed(seed)
    pol = ActorCritic(obs_dim, 4, arch, seed=seed, device="cpu")
    with torch.no_grad():
        pol.flat.mul_(scale)
        pol.flat.add_(0.05 * torch.randn(pol.num_params, generator=g))
    obs = 1.5 * torch.randn(m, obs_dim, generator=g)
    obs[0] = 0.0
    if m >= 3:
        obs[1] = 50.0
    return dict(sd=pol.state_dict(), arch=arch, obs=obs)


# (id, obs_dim, arch, n, scale): every path of the rollout-side forward, each
# at the smallest size that reaches it (the module docstring of
# tests/test_policy_inference_f64_gpu.py says which)
INFERENCE_CASES = [
    ("x6_fused_images_128", 15, (256, 256), 128, 1.5),
    ("x6_fused_images_384", 15, (256, 256), 384, 1.5),
    ("x6_refresh", 19, (256, 256), 256, 1.5),
    ("library_ragged", 15, (256, 256), 1000, 1.5),
    ("one_env", 15, (64, 64), 1, 1.5),
    ("unequal", 18, (64, 128), 257, 1.5),
    ("depth1", 12, (128,), 255, 1.5),
    ("depth3", 16, (64, 64, 64), 300, 1.5),
    ("narrow_head", 32, (256, 252), 100, 1.5),
    ("tiny", 4, (4,), 7, 1.5),
    ("width_8", 8, (64, 64), 65, 1.5),
    ("width_24", 24, (64, 64), 65, 1.5),
    ("second_round", 15, (64, 64), 2053, 1.5),
    ("saturated", 15, (256, 256), 384, 4.0),
]
INFERENCE_SEED = 11
SMALL_N = 64            # below it the sharp check is per entry, against SMALL_REF_ROWS rows
SMALL_REF_ROWS = 256


def _errors(mean, value, mean64, value64):
    """|out - f64| over all 5 m outputs as one (m, 5) f64 tensor."""
    m = torch.as_tensor(mean).detach().cpu().double().reshape(mean64.shape)
    v = torch.as_tensor(value).detach().cpu().double().reshape(value64.shape)
    return torch.cat([(m - mean64).abs(), (v - value64).abs()[:, None]], 1)


def inference_reference(sd, arch, obs):
    """What check_inference needs of one (policy, observations) pair: the f64
    outputs with their hard bound (forward_bound64 + one fp32 ulp of the
    reference for the final store) and the plain restatement's rms / largest
    error (forward32_cpu), the sharp check's yardstick."""
    mean64, dmean, value64, dvalue = forward_bound64(sd, arch, obs)
    ref = torch.cat([mean64, value64[:, None]], 1)
    hard = torch.cat([dmean, dvalue[:, None]], 1) + ulp32(ref)
    err32 = _errors(*forward32_cpu(sd, arch, obs), mean64, value64)
    return dict(mean64=mean64, value64=value64, dmean=dmean, dvalue=dvalue, hard=hard,
                ref_rms=err32.pow(2).mean().sqrt().item(), ref_max=err32.max().item(),
                ref_hard=(err32 / hard).max().item(), n=obs.shape[0])


@functools.lru_cache(maxsize=None)
def inference_case(obs_dim, arch, n, scale, seed=INFERENCE_SEED):
    """inference_fixture + inference_reference of one case, computed once per
    process and shared (read-only) by every test that needs it.  Below
    SMALL_N rows an rms says little, so `small_max` is the plain
    restatement's largest error on the same policy's SMALL_REF_ROWS-row
    fixture."""
    fx = inference_fixture(obs_dim, arch, n, seed, scale)
    fx.update(inference_reference(fx["sd"], fx["arch"], fx["obs"]))
    if n < SMALL_N:
        fx["small_max"] = inference_case(obs_dim, arch, SMALL_REF_ROWS, scale, seed)["ref_max"]
    return fx


def check_inference(ref, mean, value, rows=None):
    """The two-tier criterion on outputs (mean, value) of the case `ref`
    (inference_case / inference_reference), over all rows or `rows`:

      hard   every entry within its fp32 bound: max error / bound <= 1
      sharp  n >= SMALL_N: the rms error over all 5 n outputs <= SHARP x the
             plain fp32 restatement's on the same fixture; below: every
             entry's error <= SHARP x the restatement's largest on the same
             policy's SMALL_REF_ROWS-row fixture

    Returns dict(hard, sharp, hard_ok, sharp_ok): the two ratios (sharp
    already divided by what it is compared with, so <= SHARP passes) and the
    verdicts; a non-finite output fails both."""
    err = _errors(mean, value, ref["mean64"], ref["value64"])
    hard_b = ref["hard"]
    if rows is not None:
        err, hard_b = err[rows], hard_b[rows]
    hard = (err / hard_b).max().item()
    if "small_max" in ref:
        sharp = err.max().item() / ref["small_max"]
    else:
        sharp = err.pow(2).mean().sqrt().item() / ref["ref_rms"]
    finite = bool(torch.isfinite(err).all())
    return dict(hard=hard, sharp=sharp, hard_ok=finite and hard <= 1.0,
                sharp_ok=finite and sharp <= SHARP)
