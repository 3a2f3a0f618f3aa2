"""SB3 PPO.train's minibatch loss, gradient and fp32 error envelope in f64
(SURVEY.md Appendix C restatement; SB3 is absent, so "parity unpinned" with
respect to SB3 itself).  Test infrastructure shared by the flagship-size
parity test and the data-parallel union-gradient check
(tests/test_ppo_flagship_parity_gpu.py, tests/dp_train_worker.py)."""
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
