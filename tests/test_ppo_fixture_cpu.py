"""The in-distribution minibatch fixture (ppo_f64.midtraining_minibatch) and
the f64 reference's bound, checked without a GPU.

* The fixture's own properties (guard band empty, <= 1 % of rows moved, 10-35 %
  of rows beyond each clip edge, >= m / 4 effective rows) at the four
  configurations of tests/test_ppo_step_f64_gpu.py.
* The reference alone stays inside the bound: torch's fp32 CPU autograd of
  the same loss -- an independent fp32 evaluation with its own summation
  orders and a 1-2 ulp tanh -- is within the entrywise bound gamma(n) x
  envelope + (2 TANH_ULP + 1) u x activation envelope, n =
  ppo_f64.chain_length (3,307 / 987 / 1,814 for the depth-2 configurations:
  the order of torch's CPU reductions is not known, so the row term is m).
  Measured worst error / bound: 0.0004 (15, 2x256, 2048), 0.0048 (19, 2x64,
  300), 0.0009 (18, 64-128, 1000), the same with ent_coef = 0.01.

Fixture properties at seed 3 (fraction below / above the clip interval, rows
moved, effective rows): 0.182 / 0.225 / 1 / 993 at (15, 2x256, 2048); 0.187 /
0.267 / 0 / 149 at (19, 2x64, 300); 0.193 / 0.233 / 0 / 478 at (18, 64-128,
1000); 0.183 / 0.245 / 0 / 118 at (12, 128, 257)."""
import numpy as np
import pytest
import torch

from ppo_f64 import (chain_length, f64_reference, forward64, grad_bound, logp64,
                     midtraining_minibatch)

CONFIGS = [(15, (256, 256), 2048), (19, (64, 64), 300), (18, (64, 128), 1000),
           (12, (128,), 257)]


@pytest.mark.parametrize("obs_dim,arch,m", CONFIGS)
def test_midtraining_fixture_properties(obs_dim, arch, m):
    mb = midtraining_minibatch(obs_dim, arch, m, seed=3)
    print(f"below {mb['frac_below']:.3f} above {mb['frac_above']:.3f} moved {mb['moved']} "
          f"effective rows {mb['eff_rows']:.0f}")
    assert mb["moved"] <= 0.01 * m
    assert 0.10 <= mb["frac_below"] <= 0.35 and 0.10 <= mb["frac_above"] <= 0.35
    assert mb["eff_rows"] >= m / 4
    r = mb["ratio64"]
    for edge in (0.8, 1.2):
        assert ((r / edge - 1).abs() > 1e-4).all()
    # what it returns is consistent: the ratio is that of the returned arrays
    mean, _ = forward64(mb["sd"], arch, mb["obs"])
    lp = logp64(mean, mb["sd"]["log_std"], mb["act"])
    assert torch.equal(torch.exp(lp - mb["old_logp"].double()), r)
    # and it is a function of its arguments alone
    again = midtraining_minibatch(obs_dim, arch, m, seed=3)
    for k in ("obs", "act", "old_logp", "adv", "ret"):
        assert torch.equal(mb[k], again[k])
    assert mb["obs"].dtype == torch.float32 and mb["obs"].shape == (m, obs_dim)


def test_midtraining_fixture_advantage_offset():
    """adv_offset shifts the raw advantages only (the spread and every other
    array stay): the normalised advantage is unchanged to f32 rounding."""
    a = midtraining_minibatch(15, (64, 64), 1000, seed=3)
    b = midtraining_minibatch(15, (64, 64), 1000, seed=3, adv_offset=100.0)
    assert abs(b["adv"].double().mean().item() - a["adv"].double().mean().item() - 100) < 1e-4
    for k in ("obs", "act", "old_logp", "ret"):
        assert torch.equal(a[k], b[k])
    assert (a["adv_norm64"] - b["adv_norm64"]).abs().max().item() < 1e-5


def _f32_autograd(mb, clip, vf_coef, ent_coef, normalize):
    """torch fp32 autograd of SB3 PPO.train's minibatch loss on the CPU."""
    sd, arch = mb["sd"], mb["arch"]
    W = {k: v.clone().float().requires_grad_(True) for k, v in sd.items()}
    outs = []
    for net, head in (("policy_net", "action_net"), ("value_net", "value_net")):
        h = mb["obs"]
        for k in range(len(arch)):
            h = torch.tanh(torch.nn.functional.linear(
                h, W[f"mlp_extractor.{net}.{2 * k}.weight"],
                W[f"mlp_extractor.{net}.{2 * k}.bias"]))
        outs.append(torch.nn.functional.linear(h, W[f"{head}.weight"], W[f"{head}.bias"]))
    mean, value = outs[0], outs[1].flatten()
    dist = torch.distributions.Normal(mean, W["log_std"].exp())
    lp = dist.log_prob(mb["act"]).sum(1)
    A = mb["adv"]
    if normalize:
        A = (A - A.mean()) / (A.std() + 1e-8)
    ratio = torch.exp(lp - mb["old_logp"])
    pol = -torch.min(A * ratio, A * torch.clamp(ratio, 1 - clip, 1 + clip)).mean()
    vl = torch.nn.functional.mse_loss(mb["ret"], value)
    el = -dist.entropy().sum(1).mean()
    (pol + ent_coef * el + vf_coef * vl).backward()
    return {k: v.grad.double() for k, v in W.items()}


@pytest.mark.parametrize("ent_coef", [0.0, 0.01])
@pytest.mark.parametrize("obs_dim,arch,m", CONFIGS[:3])
def test_f32_autograd_stays_within_the_f64_bound(obs_dim, arch, m, ent_coef):
    mb = midtraining_minibatch(obs_dim, arch, m, seed=3)
    g_ref, env, env_act, stats = f64_reference(
        mb["sd"], arch, mb["obs"], mb["act"], mb["old_logp"], mb["adv"], mb["ret"], 0.2, 0.5,
        True, with_act=True, ent_coef=ent_coef, with_stats=True)
    bound = grad_bound(env, env_act, chain_length(obs_dim, arch, m))
    g32 = _f32_autograd(mb, 0.2, 0.5, ent_coef, True)
    worst = 0.0
    for k in g_ref:
        r = ((g32[k] - g_ref[k]).abs() / (bound[k] + 1e-30)).max().item()
        worst = max(worst, r)
        assert r <= 1.0, f"{k}: fp32 autograd {r:.3f} x its bound"
    print(f"worst error / bound: {worst:.4f}")
    # the stats the reference reports are those of its own fixture
    assert stats["clip_fraction"][0] == pytest.approx(mb["frac_below"] + mb["frac_above"],
                                                      abs=1e-12)
    assert stats["clip_count"] == round(stats["clip_fraction"][0] * m)


def test_f64_reference_entropy_term_and_stats():
    """ent_coef adds ent_coef * entropy_loss: -ent_coef on every log_std
    gradient entry (and +|ent_coef| on its envelope), nothing elsewhere; the
    stats are SB3's expressions of the same arrays."""
    mb = midtraining_minibatch(12, (128,), 257, seed=3)
    a = (mb["sd"], mb["arch"], mb["obs"], mb["act"], mb["old_logp"], mb["adv"], mb["ret"],
         0.2, 0.5, True)
    g0, e0 = f64_reference(*a)
    g1, e1, st = f64_reference(*a, ent_coef=0.01, with_stats=True)
    for k in g0:
        if k == "log_std":
            assert torch.allclose(g1[k], g0[k] - 0.01, rtol=0, atol=1e-15)
            assert torch.allclose(e1[k], e0[k] + 0.01, rtol=0, atol=1e-15)
        else:
            assert torch.equal(g1[k], g0[k]) and torch.equal(e1[k], e0[k])
    r, A = mb["ratio64"], mb["adv_norm64"]
    pl = -torch.min(A * r, A * r.clamp(0.8, 1.2)).mean().item()
    vl = ((mb["ret"].double() - mb["value64"]) ** 2).mean().item()
    H = float((0.5 + 0.5 * np.log(2 * np.pi) + mb["sd"]["log_std"].double()).sum())
    assert st["policy_loss"][0] == pytest.approx(pl, rel=1e-12)
    assert st["value_loss"][0] == pytest.approx(vl, rel=1e-12)
    assert st["entropy_loss"][0] == pytest.approx(-H, rel=1e-12)
    assert st["loss"][0] == pytest.approx(pl - 0.01 * H + 0.5 * vl, rel=1e-12)
    assert st["approx_kl"][0] == pytest.approx(((r - 1) - r.log()).mean().item(), rel=1e-9)
    assert st["adv_mean"][0] == pytest.approx(mb["adv"].double().mean().item(), rel=1e-12)
    assert st["adv_std"][0] == pytest.approx(mb["adv"].double().std().item(), rel=1e-12)
    # a mean never exceeds the mean of |terms|
    assert all(abs(v[0]) <= v[1] * (1 + 1e-12) for k, v in st.items() if k != "clip_count")
