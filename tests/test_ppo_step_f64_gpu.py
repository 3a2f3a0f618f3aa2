"""FusedTrainStep.step against the f64 restatement of SB3's PPO.train on
minibatches that engage the clip (ppo_f64.midtraining_minibatch: 18-27 % of
rows beyond each edge of the clip interval, both branches of min(l1, l2)
taken, the clamp's zero gradient live, hundreds of rows carrying the policy
gradient), on every code path the trainer can select.  The flagship parity
test covers one point only: the first minibatch after a rollout, where the
ratio is exactly 1 on every row.

Gradient, per entry.  |fl(g_i) - g_i| <= gamma(n) * env_i + (2 TANH_ULP + 1) u
* env_act_i, the flagship test's two terms (ppo_f64.f64_reference: env is the
backward with every product replaced by the product of absolute values,
env_act the same with |1 - h^2| replaced by 1).  n is the longest chain of
dependent fp32 roundings behind an entry, counted as the flagship test counts
it (forward dots + backward dots + rows per partial sum + number of partials
+ its 448 for the elementwise steps + the tanh), per tensor and from the
launch geometry of the kernel that sums that tensor over the rows
(ppo_f64.step_chain_lengths).  What every entry shares:

    base = obs_dim + sum(arch)    forward dots: every layer's K, the head's K
         + 4 + sum(arch[1:])      backward dots: head -> top hidden, grad_z W
         + 448                    the flagship's allowance for the elementwise
                                  loss / normalisation / derivative steps
         + 4 TANH_ULP             tanh and its derivative factor, two layers

    15, (256, 256): 1,259   19, (64, 64): 687   18, (64, 128): 814   12, (128,): 616

The row term, per kernel:

  * ppo_head_kernel (heads, log_std, the top layer's biases; every path).
    min(ceil(m / 8), 1024) blocks; each of a role's two waves per block takes
    t = ceil(ceil(m / 4) / (2 blocks)) tiles of 4 rows -- t = 1 at every m
    here.  A lane's weight / bias accumulator adds 4 t rows, a loss term or
    head-bias entry t rows and the 64-lane butterfly (6); the block adds its
    4 wave slots (3); the per-block rows are summed by ppo_head_finish /
    the direct finish in grad_finish_kernel (two fixed levels either way),
    counted as their number: max(4, 7) + 3 + blocks = 266 / 48 / 135 / 43 at
    m = 2048 / 300 / 1000 / 257.
  * dr_gemm_x6_wgrad + the chunk sum (the 256 x 256 layers' weights, m =
    2048): 64 chunks of 32 rows, one k32 MFMA step each, then the 64-chunk
    sum (chunk_sum_part deferred, torch.sum otherwise): 32 + 64 = 96.
  * the library GEMM in its place (m = 300, 1000: 64 does not divide m, so
    ONE GEMM over all m rows; depth 1's layer-0 weights, m = 257, likewise):
    its order is not known, and a sum of m terms obeys gamma_{m-1} in every
    order (Higham eq. 4.4): m.
  * dr_gemm_x6_bwd_first (the first layer, x6_deferred cases only): on 256
    CUs min(2 * 64, 256) / 2 = 64 blocks per net, one 32-row step each in the
    MFMA accumulator, 64 per-block rows summed by first_finish_direct:
    32 + 64 = 96 (the CU count is read from the device).
  * first_layer_bwd_kernel (the first layer elsewhere): min(ceil(m / 16), 256)
    blocks per net, each wave ceil(ceil(m / 4) / (4 blocks)) = 1 tile of 4
    rows, 2 adds across the block's waves, the per-block rows summed by
    colsum_groups + the finish: 4 + 2 + blocks = 134 / 25 / 69 at m = 2048 /
    300 / 1000.

n = base + row term, per path (head tensors / top weights / first layer):

    15, (256, 256), m 2048, deferred       1,525 / 1,355 / 1,355
    same, per-kernel finishes, rows=       1,525 / 1,355 / 1,393
    19, (64, 64),   m 300                    735 /   987 /   712
    18, (64, 128),  m 1000                   949 / 1,814 /   883
    12, (128,),     m 257  (depth 1)         659 /   873 (layer-0 weights)

The x6 GEMMs count as fp32 dots: their product error is below one fp32
rounding (tests/test_gemm_x6_gpu.py).  No tolerance here is a fraction of a
tensor's largest entry.

Stats.  clip_fraction is a row count over m: the count must equal the f64
count exactly (the fixture keeps every row 1e-4 away from the clip edges, so
the count is well defined in fp32), and the fraction the count times the
kernel's fp32 1/m (two roundings).  loss, policy_loss, value_loss,
entropy_loss and approx_kl are within gamma(n_rows) x their f64 mean of
|terms|, n_rows the chain of the sum over rows alone
(ppo_f64.stats_chain_length): the head kernel's scalar term t + 6 + 3 +
blocks, + 4 for the finish's product with 1/m and the weighted sum that
forms `loss`: 270 / 52 / 139 / 47 at m = 2048 / 300 / 1000 / 257.  (A row's
own term carries the forward pass's roundings too, which a relative envelope
of the terms does not bound where a term cancels, approx_kl's (r - 1) - log r
for one; the measured ratios show what is left of the bound.)
adv_mean / adv_std: tests/test_ppo_kernels_gpu.py.

Measured on an MI355X, worst error / bound (gradient, stats):
    x6_deferred (trainer default)          0.0007   0.0029
    x6_per_kernel_finishes                 0.0007   0.0029
    x6_rows_in_place                       0.0007   0.0029
    library_gemms_ragged_19                0.0067   0.0129
    unequal_layers_18                      0.0017   0.0259
    depth1_ragged_12                       0.0028   0.0274
    x6_deferred_entropy                    0.0007   0.0022
    library_gemms_ragged_19_entropy        0.0067   0.0129
    x6_deferred_raw_advantage              0.0007   0.0022
    unequal_layers_18_adv_ready            0.0017   0.0259
(worst entries: the top hidden layer's weights; worst stats: loss, approx_kl,
value_loss).  The bound is a worst case over rounding signs and the errors
are not, hence the distance; what the test is for is an error that is not a
rounding error: with the clamp's gradient forced to 1 in ppo_row_policy all
ten cases fail, with the sign of ent_coef flipped in the head finish the two
entropy cases do.
"""
import functools

import pytest
import torch

from ppo_f64 import (f64_reference, gamma, grad_bound, midtraining_minibatch,
                     stats_chain_length, step_chain_lengths)

pytestmark = pytest.mark.gpu

KNOBS = ("DRONERL_X6_FUSED_IMAGES", "DRONERL_HEAD_DIRECT", "DRONERL_FL_FIRST",
         "DRONERL_GEMM_X6", "DRONERL_X6_FL", "DRONERL_X6_FL_DIRECT")
CLIP, VF = 0.2, 0.5
A = (15, (256, 256), 2048)
B = (19, (64, 64), 300)
C = (18, (64, 128), 1000)
D = (12, (128,), 257)

# (id, (obs_dim, arch, m), defer_finish, rows, adv_ready, ent_coef, normalize)
CASES = [
    ("x6_deferred", A, True, False, False, 0.0, True),
    ("x6_per_kernel_finishes", A, False, False, False, 0.0, True),
    ("x6_rows_in_place", A, True, True, False, 0.0, True),
    ("library_gemms_ragged_19", B, True, False, False, 0.0, True),
    ("unequal_layers_18", C, True, False, False, 0.0, True),
    ("depth1_ragged_12", D, False, False, False, 0.0, True),
    ("x6_deferred_entropy", A, True, False, False, 0.01, True),
    ("library_gemms_ragged_19_entropy", B, True, False, False, 0.01, True),
    ("x6_deferred_raw_advantage", A, True, False, False, 0.0, False),
    ("unequal_layers_18_adv_ready", C, True, False, True, 0.0, True),
]


@functools.lru_cache(maxsize=None)
def _fixture(cfg):
    return midtraining_minibatch(*cfg, seed=3, clip=CLIP)


@functools.lru_cache(maxsize=None)
def _reference(cfg, ent_coef, normalize):
    mb = _fixture(cfg)
    return f64_reference(mb["sd"], mb["arch"], mb["obs"], mb["act"], mb["old_logp"],
                         mb["adv"], mb["ret"], CLIP, VF, normalize, with_act=True,
                         ent_coef=ent_coef, with_stats=True)


def _run(cfg, defer, use_rows, adv_ready, ent_coef, normalize):
    """One FusedTrainStep.step on the fixture; the final flat gradient by
    SB3 name (f64, on the host), the eight stats, and whether the first
    layer's backward ran fused into dr_gemm_x6_bwd_first."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep, _sb3_name
    obs_dim, arch, m = cfg
    mb = _fixture(cfg)
    pol = ActorCritic(obs_dim, 4, arch, seed=0, device="cuda")
    pol.load_state_dict(mb["sd"])
    obs, act = mb["obs"].cuda(), mb["act"].cuda()
    aux = torch.stack([mb["old_logp"], mb["adv"], mb["ret"]], 1).contiguous().cuda()
    fs = FusedTrainStep(pol, m)
    head = K.HeadLossBackward(m, arch[-1], "cuda", CLIP, ent_coef, VF, normalize)
    rows = None
    if use_rows or adv_ready:
        # the minibatch as a random m-subset of a 3m-row rollout buffer
        g = torch.Generator().manual_seed(m)
        total = 3 * m
        idx = torch.randperm(total, generator=g)[:m]
        big = [torch.randn(total, t.shape[1], generator=g).cuda() for t in (obs, act, aux)]
        for b, t in zip(big, (obs, act, aux)):
            b[idx.cuda()] = t
        idx32 = idx.to(torch.int32).cuda()
        if use_rows:
            obs, act, aux = big
            rows = idx32
        else:
            obs, act, aux = (torch.empty_like(t) for t in (obs, act, aux))
            K.gather_minibatch(idx32, *big, obs, act, aux, adv_part=head.adv_part)
    grad, stats = fs.step(obs, act, aux, head, rows=rows, adv_ready=adv_ready,
                          defer_finish=defer)
    if defer:
        # the deferred reductions, with a clip factor and an update of exactly
        # nothing (c = 1, lr = 0): the buffer holds the gradient itself
        opt = K.ClipAdam(pol.flat.detach(), lr=0.0, max_grad_norm=1e30)
        opt.step_finish(grad, fs.finish)
    torch.cuda.synchronize()
    out = {}
    for name, _, _ in pol.layout:
        a, b, shape = pol.offsets[name]
        out[_sb3_name(name, len(arch))] = grad[a:b].view(shape).detach().cpu().double()
    # the step allocates the observation image only where it takes the fused kernel
    fused_first = getattr(fs, "_ximg", None) is not None
    return out, stats.detach().cpu().double(), fused_first


@pytest.mark.parametrize("name,cfg,defer,use_rows,adv_ready,ent_coef,normalize", CASES,
                         ids=[c[0] for c in CASES])
def test_fused_step_matches_f64_within_fp32_bounds(monkeypatch, name, cfg, defer, use_rows,
                                                   adv_ready, ent_coef, normalize):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    obs_dim, arch, m = cfg
    g_ref, env, env_act, st_ref = _reference(cfg, ent_coef, normalize)
    g_gpu, st, fused_first = _run(cfg, defer, use_rows, adv_ready, ent_coef, normalize)
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n = step_chain_lengths(obs_dim, arch, m, fused_first=fused_first, n_cu=n_cu)
    bound = grad_bound(env, env_act, n)
    ratios = {}
    for k in g_ref:
        err = (g_gpu[k].reshape(g_ref[k].shape) - g_ref[k]).abs()
        ratios[k] = (err / (bound[k] + 1e-30)).max().item()
    gs = gamma(stats_chain_length(m))
    sratios = {}
    for i, key in ((0, "loss"), (1, "policy_loss"), (2, "value_loss"), (3, "entropy_loss"),
                   (5, "approx_kl")):
        v, e = st_ref[key]
        sratios[key] = abs(st[i].item() - v) / (gs * e)
    count = st_ref["clip_count"]
    print(f"{name}: fused first layer {fused_first}, n {sorted(set(n.values()))}, "
          f"stats n {stats_chain_length(m)}")
    print(f"{name}: worst gradient error / bound {max(ratios.values()):.4f} "
          f"({max(ratios, key=ratios.get)}), worst stat error / bound "
          f"{max(sratios.values()):.4f} ({max(sratios, key=sratios.get)}), "
          f"clip count {round(st[4].item() * m)} / {count} of {m}")
    # the path the case is listed for: only the trainer's default takes the fused kernel
    assert fused_first == (cfg == A and defer and not use_rows)
    for k, r in ratios.items():
        assert r <= 1.0, f"{name} {k}: gradient error {r:.3f} x its fp32 bound"
    for k, r in sratios.items():
        assert r <= 1.0, f"{name} {k}: error {r:.3f} x its fp32 bound"
    assert 0.2 * m <= count <= 0.7 * m           # the clip is engaged (the fixture's property)
    assert round(st[4].item() * m) == count
    assert abs(st[4].item() - count / m) <= 3 * 2.0 ** -24 * count / m
