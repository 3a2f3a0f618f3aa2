"""The rollout-side policy forward against f64 on every network path.

PolicyInference.__call__ -> hidden_forward -> dr_linear_tanh2 /
dr_linear_tanh2_x6 -> dr_gemm_x6 or torch.bmm / addmm -> dr_policy_heads
decides which actions are flown, which values and log-probs enter GAE and
what scripts/eval_policy.py reports, and runs code the training step never
executes (policy_heads_kernel, preact=False at depth 1, the middle layers'
addmm + tanh_, the x6 image refresh outside FusedTrainStep).  The training
forward has its f64 checks in test_ppo_step_f64_gpu.py; this file is the
rollout side's.

Fixtures (ppo_f64.inference_fixture): weights scaled and perturbed so that
every bias, the heads' and the top layer's included, is non-zero and the
outputs have rms 0.5-2; observations 1.5 randn with row 0 all zeros and row 1
all 50.0 (the position limit, the first layer saturated).

Two tiers (ppo_f64.check_inference), both against the f64 forward:

  hard   every mean / value entry within forward_bound64's running fp32
         bound (valid for every summation order; the x6 GEMM counts as an
         fp32 dot) + one fp32 ulp of the reference for the final store.  A
         plain fp32 forward reaches 0.0001-0.075 of it: a no-false-alarm guard.
  sharp  n >= 64: the rms over all 5 n outputs of |gpu - f64| is at most 4 x
         the rms of a plain CPU fp32 restatement's error on the same fixture
         (forward32_cpu); n < 64: every entry's error at most 4 x that
         restatement's largest error on the same policy's 256-row fixture.
         The 4 is established on the CPU alone
         (test_policy_forward_bound_cpu.py: a forward whose every tanh is off
         by +-6 ulp stays within 1.5-2.6 x rms, 1.2-3.0 x max; one bf16 plane
         instead of three, a dropped head or top-layer bias, a lane mask one
         lane short fail it by 250 x - 9e6 x).

Cases (ppo_f64.INFERENCE_CASES), each the smallest size that reaches its path:

  x6_fused_images  15, (256, 256), n 128 / 384   dr_linear_tanh2_x6 builds the
                                                 weight images; dr_gemm_x6
  x6_refresh       19, (256, 256), n 256         dr_linear_tanh2 +
                                                 X6Weights.refresh + dr_gemm_x6
  library_ragged   15, (256, 256), n 1000        no multiple of 128: torch.bmm
  one_env          15, (64, 64),   n 1           the reference's one-env config
  unequal          18, (64, 128),  n 257         hd = 128: half the lanes masked
  depth1           12, (128,),     n 255         preact off: tanh in linear_tanh
  depth3           16, (64,64,64), n 300         middle addmm + tanh_ over acts2
  narrow_head      32, (256, 252), n 100         lane 63 inactive in the heads
  tiny             4,  (4,),       n 7           one active lane
  width_8 / _24    8 / 24, (64, 64), n 65        linear_tanh_kernel<8>, <24>
  second_round     15, (64, 64),   n 2053        policy_heads' grid-stride loop:
                                                 ceil(2053 / 16) = 129 blocks x
                                                 4 rows, three full rounds of
                                                 516 rows and a ragged fourth
                                                 (505 rows: the last block has
                                                 one row, two blocks none)
  saturated        15, (256, 256), n 384, scale 4  many pre-activations past the
                                                 tanh clamp (x6 path)

Further: ActorCritic.forward on the GPU (the unfused trainer's rollout path)
under the same two tiers; parameters changed between two calls (a stale x6
weight image would fail); rows poisoned with +inf / -inf / NaN (the other rows
bitwise unchanged); dr_policy_heads alone against f64; the trainer's values /
logp buffers after collect_rollouts, eager and on the replayed rollout graph;
and the first epoch's ratio on the paths test_ppo_gpu.py does not cover.

Poisoned rows.  A NaN observation entry must come out NaN in both nets'
outputs (the tanh clamp propagates NaN, common.h).  An infinite entry must
NOT: every first-layer pre-activation of that row is +-inf, tanh(+-inf) = +-1,
and the f64 forward of that row is finite -- so those two rows are held to
their f64 values (within 4 x the plain restatement's largest error), which
asks more than "non-finite" would.

dr_policy_heads alone.  Bound per output, t = tanh in f64 of the inputs as
given (of z + zb with zb): gamma(hd + 2) (|t| |W|^T + |b|) + 2 TANH_ULP u
|t| |W|^T.  The fp32 rounding of z + zb moves tanh by at most u |z + zb| (1 -
t^2) <= u |t| (x (1 - tanh^2 x) <= tanh x), inside the 1.3 ulp that TANH_ULP =
6 leaves above the device tanh's measured worst (4.7 ulp).

First epoch's ratio.  With one epoch of one minibatch approx_kl and
clip_fraction are exactly 0 wherever the rollout and the training forward run
only this project's kernels (first layer, dr_gemm_x6, heads: depth 1, and
(256, 256) with N and M multiples of 128 at any observation width).  Where a
library GEMM runs at two row counts (N rows in the rollout, M in training)
bitwise equality is the library's to give; the test records what it measures
and asserts clip_fraction == 0 and approx_kl <= the value the hard bound on
logp implies: with L = 2 dlogp per row (rollout and training log-prob each
within dlogp of f64), mean(L^2 e^L / 2 + 4 u e^L) -- the second term for
expf's result near 1 (2 ulp of 2 u each), which is what dominates.

Measured on an MI355X (rms_gpu / rms_ref, or for n < 64 the largest error /
the restatement's largest over 256 rows; worst error / hard bound):

    x6_fused_images n 128            0.603   0.00021
    x6_fused_images n 384            0.591   0.00021
    x6_refresh                       0.607   0.00018
    library_ragged                   0.986   0.00021
    one_env (zero row / generic)     0.071 / 0.197 (max)   0.00157
    unequal                          0.981   0.00099
    depth1                           0.773   0.00445
    depth3                           1.035   0.00015
    narrow_head                      1.122   0.00012
    tiny                             0.440 (max)           0.07457
    width_8 / width_24               1.068 / 1.175         0.00269
    second_round                     1.078   0.00157
    saturated                        0.622   0.00013
    unfused depth3 / library_ragged  1.133 / 1.175         0.00030
    after a parameter update         0.579 (fused images), 0.556 (refresh); the
                                     outputs moved by 1.9e5 x the sharp tolerance
    infinite rows                    0.22-0.44 of the restatement's largest error
    dr_policy_heads alone            worst 0.26 of its bound (hd 4), 0.026 at hd
                                     64, 0.003 at hd 252 / 256
    trainer values / logp            0.00015 / 0.00036 eager, 0.00011 / 0.00017
                                     on the replayed graph
    first epoch                      approx_kl = 0 and clip_fraction = 0 exactly
                                     in all four configurations, the two with
                                     library GEMMs at 8 and 64 rows included
                                     (bound 2.4e-7)

No case is above 4; the worst is 1.18.  The project's kernels sit BELOW the
plain restatement on the x6 paths because their fmaf chains and the x6 GEMM
round less often than an fp32 GEMM does.  With the value net's top-layer bias
skipped in policy_heads_kernel every depth >= 2 case of the fused forward and
every preact_zb case of the heads test fails; with the heads' lane mask one
lane short (c0 + 4 < hd) all 14 forward cases and all 36 heads cases fail;
with X6Weights.refresh skipped x6_refresh fails, and with it run once and
then skipped the second call of the parameter-update test fails (316,000 x
the reference's rms).
"""
import functools

import pytest
import torch

from ppo_f64 import (INFERENCE_CASES, SHARP, SMALL_REF_ROWS, TANH_ULP, U, check_inference,
                     forward64, forward_bound64, gamma, inference_case, inference_reference,
                     logp64)

pytestmark = pytest.mark.gpu

KNOBS = ("DRONERL_X6_FUSED_IMAGES", "DRONERL_GEMM_X6", "DRONERL_X6_FL", "DRONERL_X6_FL_DIRECT",
         "DRONERL_HEAD_DIRECT", "DRONERL_FL_FIRST", "DRONERL_DEFER_FINISH",
         "DRONERL_ROLLOUT_GRAPH", "DRONERL_TRAIN_GRAPH", "DRONERL_PPO_OVERLAP",
         "DRONERL_TUNED_GEMMS")
BY_ID = {c[0]: c for c in INFERENCE_CASES}
IDS = [c[0] for c in INFERENCE_CASES]
# which 256 x 256 path a case takes: the images built by the first layer's
# launch, by X6Weights.refresh, or no x6 GEMM at all
X6_FUSED = {"x6_fused_images_128", "x6_fused_images_384", "saturated"}
X6_REFRESH = {"x6_refresh"}


@pytest.fixture(autouse=True)
def _default_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)


def _fixture(case_id):
    _, obs_dim, arch, n, scale = BY_ID[case_id]
    return inference_case(obs_dim, arch, n, scale)


def _policy(fx):
    from drone_rl_amd.policy import ActorCritic
    pol = ActorCritic(fx["obs"].shape[1], 4, fx["arch"], seed=0, device="cuda")
    pol.load_state_dict(fx["sd"])
    return pol


def _count_x6(monkeypatch):
    """Counts of the two ways the x6 weight images get built."""
    from drone_rl_amd import policy as P
    from drone_rl_amd import ppo_kernels as K
    calls = {"fused": 0, "refresh": 0, "gemm": 0}

    def wrap(obj, name, key):
        real = getattr(obj, name)

        def f(*a, **kw):
            calls[key] += 1
            return real(*a, **kw)
        monkeypatch.setattr(obj, name, f)

    wrap(K, "linear_tanh2_x6", "fused")
    wrap(P.X6Weights, "refresh", "refresh")
    wrap(P, "gemm_x6", "gemm")
    return calls


def _infer(pol, obs):
    """(mean, value) of PolicyInference on obs, as host copies."""
    from drone_rl_amd.policy import PolicyInference
    inf = PolicyInference(pol, obs.shape[0])
    mean, value = inf(obs.cuda().contiguous())
    torch.cuda.synchronize()
    return mean.cpu().clone(), value.cpu().clone()


def _assert_two_tiers(name, ref, mean, value, rows=None):
    got = check_inference(ref, mean, value, rows)
    kind = "max_gpu / max_ref(256 rows)" if "small_max" in ref else "rms_gpu / rms_ref"
    print(f"{name}: {kind} {got['sharp']:.3f}, worst error / hard bound {got['hard']:.5f}")
    assert got["hard_ok"], f"{name}: error {got['hard']:.3g} x its fp32 bound"
    assert got["sharp_ok"], f"{name}: {kind} = {got['sharp']:.3g} > {SHARP}"
    return got


@pytest.mark.parametrize("case_id", IDS)
def test_policy_inference_matches_f64(monkeypatch, case_id):
    fx = _fixture(case_id)
    calls = _count_x6(monkeypatch)
    pol = _policy(fx)
    mean, value = _infer(pol, fx["obs"])
    # the path the case is listed for
    assert calls == {"fused": int(case_id in X6_FUSED), "refresh": int(case_id in X6_REFRESH),
                     "gemm": int(case_id in X6_FUSED | X6_REFRESH)}, calls
    _assert_two_tiers(case_id, fx, mean, value)
    if fx["n"] == 1:
        # the fixture's row 0 is the zero observation, which the first
        # layer's weights do not enter: also one generic row on its own
        obs = inference_case(*BY_ID[case_id][1:3], SMALL_REF_ROWS, BY_ID[case_id][4])["obs"][2:3]
        ref = inference_reference(fx["sd"], fx["arch"], obs)
        ref["small_max"] = fx["small_max"]
        _assert_two_tiers(case_id + " generic row", ref, *_infer(pol, obs))


@pytest.mark.parametrize("case_id", ["depth3", "library_ragged"])
def test_unfused_forward_matches_f64(case_id):
    """ActorCritic.forward on the GPU: what the trainer's rollout calls when
    the architecture does not fit the fused kernels."""
    fx = _fixture(case_id)
    pol = _policy(fx)
    with torch.no_grad():
        mean, value = pol(fx["obs"].cuda())
    _assert_two_tiers(case_id + " unfused", fx, mean.cpu(), value.cpu())


@pytest.mark.parametrize("case_id", ["x6_fused_images_128", "x6_refresh"])
def test_parameters_changed_between_calls(case_id):
    """The x6 weight images are rebuilt on every call: after an in-place
    parameter update the second result is right for the NEW parameters."""
    from drone_rl_amd.policy import PolicyInference
    fx = _fixture(case_id)
    pol = _policy(fx)
    obs = fx["obs"].cuda()
    inf = PolicyInference(pol, obs.shape[0])
    first = [t.cpu().clone() for t in inf(obs)]
    _assert_two_tiers(case_id + " first call", fx, *first)
    g = torch.Generator().manual_seed(2)
    pol.flat.data.add_((0.01 * torch.randn(pol.num_params, generator=g)).cuda())
    second = [t.cpu().clone() for t in inf(obs)]
    ref = inference_reference(pol.state_dict(), fx["arch"], fx["obs"])
    _assert_two_tiers(case_id + " second call", ref, *second)
    moved = torch.cat([(second[0] - first[0]).double(),
                       (second[1] - first[1]).double()[:, None]], 1).pow(2).mean().sqrt().item()
    tol = SHARP * ref["ref_rms"]
    print(f"{case_id}: outputs moved by rms {moved:.3e} = {moved / tol:.3g} x the sharp tolerance")
    assert moved > 100 * tol


POISON = {"x6_fused_images_384": (70, 200, 383), "unequal": (3, 130, 256),
          "second_round": (17, 1029, 2052), "library_ragged": (5, 500, 999)}


@pytest.mark.parametrize("case_id", list(POISON))
def test_poisoned_rows_stay_in_their_rows(case_id):
    """+inf, -inf and NaN written into one entry of three rows (different
    waves / tiles, the last row among them): every other row bitwise
    unchanged -- on the library GEMM path: within the sharp tier, the library
    promises no bits -- the NaN row NaN in both nets' outputs, the two
    infinite rows at their (finite) f64 values."""
    fx = _fixture(case_id)
    pol = _policy(fx)
    n = fx["n"]
    clean = _infer(pol, fx["obs"])
    obs = fx["obs"].clone()
    r_pinf, r_ninf, r_nan = POISON[case_id]
    assert r_nan == n - 1
    obs[r_pinf, 3], obs[r_ninf, 2], obs[r_nan, 1] = float("inf"), float("-inf"), float("nan")
    mean, value = _infer(pol, obs)
    others = torch.ones(n, dtype=torch.bool)
    others[list(POISON[case_id])] = False
    if case_id == "library_ragged":
        _assert_two_tiers(case_id + " other rows", fx, mean, value, rows=others)
    else:
        assert torch.equal(mean[others], clean[0][others])
        assert torch.equal(value[others], clean[1][others])
    assert torch.isnan(mean[r_nan]).all() and torch.isnan(value[r_nan])
    inf_rows = [r_pinf, r_ninf]
    mean64, value64 = forward64(fx["sd"], fx["arch"], obs[inf_rows])
    assert torch.isfinite(mean64).all() and torch.isfinite(value64).all()
    err = max((mean[inf_rows].double() - mean64).abs().max().item(),
              (value[inf_rows].double() - value64).abs().max().item())
    print(f"{case_id}: infinite rows' error {err:.3e} = {err / fx['ref_max']:.3f} x max_ref")
    assert torch.isfinite(mean[inf_rows]).all() and torch.isfinite(value[inf_rows]).all()
    assert err <= SHARP * fx["ref_max"]


# ------------------------------------------------------ dr_policy_heads alone
@functools.lru_cache(maxsize=None)
def _head_inputs(hd):
    """Inputs for the head kernel at the largest m (smaller m: the first
    rows: row 0 generic, so m = 1 is no trivial case), |z| up to 12 with a
    row of +-12 and a row of zeros."""
    g = torch.Generator().manual_seed(100 + hd)
    m = 2053
    z = (4.0 * torch.randn(2, m, hd, generator=g)).clamp(-12.0, 12.0)
    z[:, 1, ::2], z[:, 1, 1::2] = 12.0, -12.0
    z[:, 2] = 0.0
    zb = 0.5 * torch.randn(2, hd, generator=g)
    w_act, w_val = 0.5 * torch.randn(4, hd, generator=g), 0.5 * torch.randn(1, hd, generator=g)
    b_act, b_val = torch.randn(4, generator=g), torch.randn(1, generator=g)
    return z, zb, w_act, b_act, w_val, b_val


@pytest.mark.parametrize("mode", ["activations", "preact", "preact_zb"])
@pytest.mark.parametrize("m", [1, 5, 2053])
@pytest.mark.parametrize("hd", [4, 64, 252, 256])
def test_policy_heads_alone_match_f64(hd, m, mode):
    from drone_rl_amd import ppo_kernels as K
    z, zb, w_act, b_act, w_val, b_val = _head_inputs(hd)
    z = z[:, :m].contiguous()
    if mode == "activations":
        x = torch.tanh(z.double()).float()         # the kernel's input: h itself
        t = x.double()
    else:
        x = z
        t = torch.tanh(z.double() + (zb.double()[:, None] if mode == "preact_zb" else 0.0))
    mean = torch.full((m, 4), float("nan"), device="cuda")
    value = torch.full((m,), float("nan"), device="cuda")
    xd = x.cuda()
    kw = dict(zb_pi=zb[0].cuda(), zb_vf=zb[1].cuda()) if mode == "preact_zb" else {}
    K.policy_heads(xd[0], xd[1], w_act.cuda(), b_act.cuda(), w_val.cuda(), b_val.cuda(),
                   mean, value, preact=mode != "activations", **kw)
    torch.cuda.synchronize()
    worst = 0.0
    for got, tt, W, b in ((mean.cpu().double(), t[0], w_act, b_act),
                          (value.cpu().double()[:, None], t[1], w_val, b_val)):
        ref = tt @ W.double().T + b.double()
        env = tt.abs() @ W.double().abs().T
        bound = gamma(hd + 2) * (env + b.double().abs()) + 2 * TANH_ULP * U * env
        err = (got - ref).abs()
        assert torch.isfinite(got).all()
        worst = max(worst, (err / bound).max().item())
    print(f"policy_heads hd {hd} m {m} {mode}: worst error / bound {worst:.4f}")
    assert worst <= 1.0


# -------------------------------------------------------- the trainer's buffers
def _logp_bound(mean64, dmean, log_std, act):
    """(logp64, bound): |fl(logp) - logp64| <= sum_j |z_j| dmean_j / sigma_j
    (the mean's error through d (a - mu)^2 / 2 sigma^2) + gamma(16) sum_j
    (z_j^2 / 2 + |log sigma_j| + 0.919) (the row's own roundings: expf, the
    square, the reciprocal, logf, the sums)."""
    ls = log_std.double()
    z = (act.double() - mean64) / ls.exp()
    bound = (z.abs() * dmean / ls.exp()).sum(1) + \
        gamma(16) * (0.5 * z ** 2 + ls.abs() + 0.919).sum(1)
    return logp64(mean64, log_std, act), bound


def _check_buffers(tr, sd, arch, tag):
    T, N = tr.cfg.n_steps, tr.cfg.num_envs
    obs = tr.obs[:T].reshape(T * N, -1).cpu()
    mean64, dmean, value64, dvalue = forward_bound64(sd, arch, obs)
    verr = (tr.values.reshape(-1).cpu().double() - value64).abs() / dvalue
    lp64, dlp = _logp_bound(mean64, dmean, sd["log_std"], tr.actions.reshape(T * N, 4).cpu())
    lerr = (tr.logp.reshape(-1).cpu().double() - lp64).abs() / dlp
    print(f"trainer buffers ({tag}): values error / bound {verr.max().item():.5f}, "
          f"logp error / bound {lerr.max().item():.5f}")
    assert verr.max().item() <= 1.0 and lerr.max().item() <= 1.0
    return dlp


def test_trainer_rollout_buffers_match_f64():
    """values[t] and logp[t] of collect_rollouts are those of obs[t] and
    actions[t] under the f64 forward, on the eager first call and on the
    replayed rollout graph (the third call)."""
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    fx = _fixture("x6_fused_images_128")
    tr = PPOTrainer(PPOConfig(num_envs=128, n_steps=4, batch_size=512, n_epochs=1, seed=5))
    tr.policy.load_state_dict(fx["sd"])
    sd = tr.policy.state_dict()
    assert all(torch.equal(sd[k], fx["sd"][k]) for k in sd)
    tr.collect_rollouts()
    _check_buffers(tr, sd, fx["arch"], "eager")
    tr.collect_rollouts()
    tr.collect_rollouts()
    assert tr._rgraph is not None
    _check_buffers(tr, sd, fx["arch"], "replayed graph")
    tr.close()


# ------------------------------------------------- the first epoch's ratio
# (id, PPOConfig fields, only this project's kernels between obs and logp)
FIRST_EPOCH = [
    ("two_by_64_8_envs", dict(net_arch=(64, 64), num_envs=8, n_steps=8), False),
    ("depth1", dict(net_arch=(128,), num_envs=8, n_steps=8), True),
    ("depth3", dict(net_arch=(64, 64, 64), num_envs=8, n_steps=8), False),
    ("width_19_x6", dict(net_arch=(256, 256), num_envs=128, n_steps=2, variant="smooth"), True),
]


@pytest.mark.parametrize("name,kw,own_kernels", FIRST_EPOCH, ids=[c[0] for c in FIRST_EPOCH])
def test_first_epoch_ratio(name, kw, own_kernels):
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    cfg = PPOConfig(batch_size=kw["num_envs"] * kw["n_steps"], n_epochs=1, seed=6, **kw)
    tr = PPOTrainer(cfg)
    assert tr.use_fused
    tr.collect_rollouts()
    T, N = cfg.n_steps, cfg.num_envs
    sd = tr.policy.state_dict()
    obs = tr.obs[:T].reshape(T * N, -1).cpu()
    act = tr.actions.reshape(T * N, 4).cpu()
    st = tr.train().tolist()
    tr.close()
    clip_fraction, approx_kl = st[4], st[5]
    mean64, dmean, _, _ = forward_bound64(sd, cfg.net_arch, obs)
    _, dlp = _logp_bound(mean64, dmean, sd["log_std"], act)
    L = 2 * dlp
    kl_bound = (0.5 * L ** 2 * L.exp() + 4 * U * L.exp()).mean().item()
    print(f"first epoch {name}: approx_kl {approx_kl:.3e} (bound {kl_bound:.3e}), "
          f"clip_fraction {clip_fraction}")
    assert clip_fraction == 0.0
    if own_kernels:
        assert approx_kl == 0.0
    else:
        assert abs(approx_kl) <= kl_bound
