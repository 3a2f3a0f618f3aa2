"""The yardsticks of tests/test_policy_inference_f64_gpu.py, established on
the CPU from the reference alone (ppo_f64: forward_bound64, forward32_cpu,
inference_fixture, check_inference), on the very fixtures the GPU test uses
(ppo_f64.INFERENCE_CASES).

(a) Hard bound.  The plain fp32 restatement lies within forward_bound64's
    per-entry bound on every fixture; it reaches 0.0001-0.011 of it (0.075
    on the (4,) net, whose sums are too short to cancel), so the bound is a
    no-false-alarm guard, not the sharp check.

(b) The sharp check's margin.  A forward whose every tanh result is off by a
    uniform draw in +-6 ulp (TANH_ULP: above the device tanh's measured worst
    of 4.7 ulp) has an rms error against f64 of at most 4 x the plain
    restatement's, and a largest error of at most 4 x.  Measured over the
    fixtures: rms ratio 1.55-2.60, max ratio 1.17-2.96.  Hence SHARP = 4:
    the margin comes from this simulation, not from any GPU result.

(c) The checks reject wrong results.  On every fixture each of
      * the layer-1 operands rounded to bf16 (one bf16 plane instead of
        three; layer 1 is the head at depth 1),
      * value_net.bias dropped,
      * the top hidden layer's biases dropped,
      * the last four hidden columns zeroed (a lane mask one lane short)
    fails check_inference's sharp tier: the bf16 layer at 8,200-16,100 x the
    plain rms (250 x the 256-row maximum on the one-row fixture), the others
    at 1.5e4-9e6 x.  The hard bound is loose by design (a worst case over
    rounding signs and summation orders), so a defect need not fail it: the
    test prints how many do per defect and asserts nothing about that.  Here
    the bias and column defects fail the hard bound on all 14 fixtures, the
    bf16 layer on 13 (0.97 of the bound on the (256, 252) net).
"""
import pytest
import torch

from ppo_f64 import (INFERENCE_CASES, SHARP, check_inference, forward32_cpu, inference_case)

IDS = [c[0] for c in INFERENCE_CASES]


def _case(c):
    _, obs_dim, arch, n, scale = c
    return inference_case(obs_dim, arch, n, scale)


@pytest.mark.parametrize("case", INFERENCE_CASES, ids=IDS)
def test_plain_fp32_forward_within_hard_bound(case):
    fx = _case(case)
    print(f"{case[0]}: plain fp32 error / hard bound {fx['ref_hard']:.4f}, "
          f"rms {fx['ref_rms']:.3e}, max {fx['ref_max']:.3e}")
    assert fx["ref_hard"] <= 1.0
    got = check_inference(fx, *forward32_cpu(fx["sd"], fx["arch"], fx["obs"]))
    assert got["hard_ok"] and got["sharp_ok"]
    # the fixture's properties: zero row, saturating row, no zero bias
    assert not fx["obs"][0].any()
    assert case[3] < 3 or (fx["obs"][1] == 50.0).all()
    assert all(v.abs().min() > 0 for k, v in fx["sd"].items() if k.endswith("bias"))


@pytest.mark.parametrize("case", [c for c in INFERENCE_CASES if c[3] >= 64],
                         ids=[c[0] for c in INFERENCE_CASES if c[3] >= 64])
def test_six_ulp_tanh_stays_within_the_sharp_margin(case):
    """(b): rms and largest error with every tanh off by up to TANH_ULP ulp,
    against the plain restatement's."""
    from ppo_f64 import TANH_ULP, _errors
    fx = _case(case)
    g = torch.Generator().manual_seed(1)
    out = forward32_cpu(fx["sd"], fx["arch"], fx["obs"], tanh_ulps=TANH_ULP, generator=g)
    err = _errors(*out, fx["mean64"], fx["value64"])
    rms = err.pow(2).mean().sqrt().item() / fx["ref_rms"]
    mx = err.max().item() / fx["ref_max"]
    print(f"{case[0]}: 6-ulp tanh rms ratio {rms:.2f}, max ratio {mx:.2f}")
    assert rms <= SHARP and mx <= SHARP
    assert check_inference(fx, *out)["hard_ok"]


def _defects(fx):
    """name -> (mean, value) of four wrong forwards of the fixture."""
    sd, arch, obs = fx["sd"], fx["arch"], fx["obs"]
    top = 2 * (len(arch) - 1)

    def edited(fn):
        e = {k: v.clone() for k, v in sd.items()}
        fn(e)
        return forward32_cpu(e, arch, obs)

    def no_top_bias(e):
        e[f"mlp_extractor.policy_net.{top}.bias"].zero_()
        e[f"mlp_extractor.value_net.{top}.bias"].zero_()

    def short_mask(e):          # hidden columns the heads never see
        e["action_net.weight"][:, -4:] = 0
        e["value_net.weight"][:, -4:] = 0

    return {"bf16_layer_1": forward32_cpu(sd, arch, obs, bf16_layer=1),
            "value_bias_dropped": edited(lambda e: e["value_net.bias"].zero_()),
            "top_bias_dropped": edited(no_top_bias),
            "last_four_columns_zeroed": edited(short_mask)}


def test_defects_fail_the_sharp_check():
    """(c): every defect fails the sharp tier on every fixture; how many also
    fail the hard bound is printed, not asserted (the hard bound is loose)."""
    hard_fails = {}
    for case in INFERENCE_CASES:
        fx = _case(case)
        for name, out in _defects(fx).items():
            got = check_inference(fx, *out)
            print(f"{case[0]} {name}: sharp ratio {got['sharp']:.3g}, "
                  f"error / hard bound {got['hard']:.3g}")
            assert not got["sharp_ok"], (case[0], name, got)
            hard_fails[name] = hard_fails.get(name, 0) + (not got["hard_ok"])
    for name, k in hard_fails.items():
        print(f"{name}: fails the hard bound on {k} of {len(INFERENCE_CASES)} fixtures")
