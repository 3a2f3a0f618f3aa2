"""The network's tanh (common.h tanh_rat / tanh_rat2) measured on the device
against f64 tanh.  ppo_f64.TANH_ULP, the budget the f64 parity bounds give
it, came from a numpy simulation with an exact quotient; the device divides
with v_rcp_f32.

Two call sites can be driven as an elementwise tanh with exact plumbing:

* dr_linear_tanh with k = n = 4, W = I, b = 0: column j's chain is
  fma(x_k, 0, acc) = acc for k != j (finite x_k) and fma(x_j, 1, +0) = x_j,
  then x_j + 0, so h[r, j] = tanh_rat2(x[r, j]).
* dr_policy_heads with preact, hd = 4, W_act = I, b_act = 0: mean[r, j] =
  tanh4(z)[j] * 1 + zeros, summed over lanes that hold zeros.

Both start their accumulator at +0, so -0 comes out as +0 before the tanh
sees it: the sign of a zero is not observable through either call site, and
+-0 is asserted to give a zero.  inf * 0 is NaN, so an inf (or NaN) sits in
column 0 of a row of zeros and only that column is read.

Sweep: 2^20 log-spaced magnitudes in [2^-126, 16) with both signs, every f32
within 2^10 ulp of 0.55 (where the two-form evaluation switches) and of the
clamp 7.9053111, 2^12 subnormals.

Measured on an MI355X: worst 4.703 ulp (at x = 6.7361155; 4.219 below |x| =
0.55), inside TANH_ULP = 6; the two call sites agree on every input.  Before
the polynomials carried their common factor 2^8 (common.h kTanhScale) the
product x P(x^2) underflowed to a subnormal for |x| < 2.4e-36 and 50,492 of
the sweep's inputs in [2^-126, 3.8e-37] missed the budget, by up to 103 ulp
(an absolute error below 2e-43).  The scaling changed no result bit outside
|x| <= 2.4e-36 (compared over this sweep on the device).
"""
import numpy as np
import pytest
import torch

from ppo_f64 import TANH_ULP

pytestmark = pytest.mark.gpu

CLAMP = np.float32(7.90531110763549805)


def _neighbours(x, k):
    """Every f32 within k ulp of x."""
    b = np.array([x], np.float32).view(np.int32)[0]
    return np.arange(b - k, b + k + 1, dtype=np.int32).view(np.float32)


def _inputs():
    mag = np.exp2(np.linspace(-126.0, 4.0, 1 << 20, endpoint=False)).astype(np.float32)
    mag = np.concatenate([mag, _neighbours(0.55, 1 << 10), _neighbours(CLAMP, 1 << 10)])
    sub = np.linspace(1, (1 << 23) - 1, 1 << 12).astype(np.int32).view(np.float32)
    x = np.concatenate([mag, -mag, sub, -sub])
    x = np.concatenate([x, np.ones(-len(x) % 4, np.float32)]).reshape(-1, 4)
    special = np.zeros((6, 4), np.float32)
    special[1, :] = -0.0
    special[2, 0], special[3, 0], special[4, 0] = np.inf, -np.inf, np.nan
    return np.concatenate([x, special]), len(x)


def _via_linear_tanh(x):
    from drone_rl_amd import ppo_kernels as K
    out = torch.full_like(x, float("nan"))
    K.linear_tanh(x, torch.eye(4, device="cuda"), torch.zeros(4, device="cuda"), out)
    return out


def _via_policy_heads(x):
    from drone_rl_amd import ppo_kernels as K
    m = x.shape[0]
    mean = torch.full_like(x, float("nan"))
    value = torch.empty(m, device="cuda")
    z4 = torch.zeros(4, device="cuda")
    K.policy_heads(x, torch.zeros_like(x), torch.eye(4, device="cuda"), z4,
                   torch.zeros(1, 4, device="cuda"), torch.zeros(1, device="cuda"), mean, value,
                   preact=True)
    assert (value == 0).all()
    return mean


def test_network_tanh_within_its_ulp_budget_on_the_device():
    xs, n_sweep = _inputs()
    x = torch.from_numpy(xs).cuda()
    a = _via_linear_tanh(x).cpu().numpy()
    b = _via_policy_heads(x).cpu().numpy()
    torch.cuda.synchronize()
    # the two call sites agree bitwise (sweep: every column; specials: as
    # read): the bit patterns of every non-zero result are equal and the zero
    # results fall on the same inputs -- the sign of a zero result (the
    # smallest subnormal inputs) is the plumbing's: both call sites add the
    # tanh to an accumulator that starts at +0
    def same_bits(p, q):
        nz = p != 0
        return (np.array_equal(nz, q != 0) and
                np.array_equal(p.view(np.int32)[nz], q.view(np.int32)[nz]))
    assert same_bits(a[:n_sweep], b[:n_sweep])
    sp_a, sp_b = a[n_sweep:], b[n_sweep:]
    assert same_bits(sp_a[:4, 0], sp_b[:4, 0])
    # specials: zeros give zeros, +-inf the clamp's value (1 - <= 3 ulp), NaN stays NaN
    assert (sp_a[0] == 0).all() and (sp_a[1] == 0).all()
    assert (sp_b[0] == 0).all() and (sp_b[1] == 0).all()
    ulp1 = float(np.spacing(np.float32(1.0)))            # tanh(7.9053) = 1 - 2.26 ulp
    for sp in (sp_a, sp_b):
        assert 0 <= 1.0 - float(sp[2, 0]) <= 3 * ulp1
        assert 0 <= 1.0 + float(sp[3, 0]) <= 3 * ulp1
        assert np.isnan(sp[4, 0])
        assert (sp[5] == 0).all()
    xv, h = xs[:n_sweep].ravel(), a[:n_sweep].ravel()
    assert np.isfinite(h).all()
    assert (np.abs(h) <= 1.0).all()                     # 1 - h^2 never negative
    assert ((h == 0) | (np.sign(h) == np.sign(xv))).all()
    ref = np.tanh(xv.astype(np.float64))
    cr = ref.astype(np.float32)                          # the correctly rounded result
    normal = np.abs(cr) >= np.float32(2.0 ** -126)
    ulp = np.spacing(np.abs(cr[normal])).astype(np.float64)
    err = np.abs(h[normal].astype(np.float64) - ref[normal]) / ulp
    k = int(np.argmax(err))
    print(f"worst tanh error {err.max():.3f} ulp at x = {xv[normal][k]!r} "
          f"(budget TANH_ULP = {TANH_ULP}); |x| < 0.55: {err[np.abs(xv[normal]) < 0.55].max():.3f}, "
          f"above: {err[np.abs(xv[normal]) >= 0.55].max():.3f}")
    assert err.max() <= TANH_ULP, f"{err.max():.3f} ulp at x = {xv[normal][k]!r}"
