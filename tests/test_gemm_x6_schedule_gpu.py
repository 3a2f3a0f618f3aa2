"""The x6 GEMM kernels (csrc/gemm_x6.hip) at every pipeline depth and on every
row: gemm_x6_ws16_kernel (dr_gemm_x6), gemm_x6_wgrad16_kernel
(dr_gemm_x6_wgrad) and gemm_x6_fl16_kernel (dr_gemm_x6_bwd_first).

A block's code path is set by R, the number of 32-row steps it owns (the
prologue branches on R > 1 and R > 2; the staging clamps engage in the last
three steps), and by G_, the 32-row stages of a weight-gradient chunk.  The
shapes are derived from the device's CU count (tests/x6_cases.py) so that the
launches have the R sets {1}, {2,1}, {2}, {3,2}, {3}, {4,3}, {5,4}, {6} and
G_ = 1, 2, 3, 4, and three kinds of check run on them:

  * exact: integer operands whose every partial sum is exact in f32 in any
    order (envelope sum |a b| <= 2^22 units, the three dropped plane products
    identically zero) -- the kernel must return the f64 GEMM bit for bit, on
    every row, column, chunk and per-block partial row;
  * accuracy: the project's criteria (e6 <= e32, e6 < 4e-7 relative to
    sum |a b|; the Higham bound of the fused kernel with the chain length of
    the shape) over all rows and chunks of random operands;
  * the split on designed values, and the containment of non-finite inputs.
"""
import math

import numpy as np
import pytest
import torch

import x6_cases as X
from drone_rl_amd import _lib
from drone_rl_amd._lib import check, ptr

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
W_IMG = 3 * 256 * 256 * 2


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _shape(batch, rs):
    """The smallest m whose launch has the R set `rs` on this device; the
    plan is asserted, never trusted."""
    n_cu = _n_cu()
    m = X.smallest_m(rs, n_cu, batch)
    assert X.r_set(m, n_cu, batch) == tuple(rs)
    if batch == 2:
        assert X.blocks_per_net(m, n_cu, 2) == _lib.lib().dr_gemm_x6_bwd_first_rows(m)
    return m


def _image(W, transpose):
    L = _lib.lib()
    nb = L.dr_gemm_x6_weights_bytes(W.shape[0])
    assert nb == W.shape[0] * W_IMG
    img = torch.zeros(nb * (2 if transpose == 2 else 1), dtype=torch.uint8, device="cuda")
    check(L.dr_gemm_x6_split_weights(W.shape[0], ptr(W), transpose, ptr(img), _stream()))
    return img


def _gemm(A, img):
    C = torch.full((A.shape[0], A.shape[1], 256), float("nan"), device="cuda")
    check(_lib.lib().dr_gemm_x6(A.shape[0], A.shape[1], ptr(A), ptr(img), ptr(C), _stream()))
    torch.cuda.synchronize()
    return C


def _wgrad(G, H, chunks):
    ws = torch.full((G.shape[0], chunks, 256, 256), float("nan"), device="cuda")
    check(_lib.lib().dr_gemm_x6_wgrad(G.shape[0], G.shape[1], chunks, ptr(G), ptr(H), ptr(ws),
                                      _stream()))
    torch.cuda.synchronize()
    return ws


def test_plan_reaches_every_row_step_set_on_this_device():
    n_cu = _n_cu()
    for batch in (2, 1):
        got = X.plan(n_cu, batch)
        assert [rs for rs, _ in got] == list(X.R_SETS if batch == 2 else X.R_SETS_ONE_NET)
        for rs, m in got:
            assert m % 128 == 0 and X.r_set(m, n_cu, batch) == rs
            if batch == 2:
                assert X.blocks_per_net(m, n_cu, 2) == _lib.lib().dr_gemm_x6_bwd_first_rows(m)
    if n_cu == 256:
        assert [m for _, m in X.plan(256, 2)] == [128, 4224, 8192, 8320, 12288, 12416, 16512,
                                                  24576]


def test_exact_families_use_the_six_kept_products_and_no_dropped_one():
    seen = set()
    for fam in X.FAMILIES:
        A = X.exact_A(fam, 2, 256, 1, "cuda")
        W = X.exact_W(fam, 2, 1, "cuda")
        G, H = X.exact_GH(fam, 2, 256, 1, "cuda")
        for a, bt in ((A, W), (A, W.transpose(1, 2)), (G.transpose(1, 2), H.transpose(1, 2))):
            got = X.plane_products(a, bt)
            assert not got & set(X.DROPPED), (fam, got)
            seen |= got
    assert seen == set(X.KEPT), seen


# ---------------------------------------------------------------------------
# exact: dr_gemm_x6
_FWD_CASES = [(2, rs) for rs in X.R_SETS] + [(1, rs) for rs in X.R_SETS_ONE_NET]


@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("batch,rs", _FWD_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_x6_is_exact_on_every_row(batch, rs, family):
    """All four image forms (transpose 0, 1 and the two halves of a
    transpose-2 image) against the f64 GEMM of the same integers: equal on
    every row and column.  A stale or duplicated row step, a swapped plane
    buffer, a wrong column tile or a missing plane product changes a value."""
    m = _shape(batch, rs)
    A = X.exact_A(family, batch, m, 10 * len(rs) + rs[0], "cuda")
    W = X.exact_W(family, batch, rs[0], "cuda")
    assert not X.plane_products(A, W) & set(X.DROPPED)
    assert not X.plane_products(A, W.transpose(1, 2)) & set(X.DROPPED)
    A64, W64 = A.double(), W.double()
    ref = {0: torch.bmm(A64, W64.transpose(1, 2)), 1: torch.bmm(A64, W64)}
    for t, Bt in ((0, W64), (1, W64.transpose(1, 2))):
        env = torch.bmm(A64.abs(), Bt.abs().transpose(1, 2)).max().item()
        assert 0 < env <= X.ENVELOPE, (t, env)
    img2 = _image(W, 2)
    # a transpose-2 image: the transpose-0 form (z = h W^T) first, then transpose 1
    forms = ((0, _image(W, 0)), (1, _image(W, 1)), (0, img2[:batch * W_IMG]),
             (1, img2[batch * W_IMG:]))
    assert torch.equal(forms[0][1], forms[2][1]) and torch.equal(forms[1][1], forms[3][1])
    for i, (t, img) in enumerate(forms):
        C = _gemm(A, img).double()
        bad = (C != ref[t]).nonzero()
        assert bad.numel() == 0, (i, t, len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------
# exact: dr_gemm_x6_wgrad, every chunk
@pytest.mark.parametrize("family", X.FAMILIES)
@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("m,chunks", [(32, 1), (192, 3), (480, 5), (128, 1), (2048, 16)])
def test_wgrad_is_exact_in_every_chunk(m, chunks, batch, family):
    """G_ = (m / chunks) / 32 = 1, 2, 3, 4 stages per chunk (the loads'
    clamps differ at 1, 2 and >= 3), odd chunk counts, one and two nets."""
    rows = m // chunks
    assert rows // 32 == {32: 1, 192: 2, 480: 3, 128: 4, 2048: 4}[m]
    G, H = X.exact_GH(family, batch, m, m + chunks, "cuda")
    Gc = G.double().view(batch, chunks, rows, 256)
    Hc = H.double().view(batch, chunks, rows, 256)
    ref = torch.einsum("bcrn,bcrk->bcnk", Gc, Hc)
    env = torch.einsum("bcrn,bcrk->bcnk", Gc.abs(), Hc.abs()).max().item()
    assert 0 < env <= X.ENVELOPE, env
    ws = _wgrad(G, H, chunks).double()
    bad = (ws != ref).nonzero()
    assert bad.numel() == 0, (len(bad), bad[:4].tolist())


# ---------------------------------------------------------------------------
# dr_gemm_x6_bwd_first
def _bwd_first_runs(gz, W, h, x):
    """-> (per-block partial rows (per, 2, 16, 256) of direct = 1, the total
    of direct = 0, the total of the unfused path), f64, and the group count."""
    L = _lib.lib()
    m = gz.shape[1]
    s = _stream()
    img = _image(W, 1)                                              # C = A W
    ximg = torch.zeros(L.dr_gemm_x6_x_bytes(m), dtype=torch.uint8, device="cuda")
    check(L.dr_gemm_x6_split_x(m, 15, ptr(x), ptr(ximg), s))
    wsb = L.dr_first_layer_backward2_workspace_bytes(m, 15, 256)
    ws = [torch.zeros(wsb, dtype=torch.uint8, device="cuda") for _ in range(3)]
    for direct in (1, 0):
        check(L.dr_gemm_x6_bwd_first(2, m, 15, ptr(gz), ptr(img), ptr(h), ptr(ximg),
                                     ptr(ws[1 - direct]), wsb, direct, s))
    gh = _gemm(gz, img)
    dw = torch.zeros(2, 256, 15, device="cuda")
    db = torch.zeros(2, 256, device="cuda")
    check(L.dr_first_layer_backward2(m, 15, 256, ptr(x), None, ptr(gh[0]), ptr(h[0]), ptr(dw[0]),
                                     ptr(db[0]), ptr(gh[1]), ptr(h[1]), ptr(dw[1]), ptr(db[1]),
                                     1, ptr(ws[2]), wsb, s))
    torch.cuda.synchronize()
    per = L.dr_gemm_x6_bwd_first_rows(m)
    rows = ws[0].view(torch.float32)[:per * 2 * 16 * 256].double().view(per, 2, 16, 256)
    fused, unfused = X.level1_groups(ws[1], m), X.level1_groups(ws[2], m)
    return rows, fused.sum(0), unfused.sum(0), fused.shape[0]


def _bwd_first_ref(gz, W, h, x, per):
    """f64: the per-block partial rows (block j0 of a net owns the row steps
    j0, j0 + per, ...) and their envelopes, (per, 2, 16, 256) each."""
    m = gz.shape[1]
    steps = m // 32
    r_max = -(-steps // per)
    gz64, W64, h64 = gz.double(), W.double(), h.double()
    d = 1 - h64 * h64
    xe = torch.cat([x.double(), torch.ones(m, 1, dtype=torch.float64, device=x.device)], 1)
    out = []
    for g1 in (torch.bmm(gz64, W64) * d, torch.bmm(gz64.abs(), W64.abs()) * d.abs()):
        xa = xe if not out else xe.abs()
        g1p = torch.zeros(2, r_max * per * 32, 256, dtype=torch.float64, device=x.device)
        g1p[:, :m] = g1
        xp = torch.zeros(r_max * per * 32, 16, dtype=torch.float64, device=x.device)
        xp[:m] = xa
        out.append(torch.einsum("bkjrn,kjrf->jbfn", g1p.view(2, r_max, per, 32, 256),
                                xp.view(r_max, per, 32, 16)))
    return out


@pytest.mark.parametrize("family", ["gz_wide", "w_wide"])
@pytest.mark.parametrize("rs", X.R_SETS, ids=lambda v: str(v).replace(" ", ""))
def test_bwd_first_is_exact_per_block_and_in_total(rs, family):
    """direct = 1: the partial row of block (j0, net) is exactly the f64 sum
    over THAT block's row steps; direct = 0 and the unfused path (dr_gemm_x6 +
    dr_first_layer_backward2) give exactly the whole-minibatch total.  All
    values lie on the grid of 1/4 (1 - h^2 in {1, 0.75, 0})."""
    m = _shape(2, rs)
    per = X.blocks_per_net(m, _n_cu(), 2)
    gz, W, h, x = X.exact_bwd_first(family, m, rs[0] + len(rs), "cuda")
    ref, env = _bwd_first_ref(gz, W, h, x, per)
    assert torch.equal(ref * 4, (ref * 4).round())
    assert 0 < 4 * env.sum(0).max().item() <= X.ENVELOPE
    assert 0 < torch.bmm(gz.double().abs(), W.double().abs()).max().item() <= X.ENVELOPE
    rows, fused, unfused, _ = _bwd_first_runs(gz, W, h, x)
    bad = (rows != ref).nonzero()
    assert bad.numel() == 0, ("direct", len(bad), bad[:4].tolist())
    total = ref.sum(0)
    assert torch.count_nonzero(total).item() > total.numel() // 4
    assert torch.equal(fused, total), "direct = 0"
    assert torch.equal(unfused, total), "unfused"


# ---------------------------------------------------------------------------
# accuracy against f64 on every row and chunk
def _errors(C, A, Wt):
    ref = torch.bmm(A.double(), Wt.double())
    den = torch.bmm(A.abs().double(), Wt.abs().double()).clamp_min(1e-30)
    r32 = torch.bmm(A, Wt)
    return (((C.double() - ref).abs() / den).max().item(),
            ((r32.double() - ref).abs() / den).max().item())


_ACC_CASES = [((3, 2), 0), ((3, 2), 1), ((4, 3), 0), ((4, 3), 1), ((5, 4), 0), ((5, 4), 1),
              (65536, 0)]


@pytest.mark.parametrize("rs,transpose", _ACC_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_gemm_x6_as_accurate_as_fp32_on_all_rows(rs, transpose):
    m = rs if isinstance(rs, int) else _shape(2, rs)
    g = torch.Generator().manual_seed(m + transpose)
    A = torch.tanh(torch.randn(2, m, 256, generator=g)).cuda()
    W = (torch.randn(2, 256, 256, generator=g) * (2 / 256) ** 0.5).cuda()
    C = _gemm(A, _image(W, transpose))
    e6, e32 = _errors(C, A, W if transpose else W.transpose(1, 2))
    print(f"x6 forward m={m} transpose={transpose}: e6={e6:.3e} e32={e32:.3e}")
    assert e6 <= e32, (e6, e32)
    assert e6 < 4e-7


@pytest.mark.parametrize("m,chunks", [(192, 3), (480, 5), (3072, 4), (65536, 64)])
def test_wgrad_as_accurate_as_fp32_in_all_chunks(m, chunks):
    g = torch.Generator().manual_seed(m)
    G = (torch.randn(2, m, 256, generator=g) * 1e-3).cuda()
    H = torch.tanh(torch.randn(2, m, 256, generator=g)).cuda()
    ws = _wgrad(G, H, chunks)
    rows = m // chunks
    Gt = G.view(2 * chunks, rows, 256).transpose(1, 2)
    Hc = H.view(2 * chunks, rows, 256)
    e6, e32 = _errors(ws.view(2 * chunks, 256, 256), Gt, Hc)
    print(f"x6 wgrad m={m} chunks={chunks}: e6={e6:.3e} e32={e32:.3e}")
    assert e6 <= e32, (e6, e32)
    assert e6 < 4e-7


@pytest.mark.parametrize("rs", [(3, 2), (4, 3)], ids=lambda v: str(v).replace(" ", ""))
def test_bwd_first_within_the_bound_of_its_own_chain(rs):
    """Against f64 within Higham's gamma_n sum |terms| with n the chain length
    of this shape: the 256-term dot product and the add of its two
    accumulators (257), the three dropped plane products of each x6 GEMM
    (<= 2^-23 = 2 u of |a b| together: + 2 each), the three elementwise
    roundings of grad_z1, the rows a block sums (32 R), and the blocks a
    level-1 group sums.  direct = 1 is
    held per block (no group sum); the unfused path by the rows of one
    level-1 group in any order.  The figures are printed for DESIGN.md."""
    m = _shape(2, rs)
    per = X.blocks_per_net(m, _n_cu(), 2)
    g = torch.Generator().manual_seed(7 + m)
    gz = (torch.randn(2, m, 256, generator=g) * 1e-3).cuda()
    W = (torch.randn(2, 256, 256, generator=g) * 0.06).cuda()
    h = torch.tanh(torch.randn(2, m, 256, generator=g) * 1.5).cuda()
    x = (torch.randn(m, 15, generator=g) * 2).cuda()
    ref, env = _bwd_first_ref(gz, W, h, x, per)
    rows, fused, unfused, ng = _bwd_first_runs(gz, W, h, x)
    gam = lambda n: n * U / (1 - n * U)
    n_block = 257 + 2 + 3 + 32 * rs[0] + 2
    n_fused = n_block + -(-per // ng)
    n_unfused = 257 + 2 + 3 + -(-m // ng)
    tiny = 1e-30
    ratios = {
        "direct": (((rows - ref).abs() / env.clamp_min(tiny)).max().item(), gam(n_block)),
        "fused": (((fused - ref.sum(0)).abs() / env.sum(0).clamp_min(tiny)).max().item(),
                  gam(n_fused)),
        "unfused": (((unfused - ref.sum(0)).abs() / env.sum(0).clamp_min(tiny)).max().item(),
                    gam(n_unfused)),
    }
    for name, (err, bound) in ratios.items():
        print(f"x6 bwd_first m={m} {name}: err/env={err:.3e} bound={bound:.3e} "
              f"ratio={err / bound:.2e}")
    for name, (err, bound) in ratios.items():
        assert err <= bound, (name, err, bound)


# ---------------------------------------------------------------------------
# the split on designed values
def _check_planes(planes_u16, x_f32, exact_mask, what):
    """planes (3, ...) uint16 against the f32 values x.  Every plane is
    bitwise the IEEE host split (RNE with gradual underflow, no flush): where
    `exact_mask` that follows from RNE alone; elsewhere an intermediate is
    denormal and it is the device's measured behaviour under the library's
    build flags (x6_split.h), held here so that a flag or mode change that
    flushes fails.  Then h + m + l == x in f64 wherever three bf16 can hold x
    (all of `exact_mask`), and the loss is at most 2^-134, half the smallest
    bf16 denormal, elsewhere.  Returns the largest loss."""
    val = sum(X.bf16_bits_to_f32(planes_u16[p]).astype(np.float64) for p in range(3))
    x64 = x_f32.astype(np.float64)
    host = X.split3_bits(x_f32)
    for p in range(3):
        bad = np.argwhere(planes_u16[p] != host[p])
        assert len(bad) == 0, (what, "plane", p, len(bad), bad[:4].tolist(),
                               "in the denormal class" if not exact_mask[tuple(bad[0])] else "")
    assert np.array_equal(val[exact_mask], x64[exact_mask]), what
    host_val = sum(X.bf16_bits_to_f32(host[p]).astype(np.float64) for p in range(3))
    holds = host_val == x64
    assert holds[exact_mask].all()
    assert np.array_equal(val[holds], x64[holds]), what
    loss = np.abs(val - x64)
    assert loss.max() <= 2.0 ** -134, (what, loss.max())
    return loss.max()


def _corpus_matrix(n, seed):
    """n f32 values: the spread groups (8-aligned), then the corpus tiled in
    a seed-dependent rotation -> (values, mask of the derivable ones)."""
    exact, edge = X.split_corpus()
    st = X.corpus_stats(exact)
    assert min(st["tie1"], st["tie2_down"], st["tie2_up"], st["neg_rem"]) > 1000, st
    assert st["l_nonzero"] > 5000 and len(edge) > 200
    pats = np.concatenate([exact, edge])
    ok = np.concatenate([np.ones(len(exact), bool), np.zeros(len(edge), bool)])
    spread = X.spread_groups(64).reshape(-1)
    assert n >= len(spread) + len(pats)
    idx = (np.arange(n - len(spread)) + seed * 977) % len(pats)
    vals = np.concatenate([spread, pats[idx].view(np.float32)])
    return vals, np.concatenate([np.ones(len(spread), bool), ok[idx]])


@pytest.mark.parametrize("batch", [1, 2])
@pytest.mark.parametrize("transpose", [0, 1, 2])
def test_weight_image_is_the_exact_split_at_the_documented_place(transpose, batch):
    vals, ok = _corpus_matrix(batch * 65536, transpose + 3 * batch)
    W = torch.from_numpy(vals).view(batch, 256, 256).cuda()
    img = _image(W, transpose).cpu().numpy()
    Wn, okn = vals.reshape(batch, 256, 256), ok.reshape(batch, 256, 256)
    forms = {0: [(0, False)], 1: [(0, True)], 2: [(0, False), (1, True)]}[transpose]
    for half, tr in forms:
        planes = X.decode_weight_image(img[half * batch * W_IMG:(half + 1) * batch * W_IMG], batch)
        Bt = Wn.transpose(0, 2, 1) if tr else Wn
        mk = okn.transpose(0, 2, 1) if tr else okn
        loss = _check_planes(planes.transpose(1, 0, 2, 3), np.ascontiguousarray(Bt),
                             np.ascontiguousarray(mk), ("weights", transpose, half))
        print(f"x6 split weights transpose={transpose} half={half} batch={batch}: "
              f"largest loss {loss:.3e}")


def test_observation_image_is_the_exact_split_at_the_documented_place():
    L = _lib.lib()
    n = 512 + sum(len(c) for c in X.split_corpus())
    m = -(-n // (15 * 128)) * 128                      # the corpus once, whole
    vals, ok = _corpus_matrix(m * 15, 1)
    x = torch.from_numpy(vals).view(m, 15).cuda()
    img = torch.zeros(L.dr_gemm_x6_x_bytes(m), dtype=torch.uint8, device="cuda")
    check(L.dr_gemm_x6_split_x(m, 15, ptr(x), ptr(img), _stream()))
    torch.cuda.synchronize()
    planes = X.decode_x_image(img.cpu().numpy(), m)
    xe = np.concatenate([vals.reshape(m, 15), np.ones((m, 1), np.float32)], 1)
    mk = np.concatenate([ok.reshape(m, 15), np.ones((m, 1), bool)], 1)
    loss = _check_planes(planes, xe, mk, "observations")
    print(f"x6 split x (m = {m}): largest loss {loss:.3e}")


def test_gemm_of_designed_values_in_one_group_is_as_accurate_as_fp32():
    """Magnitudes spread over 2^+-60 inside every 8-value group of A and W:
    the in-kernel split (staging, v_cvt_pk_bf16_f32 pieces) keeps fp32
    accuracy where the planes' exponents differ by more than bf16's 8 bits."""
    m = 256
    A = torch.from_numpy(X.spread_groups(2 * m * 32).reshape(2, m, 256) * 2.0 ** -30).cuda()
    W = torch.from_numpy(X.spread_groups(2 * 256 * 32).reshape(2, 256, 256) * 2.0 ** -30).cuda()
    C = _gemm(A, _image(W, 0))
    e6, e32 = _errors(C, A, W.transpose(1, 2))
    print(f"x6 forward spread groups: e6={e6:.3e} e32={e32:.3e}")
    assert math.isfinite(e6) and e6 <= e32, (e6, e32)
    assert e6 < 4e-7


# ---------------------------------------------------------------------------
# non-finite containment
def test_non_finite_inputs_stay_in_their_row_column_and_chunk():
    m = _shape(2, (3, 2))
    per = X.blocks_per_net(m, _n_cu(), 2)
    g = torch.Generator().manual_seed(5)
    A = torch.tanh(torch.randn(2, m, 256, generator=g)).cuda()
    W = (torch.randn(2, 256, 256, generator=g) * 0.09).cuda()
    # an inf in iteration k = 1 of block 1 (net 0), a NaN in k = 2 of block 0 (net 1)
    r_inf, r_nan = (1 + per) * 32 + 5, 2 * per * 32 + 27
    assert r_nan < m
    bad = A.clone()
    bad[0, r_inf, 77] = float("inf")
    bad[1, r_nan, 200] = float("nan")
    zeroed = A.clone()
    zeroed[0, r_inf, 77] = 0.0
    zeroed[1, r_nan, 200] = 0.0
    img = _image(W, 0)
    Cb, Cz = _gemm(bad, img), _gemm(zeroed, img)
    assert not torch.isfinite(Cb[0, r_inf]).any() and not torch.isfinite(Cb[1, r_nan]).any()
    keep = torch.ones(2, m, dtype=torch.bool, device="cuda")
    keep[0, r_inf] = keep[1, r_nan] = False
    assert torch.isfinite(Cz).all()
    assert torch.equal(Cb[keep].view(torch.int32), Cz[keep].view(torch.int32))
    # one non-finite weight: its output column of its net only
    Wb = W.clone()
    Wb[1, 130, 9] = float("inf")
    Wz = W.clone()
    Wz[1, 130, 9] = 0.0
    Cb, Cz = _gemm(A, _image(Wb, 0)), _gemm(A, _image(Wz, 0))
    assert not torch.isfinite(Cb[1, :, 130]).any()
    keep = torch.ones(2, m, 256, dtype=torch.bool, device="cuda")
    keep[1, :, 130] = False
    assert torch.equal(Cb[keep].view(torch.int32), Cz[keep].view(torch.int32))
    # a NaN weight through the transpose-1 image (C = A W): column n of W
    Wb, Wz = W.clone(), W.clone()
    Wb[0, 201, 64] = float("nan")
    Wz[0, 201, 64] = 0.0
    Cb, Cz = _gemm(A, _image(Wb, 1)), _gemm(A, _image(Wz, 1))
    assert torch.isnan(Cb[0, :, 64]).all()
    keep = torch.ones(2, m, 256, dtype=torch.bool, device="cuda")
    keep[0, :, 64] = False
    assert torch.isfinite(Cz).all()
    assert torch.equal(Cb[keep].view(torch.int32), Cz[keep].view(torch.int32))
    # the weight gradient: only output row n of the chunk that holds the bad row
    chunks = 5
    mw = 480
    G = (torch.randn(2, mw, 256, generator=g) * 1e-3).cuda()
    H = torch.tanh(torch.randn(2, mw, 256, generator=g)).cuda()
    for value, (b, row, n) in ((float("inf"), (0, 96 + 70, 31)), (float("nan"), (1, 4 * 96 + 95, 255))):
        Gb, Gz = G.clone(), G.clone()
        Gb[b, row, n] = value
        Gz[b, row, n] = 0.0
        wb, wz = _wgrad(Gb, H, chunks), _wgrad(Gz, H, chunks)
        c = row // (mw // chunks)
        assert not torch.isfinite(wb[b, c, n]).any()
        keep = torch.ones(2, chunks, 256, dtype=torch.bool, device="cuda")
        keep[b, c, n] = False
        assert torch.isfinite(wz).all()
        assert torch.equal(wb[keep].view(torch.int32), wz[keep].view(torch.int32))
    # a bad entry of H: only output column k of its chunk
    for value, (b, row, k) in ((float("nan"), (0, 2 * 96 + 33, 0)), (float("-inf"), (1, 40, 129))):
        Hb, Hz = H.clone(), H.clone()
        Hb[b, row, k] = value
        Hz[b, row, k] = 0.0
        wb, wz = _wgrad(G, Hb, chunks), _wgrad(G, Hz, chunks)
        c = row // (mw // chunks)
        assert not torch.isfinite(wb[b, c, :, k]).any()
        keep = torch.ones(2, chunks, 256, 256, dtype=torch.bool, device="cuda")
        keep[b, c, :, k] = False
        assert torch.isfinite(wz).all()
        assert torch.equal(wb[keep].view(torch.int32), wz[keep].view(torch.int32))
