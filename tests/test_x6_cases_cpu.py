"""The host-side pieces of tests/test_gemm_x6_schedule_gpu.py (tests/x6_cases.py)
checked without a GPU: the shape plan on a 256-CU device, the host split, the
image decoders' index maps and the exactness conditions of the integer
operand families."""
import numpy as np
import pytest
import torch

import x6_cases as X


def test_plan_on_256_cus():
    assert [m for _, m in X.plan(256, 2)] == [128, 4224, 8192, 8320, 12288, 12416, 16512, 24576]
    assert [m for _, m in X.plan(256, 1)] == [128, 8320, 24576, 24704]
    # the shapes the suite had before: R = 1, 1, 1, 2, 16 only
    assert [X.r_set(m, 256, 2) for m in (128, 256, 384, 8192, 65536)] == \
        [(1,), (1,), (1,), (2,), (16,)]
    # other devices get their own shapes; a set a device cannot produce (m / 32
    # is a multiple of 4, so 3 x 7 steps never occur) is an error, not a lost case
    for n_cu in (304, 80, 64):
        for batch in (1, 2):
            for rs, m in X.plan(n_cu, batch):
                assert X.r_set(m, n_cu, batch) == rs and m % 128 == 0
    with pytest.raises(AssertionError):
        X.plan(7, 1)


def test_host_split_is_exact_and_rounds_to_nearest_even():
    exact, edge = X.split_corpus()
    # the corpus holds what it names, in numbers: ties of the first rounding
    # and of the second (m's last bit even and odd), remainders that reach the
    # l plane, all-ones carries with negative remainders
    st = X.corpus_stats(exact)
    assert min(st["tie1"], st["tie2_down"], st["tie2_up"], st["neg_rem"]) > 1000, st
    assert st["l_nonzero"] > 5000 and len(exact) > 15000 and len(edge) > 200
    se = X.corpus_stats(edge)
    assert se["tie2_down"] > 20 and se["tie2_up"] > 20, se
    # a second-level tie by hand: 1 + 2^-9 + 2^-17 -> h = 1, m = 2^-9 (even), l = 2^-17
    hb, mb, lb = X.split3_bits(np.array([0x3F804040], np.uint32).view(np.float32))
    assert (hb[0], mb[0], lb[0]) == (0x3F80, 0x3B00, 0x3700)
    assert X.corpus_stats(np.array([0x3F804040, 0x3F8040C0], np.uint32)) == \
        {"tie1": 0, "tie2_down": 1, "tie2_up": 1, "l_nonzero": 2, "neg_rem": 0}
    # in the denormal class the IEEE split loses at most half a bf16 denormal
    xe = edge.view(np.float32)
    ve = sum(X.bf16_bits_to_f32(p).astype(np.float64) for p in X.split3_bits(xe))
    assert np.abs(ve - xe.astype(np.float64)).max() == 2.0 ** -134
    x = exact.view(np.float32)
    h, m, l = (X.bf16_bits_to_f32(p).astype(np.float64) for p in X.split3_bits(x))
    assert np.array_equal(h + m + l, x.astype(np.float64))
    assert np.all(np.isfinite(h))
    # ties to even, the carry of an all-ones mantissa, the largest finite h
    one = lambda b: X.bf16_rne_bits(np.array([b], np.uint32).view(np.float32))[0]
    assert one(0x3F808000) == 0x3F80 and one(0x3F818000) == 0x3F82
    assert one(0x3FFFFFFF) == 0x4000 and one(0x7F7F7FFF) == 0x7F7F and one(0x7F7F8000) == 0x7F80
    # torch's conversion is the same rounding
    t = torch.from_numpy(x.copy())
    for p, q in zip(X.split3(t), X.split3_bits(x)):
        assert np.array_equal(p.numpy(), X.bf16_bits_to_f32(q))
    # all-ones mantissas leave a negative remainder, denormals are in the edge class
    hb, mb, _ = X.split3_bits(np.array([0x3FFFFFFF], np.uint32).view(np.float32))
    assert hb[0] == 0x4000 and mb[0] & 0x8000
    assert np.uint32(0x00000001) in edge and np.uint32(0x00800001) in edge
    assert np.uint32(0x7F7F7FFF) in exact and np.uint32(0x80000000) in exact


def test_image_index_maps_are_bijections():
    idx = np.concatenate([X.wimg_index().reshape(-1) + 512 * p for p in range(3)])
    assert np.array_equal(np.sort(idx), np.arange(3 * 256 * 256))
    m = 128
    img = np.arange(m // 32 * 3072 // 2, dtype=np.uint16).view(np.uint8)
    dec = X.decode_x_image(img, m)
    assert np.array_equal(np.sort(dec.reshape(-1)), np.arange(m // 32 * 1536))


def test_families_meet_the_exactness_conditions():
    seen = set()
    for fam in X.FAMILIES:
        A = X.exact_A(fam, 2, 512, 3, "cpu")
        W = X.exact_W(fam, 2, 3, "cpu")
        G, H = X.exact_GH(fam, 2, 480, 3, "cpu")
        assert torch.equal(A, A.round()) and torch.equal(W, W.round())
        # rows differ: a stale or duplicated row step cannot go unnoticed
        assert len(torch.unique(A.view(-1, 256), dim=0)) == 1024
        for t in (W, W.transpose(1, 2)):
            env = torch.bmm(A.double().abs(), t.double().abs().transpose(1, 2)).max().item()
            assert 0 < env <= X.ENVELOPE
            got = X.plane_products(A, t)
            assert not got & set(X.DROPPED)
            seen |= got
        Gc, Hc = G.double().view(2, 5, 96, 256), H.double().view(2, 5, 96, 256)
        env = torch.einsum("bcrn,bcrk->bcnk", Gc.abs(), Hc.abs())
        assert 0 < env.max().item() <= X.ENVELOPE
        # every 32-row stage of every chunk contributes to every output
        st = torch.einsum("bsrn,bsrk->bsnk", G.double().abs().view(2, 15, 32, 256),
                          H.double().abs().view(2, 15, 32, 256))
        assert (st > 0).float().mean().item() > 0.5
        assert not X.plane_products(G.transpose(1, 2), H.transpose(1, 2)) & set(X.DROPPED)
    assert seen == set(X.KEPT)


def test_bwd_first_operands_are_exact_on_the_quarter_grid():
    for fam in ("gz_wide", "w_wide"):
        for m in (128, 4224, 24576):
            gz, W, h, x = X.exact_bwd_first(fam, m, 2, "cpu")
            d = 1 - h.double() ** 2
            assert set(torch.unique(d).tolist()) <= {0.0, 0.75, 1.0}
            if m > 4224:
                continue
            env = torch.bmm(gz.double().abs(), W.double().abs()) * d
            xe = torch.cat([x.double().abs(), torch.ones(m, 1, dtype=torch.float64)], 1)
            tot = torch.einsum("bmn,mf->bfn", env, xe)
            assert 0 < 4 * tot.max().item() <= X.ENVELOPE
            # every row step reaches every column of the bias row
            per_step = env.view(2, m // 32, 32, 256).sum(2)
            assert (per_step > 0).float().mean().item() > 0.9
