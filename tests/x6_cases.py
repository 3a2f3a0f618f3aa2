"""Shared pieces of tests/test_gemm_x6_schedule_gpu.py (and their CPU checks in
tests/test_x6_cases_cpu.py): the shape plan that reaches every pipeline depth
of the x6 GEMM kernels (csrc/gemm_x6.hip), a host-side three-plane bf16 split,
the decoders of the operand images (csrc/x6_split.h) and the integer operand
families whose GEMM is exact in any summation order.

The families (all integers; envelope sum |a b| <= 2^22):
  a_wide      A: 8 nonzeros per row (one per k32 step), odd 18-bit; W: -2 .. 2
  w_wide      the mirror image: A -2 .. 2, W 8 nonzeros per row and column
  both_10bit  A: 4 nonzeros per row, |a| < 2^10; W dense, |w| < 2^10
The wide values have 18 bits, not 17: the RNE split's signed remainders carry
one bit each, so h + m already hold 17 bits and a 17-bit integer never
reaches the l plane.  8 x 2^18 x 2 = 2^22 keeps the envelope.

A block of gemm_x6_ws16_kernel / gemm_x6_fl16_kernel owns the 32-row steps
j0, j0 + per, ... of its net: R = ceil((m / 32 - j0) / per) of them, with
per = (min(batch m / 32, CUs) rounded down to a multiple of batch) / batch.
Its prologue branches on R > 1 and R > 2, and the clamps of its loop engage in
the last three steps, so the code path of a launch is its set of R values."""
import numpy as np
import torch

RS = 32                    # rows per row step
ENVELOPE = 2.0 ** 22       # sum |a b| of an exact case, in units of its grid

# the R sets the plan must reach, in the order of their smallest m
R_SETS = ((1,), (2, 1), (2,), (3, 2), (3,), (4, 3), (5, 4), (6,))
R_SETS_ONE_NET = ((1,), (2, 1), (3,), (4, 3))


def blocks_per_net(m, n_cu, batch):
    units = batch * (m // RS)
    grid = min(units, n_cu)
    grid -= grid % batch
    return grid // batch


def r_set(m, n_cu, batch):
    """The distinct row-step counts of the blocks of one launch, descending."""
    per = blocks_per_net(m, n_cu, batch)
    steps = m // RS
    return tuple(sorted({(steps - j0 + per - 1) // per for j0 in range(per)}, reverse=True))


def smallest_m(want, n_cu, batch):
    """The smallest legal m (a multiple of 128) whose launch has exactly the
    R set `want`; an R set the device cannot produce is an error, not a
    dropped case."""
    want = tuple(sorted(want, reverse=True))
    top = (want[0] + 1) * RS * max(n_cu // batch, 1) + 128
    for m in range(128, top + 1, 128):
        if r_set(m, n_cu, batch) == want:
            return m
    raise AssertionError(f"no m gives the row-step set {want} on {n_cu} CUs, batch {batch}")


def plan(n_cu, batch):
    return [(rs, smallest_m(rs, n_cu, batch)) for rs in (R_SETS if batch == 2 else R_SETS_ONE_NET)]


# ---------------------------------------------------------------------------
# host-side split: bit-level round-to-nearest-even to bf16 with gradual
# underflow (IEEE), every subtraction in f32
def bf16_rne_bits(x):
    """f32 array (finite) -> uint16 bf16 bit patterns, RNE."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_bits_to_f32(b):
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def split3_bits(x):
    """(h, m, l) bf16 bit patterns of the x6 split of the f32 array x."""
    x = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(all="ignore"):
        h = bf16_rne_bits(x)
        r = (x - bf16_bits_to_f32(h)).astype(np.float32)
        m = bf16_rne_bits(r)
        s = (r - bf16_bits_to_f32(m)).astype(np.float32)
        l = bf16_rne_bits(s)
    return h, m, l


def split3(t):
    """torch f32 tensor -> its three planes as f32 tensors (torch's own RNE
    conversion: the integer families only hold normal values)."""
    h = t.to(torch.bfloat16).float()
    r = t - h
    m = r.to(torch.bfloat16).float()
    l = (r - m).to(torch.bfloat16).float()
    return h, m, l


KEPT = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (1, 1))     # (plane of A, plane of Bt)
DROPPED = ((1, 2), (2, 1), (2, 2))


def plane_products(A, Bt):
    """Which plane products of C = A Bt^T (A (..., m, K), Bt (..., n, K)) are
    nonzero somewhere: a product is nonzero iff some k has a nonzero in both
    planes' k-th columns."""
    pa = [(p != 0).flatten(0, -2).any(0) for p in split3(A)]
    pb = [(p != 0).flatten(0, -2).any(0) for p in split3(Bt)]
    return {(i, j) for i in range(3) for j in range(3) if bool((pa[i] & pb[j]).any())}


# ---------------------------------------------------------------------------
# image decoders (x6_split.h)
def wimg_index():
    """u16 index of element j of plane 0 of Bt[n][8 c + j] in one net's weight
    image, shape (256, 32, 8); plane p is 512 u16 (W_FRAG bytes) further."""
    n = np.arange(256)[:, None]
    k0 = 8 * np.arange(32)[None, :]
    w, ct, c, s, q = n >> 6, (n >> 4) & 3, n & 15, k0 >> 5, (k0 >> 3) & 3
    off = (((w * 4 + ct) * 8 + s) * 3 * 64 + c + 16 * q) * 16      # wimg_off, bytes
    return (off // 2)[:, :, None] + np.arange(8)[None, None, :]


def decode_weight_image(img_u8, batch):
    """bytes of `batch` nets' image -> uint16 planes (batch, 3, 256 n, 256 k)."""
    u16 = np.ascontiguousarray(img_u8).view(np.uint16).reshape(batch, 3 * 256 * 256)
    idx = wimg_index().reshape(256, 256)
    return np.stack([u16[:, idx + 512 * p] for p in range(3)], axis=1)


def decode_x_image(img_u8, m):
    """The observation image -> uint16 planes (3, m, 16 features)."""
    planes = np.ascontiguousarray(img_u8).view(np.uint16).reshape(m // 32, 3, 4, 16, 8)
    e = np.arange(8)
    q = np.arange(4)[:, None]
    rows = np.where(e[None, :] < 4, 4 * q + e[None, :], 16 + 4 * q + e[None, :] - 4)   # (q, e)
    out = np.zeros((3, m // 32, 32, 16), dtype=np.uint16)
    for p in range(3):
        for f in range(16):
            out[p][:, rows, f] = planes[:, p, :, f, :]
    return out.reshape(3, m, 16)


# ---------------------------------------------------------------------------
# designed f32 values of the split tests, as bit patterns
def split_corpus():
    """-> (exact, edge): uint32 bit patterns.  `exact`: x and every
    intermediate of its split (h, x - h, m, (x - h) - m, l) is zero or a normal
    number of its format, so the planes follow from RNE alone.  `edge`: the
    rest of the corpus (f32 denormals, the smallest normals): some
    intermediate is denormal, and what the device does with it is measured."""
    pats = []
    exps = list(range(1, 254))
    ones = [(e << 23) | 0x7FFFFF for e in exps]                       # h rounds up
    ties = [(e << 23) | (k << 16) | 0x8000 for e in exps
            for k in (0, 1, 2, 3, 0x7E, 0x7F)]                         # bf16 ties
    # remainders of exactly 8 bits (bit 7 the last): m holds them, l = 0
    rem8 = [(e << 23) | (k << 16) | (mm << 8) | 0x80 for e in exps[::3]
            for k in (0, 1, 0x7F) for mm in (0x00, 0x01, 0x02, 0x7F, 0x80, 0x81, 0xFE, 0xFF)]
    # ties of the second rounding: the remainder x - h has 9 significant bits,
    # the last one set (top bit t, 7 bits between, bit t - 8), m's last bit
    # even and odd; above 0x8000 h rounds up and the remainder is negative
    low = [(1 << t) | (mid << (t - 7)) | (1 << (t - 8)) for t in (14, 13, 11, 8)
           for mid in (0x00, 0x01, 0x02, 0x55, 0x7E, 0x7F)]
    low += [0x10000 - v for v in low]
    ties2 = [(e << 23) | (k << 16) | v for e in exps[::8] for k in (0, 1, 0x7F) for v in low]
    # full 24-bit mantissas over the whole exponent range
    full = [(exps[i % len(exps)] << 23) | ((i * 2654435761 + 0x5BD1E995) & 0x7FFFFF)
            for i in range(1500)]
    pow2 = [e << 23 for e in range(1, 255)]
    misc = [0x00000000, 0x7F7F7FFF, 0x7F7F0000, 0x7F000000, 0x3F800001, 0x3F808081,
            0x3FFFFFFF, 0x3F7FFFFF, 0x4B7FFFFF, 0x4B800001, 0x3EAAAAAB, 0x40490FDB]
    den = [0x00000001, 0x00000002, 0x00000003, 0x00007FFF, 0x00008000, 0x00008001,
           0x00010000, 0x00018000, 0x00012345, 0x00400000, 0x007FFFFF, 0x007F8000,
           0x00800000, 0x00800001, 0x00808080, 0x00FFFFFF, 0x00FF8000, 0x01000001,
           0x017FFFFF, 0x0A7FFFFF, 0x0B800001]
    pats = np.array(ones + ties + rem8 + ties2 + full + pow2 + misc + den, dtype=np.uint32)
    pats = np.unique(np.concatenate([pats, pats | np.uint32(0x80000000)]))
    x = pats.view(np.float32)
    h, m, l = split3_bits(x)
    with np.errstate(all="ignore"):
        hf, mf = bf16_bits_to_f32(h), bf16_bits_to_f32(m)
        r = (x - hf).astype(np.float32)
        s = (r - mf).astype(np.float32)
    tiny = np.float32(2.0 ** -126)
    ok = np.ones(len(x), dtype=bool)
    for v in (x, hf, r, mf, s, bf16_bits_to_f32(l)):
        ok &= (v == 0) | (np.abs(v) >= tiny)
    # a remainder below bf16's 8 bits would not be exact either
    ok &= (hf.astype(np.float64) + mf.astype(np.float64)
           + bf16_bits_to_f32(l).astype(np.float64)) == x.astype(np.float64)
    return pats[ok], pats[~ok]


def corpus_stats(pats):
    """Counts over bit patterns: ties of the first rounding (x to h), ties of
    the second (x - h to m) with m rounded down / up in magnitude, nonzero l
    planes, negative remainders of a positive x."""
    x = np.ascontiguousarray(pats, dtype=np.uint32).view(np.float32)
    h, m, l = split3_bits(x)
    with np.errstate(all="ignore"):
        r = (x - bf16_bits_to_f32(h)).astype(np.float32)
    rb = r.view(np.uint32)
    tie2 = (r != 0) & ((rb & 0xFFFF) == 0x8000)
    up = tie2 & ((m & 0x7FFF) > ((rb >> 16) & 0x7FFF).astype(np.uint16))
    return {"tie1": int(((pats & 0xFFFF) == 0x8000).sum()), "tie2_down": int((tie2 & ~up).sum()),
            "tie2_up": int(up.sum()), "l_nonzero": int(((l & 0x7FFF) != 0).sum()),
            "neg_rem": int(((x > 0) & (r < 0)).sum())}


def level1_groups(ws, m, nets=2, k=15, n=256):
    """The level-1 groups the first-layer workspace `ws` (a uint8 tensor)
    holds after dr_first_layer_backward2(defer = 1) or dr_gemm_x6_bwd_first
    (direct = 0): f64 (groups, nets, k + 1, n), the bias in feature row k."""
    nb = min(-(-m // 16), 256)
    P = nets * (k + 1) * n
    gsize = -(-nb // 16)
    ng = -(-nb // gsize)
    off = ((4 * nb * P + 255) & ~255) // 4
    return ws.view(torch.float32)[off:off + ng * P].double().view(ng, nets, k + 1, n)


def spread_groups(n_groups):
    """(n_groups, 8) f32: each 8-value group spans 2^-60 .. 2^60 with full
    24-bit mantissas, the order rotated from group to group."""
    exps = np.array([-60, -43, -26, -9, 9, 26, 43, 60])
    out = np.zeros((n_groups, 8), dtype=np.float32)
    for g in range(n_groups):
        mant = 1.0 + ((np.arange(8) * 2654435761 + g * 40503) % (1 << 23)) / float(1 << 23)
        sign = np.where((np.arange(8) + g) & 1, -1.0, 1.0)
        out[g] = (sign * mant * 2.0 ** np.roll(exps, g)).astype(np.float32)
    return out


# ---------------------------------------------------------------------------
# exact integer operands
def mix(rows, cols, seed):
    """A 32-bit hash of (row, column, seed) as int64 tensors (broadcast)."""
    x = (rows * 0x9E3779B1 + cols * 0x85EBCA77 + seed * 0x27D4EB2F + 0x165667B1) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x = x ^ (x >> 12)
    x = (x * 0x297A2D39) & 0xFFFFFFFF
    return x ^ (x >> 15)


def _signed(h, mag):
    return torch.where((h >> 31) & 1 == 1, -mag, mag)


def _odd18(h):
    return _signed(h, ((h >> 4) & 0x1FFFF) | 0x20001)         # odd, 2^17 < |v| < 2^18


def _small(h):
    return (h % 5) - 2                                         # -2 .. 2


def _int10(h):
    return _signed(h, (h >> 3) & 0x3FF)                        # |v| < 2^10


def _grid(n_rows, n_cols, dev):
    r = torch.arange(n_rows, device=dev, dtype=torch.int64)[:, None]
    c = torch.arange(n_cols, device=dev, dtype=torch.int64)[None, :]
    return r, c


FAMILIES = ("a_wide", "w_wide", "both_10bit")


def exact_A(family, batch, m, seed, dev):
    """(batch, m, 256) f32 of integers, a function of the global row index."""
    r, c = _grid(batch * m, 256, dev)
    h = mix(r, c, seed)
    if family == "a_wide":       # one odd 18-bit value in each k32 step
        pos = mix(r, c >> 5, seed + 1) & 31
        v = torch.where((c & 31) == pos, _odd18(h), torch.zeros_like(h))
    elif family == "w_wide":
        v = _small(h)
    else:                        # one 10-bit value in each 64-wide group of k
        pos = mix(r, c >> 6, seed + 1) & 63
        v = torch.where((c & 63) == pos, _int10(h), torch.zeros_like(h))
    return v.float().view(batch, m, 256)


def exact_W(family, batch, seed, dev):
    """(batch, 256, 256) f32 of integers.  The wide family is nonzero where
    (k + 5 n) % 32 == 0: 8 entries in every row and in every column, so W
    and W^T both keep the envelope."""
    r, c = _grid(batch * 256, 256, dev)
    h = mix(r, c, seed + 2)
    if family == "a_wide":
        v = _small(h)
    elif family == "w_wide":
        v = torch.where((c + 5 * r) % 32 == 0, _odd18(h), torch.zeros_like(h))
    else:
        v = _int10(h)
    return v.float().view(batch, 256, 256)


def exact_GH(family, batch, m, seed, dev):
    """Weight-gradient operands (G, H), each (batch, m, 256): the reduction
    runs over rows, so the sparse operand has its nonzeros on a diagonal
    pattern of rows -- at most 8 (wide) or 4 (10-bit) per column in any 128
    consecutive rows, and at least one per column in every 32-row stage."""
    r, c = _grid(batch * m, 256, dev)
    hg, hh = mix(r, c, seed + 3), mix(r, c, seed + 4)
    zero = torch.zeros_like(hg)
    if family == "a_wide":
        g, h = torch.where((r + 3 * c) % 16 == 0, _odd18(hg), zero), _small(hh)
    elif family == "w_wide":
        g, h = _small(hg), torch.where((r + 3 * c) % 16 == 0, _odd18(hh), zero)
    else:
        g, h = torch.where((r + 3 * c) % 32 == 0, _int10(hg), zero), _int10(hh)
    return g.float().view(batch, m, 256), h.float().view(batch, m, 256)


def exact_bwd_first(family, m, seed, dev):
    """Operands of dr_gemm_x6_bwd_first whose every partial and total is exact
    on the grid of 1/4: grad_z with four nonzeros per row, W, the tanh outputs
    h in {0, +-0.5, +-1} with 1 - h^2 nonzero on one row per row step and
    column, x in {-1, 0, 1}.  The value width follows from the envelope of the
    WHOLE minibatch: (m / 32) rows x 4 quarter-units x 4 nonzeros x 2^bits
    <= 2^22."""
    bits = min(10, int(np.floor(18 - np.log2(m // RS))))
    assert bits >= 2
    r, c = _grid(2 * m, 256, dev)
    hz, hw = mix(r, c, seed + 5), mix(_grid(512, 256, dev)[0], c, seed + 6)
    wide = lambda h: _signed(h, ((h >> 3) & ((1 << bits) - 1)) | 1)      # odd, < 2^bits
    unit = lambda h: _signed(h, torch.ones_like(h))
    pos = mix(r, c >> 6, seed + 7) & 63
    at = (c & 63) == pos
    zero = torch.zeros_like(hz)
    if family == "gz_wide":
        gz, W = torch.where(at, wide(hz), zero), (hw % 3) - 1
    else:
        gz, W = torch.where(at, unit(hz), zero), wide(hw)
    hh = mix(r, c, seed + 8)
    on = (r + c) % RS == 0
    hval = torch.where(on, torch.where(hh & 1 == 1, 0.5, 0.0) * torch.where(hh & 2 == 2, -1.0, 1.0),
                       torch.where(hh & 2 == 2, -1.0, 1.0))
    rx, cx = _grid(m, 15, dev)
    x = (mix(rx, cx, seed + 9) % 3) - 1
    return (gz.float().view(2, m, 256), W.float().view(2, 256, 256),
            hval.float().view(2, m, 256), x.float())
