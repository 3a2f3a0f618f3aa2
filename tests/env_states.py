"""A designed corpus of env states for the step / rollout kernels, and the
checks that the CPU and GPU tests of it share.  Plain numpy, deterministic,
no GPU.  TEST INFRASTRUCTURE ONLY.

`corpus(dtype, variant)` returns named row blocks of states at the places the
env kernels can go wrong and a random policy never reaches:

  C_lanes  wave patterns of the out-of-range trig branch (first, so that it
           starts at row 0: see "row -> lane" below)
  A        quadrants: multiples of RN(pi/2) and their 1..3 ulp neighbours,
           signed zeros, the smallest subnormal and normal, in each angle
  B        gimbal: theta = odd k RN(pi/2) plus offsets down to one ulp
  C        the fast-range boundary: every float within 64 ulp of +-2^19
  D        huge and non-finite: |x| up to the format's top, the worst
           cancellations of the 3-FMA reduction, inf / NaN angles, NaN in
           pos / vel / omega
  E        termination and bonus edges on positions that stay put
  F        reset sources: out-of-range and non-finite angles that crash or
           time out now, one step and two steps ahead (a rollout resets them
           inside the launch)

Every array is np.float64 and holds values representable in the state dtype
("f64" or "f32"); "step" is int32, "action" / "motion" / "motor" float32.

Row -> lane.  Env i is lane i % 64 of wave i // 64 in the 64-rows-per-wave
step kernel and in all three rollout kernels (their wave bases are multiples
of 64), and lane i % 32 of wave i // 32 in the 32-rows-per-wave step forms,
which therefore see each C_lanes pattern as two half waves.  C_lanes is a
whole number of 64-row waves starting at row 0.

The gym variant's three options are corpus kinds of their own ("wind",
"waypoint", "airframe": OPTIONS): the same blocks, plus the words that are
loaded through set().  wind: mean wind and gust per row, block D's finite rows
also at signed zeros, the largest finite f32 and inf / NaN; the drag moves the
velocity ahead of the gym step, so block E's positions and targets are derived
from the restatement's vel_new dt (_wind_block_e).  airframe: m, s and the
gains inside the largest admitted spreads, at their ends, and at 1.0f in all
six words.  waypoint: the index j up to 2^24 - 1, eps over {0, 0.5, 1}; block
E's bonus edge is the f32 reach radius, with rows that reach in the step that
crashes (and, E being crossed with the time limit, in the step that times out).

The "tag" variant pairs row 2j (pursuer) with row 2j + 1 (evader); every
block has an even length, so no pair straddles two blocks."""
import zlib

import numpy as np

DT = 0.02
G = 9.81
MOTOR_MAX = 3 * 1.0 * 9.81 / 4.0
FAST = 524288.0                     # trig.h: the fast range is |x| < 2^19
SMOOTH = (0.35, 0.02)               # motor_alpha, rate_penalty of the tests
TAG = (0.3, 0.5)                    # tag_radius, crash_penalty of the tests
# The gym variant's options as corpus kinds: the constructor keywords of the
# tests.  0.3 is no f32 value, so (S)radius differs from the f64 literal; the
# spreads are the largest check_airframe admits (1/m and 1/s up to 10).
OPTIONS = {"wind": dict(drag=0.5, wind_speed=2.0, gust_sigma=0.5, gust_rate=0.1),
           "waypoint": dict(reach_radius=0.3, reach_bonus=1.0),
           "airframe": dict(mass_spread=0.9, inertia_spread=0.9, motor_spread=0.5)}
SEED = 7                          # of every batch and of the restatements' draws
J_TOP = (1 << 24) - 1               # the largest index below the Philox tag's bits
VEC = ("pos", "vel", "euler", "omega", "target")
I3 = (0.005, 0.005, 0.01)
FACTOR = 0.5 / np.sqrt(2.0)


def ftype(dtype):
    return {"f64": np.float64, "f32": np.float32}[dtype]


def max_steps_of(variant):
    return 1000 if variant == "vectorized" else 200


def bonus_edge(variant):
    """The distance below which the bonus is paid: the kernel's (S)0.05 /
    (S)1 literal, or the waypoint handle's f32 radius."""
    if variant == "waypoint":
        return float(np.float32(OPTIONS["waypoint"]["reach_radius"]))
    return 1.0 if variant == "vectorized" else 0.05


def bonus_of(variant):
    if variant == "waypoint":
        return float(np.float32(OPTIONS["waypoint"]["reach_bonus"]))
    return 1.0


def rn(x, dtype):
    """x rounded to the state dtype, as float64."""
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float64).astype(ftype(dtype)).astype(np.float64)


def ulp_steps(x, k, dtype):
    """The float k steps from x (state dtype) towards +inf (k > 0) / -inf."""
    f = ftype(dtype)
    x = np.asarray(x, np.float64).astype(f)
    to = f(np.inf) if k > 0 else f(-np.inf)
    for _ in range(abs(int(k))):
        x = np.nextafter(x, to)
    return x.astype(np.float64)


def hold_velocity(dtype):
    """RN(g dt) in the state dtype: from it, with zero thrust, the kernel's
    acc_z dt = -RN(g dt) cancels the velocity exactly."""
    f = ftype(dtype)
    return float(f(np.float64(f(G)) * np.float64(f(DT))))


def _rng(name, dtype, variant):
    return np.random.default_rng(zlib.crc32(f"{name}/{dtype}/{variant}".encode()))


def _generic(n, rng, variant):
    s = {"pos": rng.uniform(-0.5, 0.5, (n, 3)) + [0.0, 0.0, 2.0],
         "vel": rng.normal(0, 0.3, (n, 3)),
         "euler": rng.uniform(-np.pi, np.pi, (n, 3)),
         "omega": rng.normal(0, 0.5, (n, 3)),
         "target": rng.uniform(-1, 1, (n, 3)) + [0.0, 0.0, 1.0],
         "step": rng.integers(0, 150, n).astype(np.int32),
         "action": rng.uniform(0, MOTOR_MAX, (n, 4)).astype(np.float32),
         "motion": np.concatenate([rng.uniform(0.1, 0.5, (n, 3)), rng.uniform(0.5, 2.0, (n, 3)),
                                   rng.uniform(0, 2 * np.pi, (n, 3))], 1).astype(np.float32),
         "motor": rng.uniform(0, MOTOR_MAX, (n, 4)).astype(np.float32)}
    return s


def _angle_rows(name, dtype, variant, vals, where):
    """One row per (value, placement): `where` lists tuples of angle indices
    that receive the value (the other angles stay generic)."""
    vals = np.asarray(vals, np.float64)
    rng = _rng(name, dtype, variant)
    s = _generic(len(vals) * len(where), rng, variant)
    r = 0
    for idx in where:
        for k in idx:
            s["euler"][r:r + len(vals), k] = vals
        r += len(vals)
    return s


def _pio2(dtype):
    return float(rn(np.pi / 2, dtype))


def _block_a(dtype, variant):
    p = _pio2(dtype)
    f = ftype(dtype)
    base = rn(np.arange(-16, 17) * p, dtype)
    vals = [ulp_steps(base, k, dtype) for k in range(-3, 4)]
    fi = np.finfo(f)
    tiny = np.array([0.0, float(fi.smallest_subnormal), float(fi.tiny)])
    vals = np.concatenate(vals + [tiny, -tiny])
    s = _angle_rows("A", dtype, variant, vals, [(0,), (1,), (2,)])
    # the other two angles over [-8 pi, 8 pi]
    rng = _rng("A2", dtype, variant)
    n = len(vals)
    for j in range(3):
        for k in range(3):
            if k != j:
                s["euler"][j * n:(j + 1) * n, k] = rng.uniform(-8 * np.pi, 8 * np.pi, n)
    g = _generic(512, rng, variant)
    g["euler"] = rng.uniform(-8 * np.pi, 8 * np.pi, (512, 3))
    return _cat([s, g])


def _block_b(dtype, variant):
    p = _pio2(dtype)
    ks = np.array([k for k in range(-9, 10) if k % 2])
    base = rn(ks * p, dtype)
    jmax = 16 if dtype == "f64" else 7
    offs = np.concatenate([[0.0]] + [[10.0 ** -j, -10.0 ** -j] for j in range(1, jmax + 1)])
    vals = [rn(base[:, None] + offs[None, :], dtype).ravel()]
    vals += [ulp_steps(base, k, dtype) for k in (-3, -2, -1, 1, 2, 3)]
    return _angle_rows("B", dtype, variant, np.concatenate(vals), [(1,)])


def boundary_values(dtype):
    """Every float within 64 ulp of +-2^19 (129 each side)."""
    up = [ulp_steps(FAST, 0, dtype)]
    dn = []
    for k in range(1, 65):
        up.append(ulp_steps(FAST, k, dtype))
        dn.append(ulp_steps(FAST, -k, dtype))
    v = np.array(dn[::-1] + up, np.float64).ravel()
    return np.concatenate([v, -v])


def _block_c(dtype, variant):
    return _angle_rows("C", dtype, variant, boundary_values(dtype),
                       [(0,), (1,), (2,), (0, 1, 2)])


def _block_c_lanes(dtype, variant):
    """Nine 64-row waves: {all lanes, lane 17 alone, odd lanes} out of range
    x {phi, psi, all three angles}."""
    rng = _rng("C_lanes", dtype, variant)
    s = _generic(9 * 64, rng, variant)
    inside = float(ulp_steps(FAST, -1, dtype))
    lanes = np.arange(64)
    w = 0
    for angles in ((0,), (2,), (0, 1, 2)):
        for pat in (np.ones(64, bool), lanes == 17, lanes % 2 == 1):
            sign = np.where(rng.random(64) < 0.5, -1.0, 1.0)
            for k in angles:
                s["euler"][w * 64:(w + 1) * 64, k] = sign * np.where(pat, FAST, inside)
            w += 1
    return s


def worst_cancellation(dtype, count):
    """The `count` multiples k pi/2, k <= 3.3e5, whose nearest float of the
    state dtype lies closest to them (the smallest reduced argument of the
    3-FMA reduction), as (k, x).  r = (x - k P1) - k P2 is exact enough in
    f64 with P1 split into two 26-bit halves: both products with k < 2^19
    are exact and so is the first difference."""
    P1, P2 = 1.57079632679489655800e+00, 6.12323399573676603587e-17
    P1h = float((np.array([P1]).view(np.int64) & ~np.int64((1 << 27) - 1)).view(np.float64)[0])
    P1l = P1 - P1h
    k = np.arange(1, 330001, dtype=np.float64)
    x = rn(k * (np.pi / 2), dtype)
    r = np.abs(((x - k * P1h) - k * P1l) - k * P2)
    if dtype == "f32":
        r = r / np.spacing(x.astype(np.float32)).astype(np.float64)   # relative to an ulp
    else:
        r = r / np.spacing(x)
    idx = np.argsort(r, kind="stable")[:count]
    return k[idx], x[idx]


def _block_d(dtype, variant):
    top = 1e300 if dtype == "f64" else 3e38
    mags = rn(np.exp(np.linspace(np.log(FAST), np.log(top), 256)), dtype)
    mags[0] = FAST
    huge = _angle_rows("D_huge", dtype, variant, np.concatenate([mags, -mags]),
                       [(0,), (1,), (2,)])
    _, xw = worst_cancellation(dtype, 128)
    kl = np.unique(np.round(np.exp(np.linspace(0, np.log(3.3e5), 172))))
    xl = rn(kl * (np.pi / 2), dtype)
    x = np.concatenate([xw, xl])
    x = np.concatenate([x, ulp_steps(x, 1, dtype), ulp_steps(x, -1, dtype)])
    x = np.concatenate([x, -x])
    canc = _angle_rows("D_canc", dtype, variant, x, [(0,)])
    n = len(x)
    # the placement rotates over the three angles
    rng = _rng("D_canc2", dtype, variant)
    gen = rng.uniform(-np.pi, np.pi, n)
    for j in (1, 2):
        m = np.arange(n) % 3 == j
        canc["euler"][m, j] = canc["euler"][m, 0]
        canc["euler"][m, 0] = rn(gen[m], dtype)
    nf = _generic(72, _rng("D_nf", dtype, variant), variant)
    for rep in range(4):
        r = rep * 18
        for j, val in enumerate((np.inf, -np.inf, np.nan)):
            for k in range(3):
                nf["euler"][r + 3 * j + k, k] = val
        for j, fld in enumerate(("pos", "vel", "omega")):
            for k in range(3):
                nf[fld][r + 9 + 3 * j + k, k] = np.nan
    return _cat([huge, canc, nf])


def _unit(rng, n):
    u = rng.normal(size=(n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def _block_e(dtype, variant):
    f = ftype(dtype)
    fi = np.finfo(f)
    rng = _rng("E", dtype, variant)
    tiny = 1e-300 if dtype == "f64" else 1e-38
    sub = float(fi.smallest_subnormal)
    pos = []
    # pz at and around zero
    for pz in (0.0, -0.0, sub, -sub, tiny, -tiny):
        pos.append([0.25, -0.125, pz])
    # |p|^2 exactly 2500 and each component's neighbours
    for b in ((30.0, 40.0, 0.0), (0.0, 0.0, 50.0), (14.0, 48.0, 0.0), (30.0, 0.0, 40.0)):
        pos.append(list(b))
        for k in range(3):
            for d in (-1, 1):
                q = list(b)
                q[k] = float(ulp_steps(b[k], d, dtype))
                if q[2] >= 0 and not (q[2] == 0 and np.signbit(q[2])):
                    pos.append(q)
    pos = np.array(pos)
    # 2,000 directions (upper half space) scaled to 50 (1 + k eps), k = -8..8
    u = _unit(rng, 2000)
    u[:, 2] = np.abs(u[:, 2])
    kk = (np.arange(2000) % 17) - 8
    shell = u * (50.0 * (1.0 + kk * float(fi.eps)))[:, None]
    pos = np.concatenate([pos, shell])
    n0 = len(pos)
    s = _generic(n0, rng, variant)
    s["pos"] = pos
    parts = [s]
    # bonus edge: |target - pos| (tag: the partner distance) at the edge's
    # neighbours, on an axis (exact distance) and in generic directions
    tag = variant == "tag"
    edge = float(np.float32(TAG[0])) if tag else float(rn(bonus_edge(variant), dtype))
    near = [float(ulp_steps(edge, k, dtype)) for k in range(-3, 4)]
    if variant == "waypoint" and dtype == "f64":
        # between the f64 literal and the handle's f32 radius: reaches, which a
        # comparison with the literal would miss
        lit = OPTIONS["waypoint"]["reach_radius"]
        near += [lit, float(ulp_steps(lit, 1, dtype)), 0.5 * (lit + edge)]
    offs =[np.eye(3)[k] * r for k in range(3) for r in near]
    gu = _unit(rng, 200)
    offs += list(gu * (edge * (1.0 + ((np.arange(200) % 9) - 4) * float(fi.eps)))[:, None])
    offs = np.array(offs)
    m = len(offs)
    if tag:
        b = _generic(2 * m, rng, variant)
        axis = np.repeat(np.arange(3), len(near))
        base = rng.uniform(-0.5, 0.5, (m, 3)) + [0.0, 0.0, 2.0]
        # axis rows: the pursuer sits at 0 on the axis, so the difference is
        # exact (on the z axis it sits on the ground, +0, the evader above)
        base[np.arange(len(axis)), axis] = 0.0
        b["pos"][0::2] = base
        b["pos"][1::2] = base + offs
        parts.append(b)
        # partner crashed / NaN: (crash, fine), (fine, crash), (crash, crash),
        # (NaN, fine), (fine, NaN), (NaN, crash)
        c = _generic(12, rng, variant)
        kinds = [("c", "f"), ("f", "c"), ("c", "c"), ("n", "f"), ("f", "n"), ("n", "c")]
        for j, pr in enumerate(kinds):
            for h, kind in enumerate(pr):
                if kind == "c":
                    c["pos"][2 * j + h, 2] = -tiny
                elif kind == "n":
                    c["pos"][2 * j + h, 0] = np.nan
        parts.append(c)
    else:
        b = _generic(m, rng, variant)
        if variant == "vectorized":
            b["pos"] = np.array([0.0, 0.0, 10.0]) + offs
        else:
            base = rng.uniform(-0.5, 0.5, (m, 3)) + [0.0, 0.0, 2.0]
            nax = 3 * len(near)
            base[np.arange(nax), np.repeat(np.arange(3), len(near))] = 0.0
            b["pos"] = base
            b["target"] = base + offs
        parts.append(b)
        if variant == "waypoint":
            # a reach in the step that also crashes: below the ground or past
            # the shell, the waypoint a third of the radius away
            c = _generic(48, rng, variant)
            c["pos"][:24] = [0.25, -0.125, -tiny]
            c["pos"][24:] = u[:24] * (50.0 * (1.0 + 8 * float(fi.eps)))
            c["target"] = c["pos"] + _unit(rng, 48) * (edge / 3)
            parts.append(c)
    e = _cat(parts)
    n = len(e["step"])
    # the state that holds position: zero command (and motors), vel = (0, 0, RN(g dt))
    e["action"][:] = 0.0
    e["motor"][:] = 0.0
    e["motion"][:, :3] = 0.0
    e["vel"][:] = [0.0, 0.0, hold_velocity(dtype)]
    # crossed with the time limit: each state at a generic step, two steps
    # and one step before the limit
    ms = max_steps_of(variant)
    out = []
    for st in (10, ms - 2, ms - 1):
        x = {k: v.copy() for k, v in e.items()}
        x["step"] = np.full(n, st, np.int32)
        out.append(x)
    return _cat(out)


def _block_f(dtype, variant):
    top = 1e300 if dtype == "f64" else 3e38
    ms = max_steps_of(variant)
    finite = [FAST, -FAST, 1e10, -top, top]
    s = _angle_rows("F_fin", dtype, variant, rn(np.repeat(finite, 3), dtype),
                    [(0,), (1,), (2,), (0, 1, 2)])
    n = len(s["step"])
    kind = np.arange(n) % 3
    s["pos"][kind == 0, 2] = -0.5                    # crashes now
    s["step"] = np.where(kind == 1, ms - 1, np.where(kind == 2, ms - 2, 10)).astype(np.int32)
    t = _angle_rows("F_nf", dtype, variant, np.repeat([np.inf, -np.inf, np.nan], 3),
                    [(0,), (1,), (2,), (0, 1, 2)])
    m = len(t["step"])
    kind = np.arange(m) % 3
    t["step"] = np.where(kind == 1, ms - 1, np.where(kind == 2, ms - 2, 10)).astype(np.int32)
    return _cat([s, t])


def _cat(parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _wind_words(c, dtype):
    """(n,6) f32: mean wind uniform in +-2, gust normal(0, 0.5); on finite
    in-range rows of block D the signed zeros, the largest finite f32 and
    inf / NaN in each axis of the mean wind and of the gust."""
    n = c["n"]
    rng = _rng("wind_words", dtype, "wind")
    w = np.concatenate([rng.uniform(-2, 2, (n, 3)), rng.normal(0, 0.5, (n, 3))],
                       1).astype(np.float32)
    top = np.finfo(np.float32).max
    pats = [(0.0, 0.0), (-0.0, -0.0), (0.0, -0.0), (top, 0.0), (-top, 0.0), (0.0, top),
            (0.0, -top), (top, top), (np.inf, 0.0), (-np.inf, 0.0), (0.0, np.inf),
            (0.0, -np.inf), (np.inf, -np.inf), (np.nan, 0.0), (0.0, np.nan)]
    d = c["blocks"]["D"]
    ok = np.ones(n, bool)
    for k in ("pos", "vel", "euler", "omega"):
        ok &= np.isfinite(c[k]).all(1)
    ok &= (np.abs(c["euler"]) < FAST).all(1)
    cand = np.flatnonzero(ok[d]) + d.start
    rows = cand[::len(cand) // (3 * len(pats))][:3 * len(pats)]
    special = np.zeros(n, bool)
    for r, row in enumerate(rows):
        m, g = pats[r // 3]
        if r // 3 < 3:                              # the signed zeros: all six words
            w[row, :3], w[row, 3:] = m, g
        else:
            w[row, r % 3], w[row, 3 + r % 3] = m, g
        special[row] = True
    return w, special


def _airframe_words(c, dtype):
    """(n,6) f32: m, s uniform in 1 +- 0.9, the gains in 1 +- 0.5 (1.0f +
    spread * xi in f32, as the draw forms them); of every 16 rows one at 1.0f in
    all six words and six with m, s or a gain at exactly 1 -+ spread."""
    n = c["n"]
    o = OPTIONS["airframe"]
    rng = _rng("airframe_words", dtype, "airframe")
    sp = np.array([o["mass_spread"], o["inertia_spread"]] + [o["motor_spread"]] * 4, np.float32)
    one = np.float32(1.0)
    af = one + sp * rng.uniform(-1, 1, (n, 6)).astype(np.float32)
    r = np.arange(n) % 16
    af[r == 0] = one
    for k, (col, sign) in enumerate([(0, -1), (0, 1), (1, -1), (1, 1), (2, -1), (5, 1)], 1):
        af[r == k, col] = one + np.float32(sign) * sp[col]
    return af


def _waypoint_words(c, dtype):
    """(n,2) i32 (j, q) with j over {0, 1, 3, 2^24 - 2, 2^24 - 1}, and the
    curriculum eps (n,) over {0, 0.5, 1}: every pair occurs in every block of
    15 rows.  The top indices show that the counter word is not truncated
    where it is OR-ed under the Philox tag."""
    n = c["n"]
    rng = _rng("waypoint_words", dtype, "waypoint")
    j = np.array([0, 1, 3, J_TOP - 1, J_TOP], np.int32)[np.arange(n) % 5]
    wp = np.stack([j, rng.integers(0, 1000, n).astype(np.int32)], 1)
    return wp, np.array([0.0, 0.5, 1.0])[np.arange(n) % 3]


def _wind_block_e(c, dtype):
    """The drag moves the velocity ahead of the gym step, so block E does not
    hold position.  vel_new dt does not depend on pos: taken once from the
    restatement, each row's pos becomes P - vel_new dt and its target moves
    with the position the restatement then reaches, P the position (and
    target - P the offset) the block was designed at.  The rows at pz = 0,
    +-subnormal, +-tiny become the 0, +-1, +-3 ulp neighbours of -vel_new_z dt."""
    e = c["blocks"]["E"]
    s, _, _, _ = oracle_step("wind", c)
    vdt = s["vel"][e] * DT
    P, off = c["pos"][e].copy(), c["target"][e] - c["pos"][e]
    pos = rn(P - vdt, dtype)
    third = (e.stop - e.start) // 3
    for t in range(3):
        for r, k in enumerate((0, 0, 1, -1, 3, -3)):
            i = t * third + r
            pos[i, 2] = ulp_steps(rn(-vdt[i, 2], dtype), k, dtype)
    c["pos"][e] = pos
    s, _, _, _ = oracle_step("wind", c)
    c["target"][e] = rn(s["pos"][e] + off, dtype)


_BLOCKS = (("C_lanes", _block_c_lanes), ("A", _block_a), ("B", _block_b), ("C", _block_c),
           ("D", _block_d), ("E", _block_e), ("F", _block_f))
_CACHE = {}


def corpus(dtype, variant):
    """dict: "blocks" {name: slice}, pos / vel / euler / omega / target (n,3)
    f64 holding state-dtype values, step (n,) i32, action (n,4) f32, "motion"
    (n,9) f32 (moving), "motor" (n,4) f32 (smooth), "pairs" (n,) the
    partner's row (tag), "n", "max_steps".  `variant` may be one of the gym
    options' kinds (OPTIONS): then the words loaded through set() come too,
    "wind" (n,6) f32 with "wind_special" (n,) marking block D's extreme rows,
    "airframe" (n,6) f32, "waypoint" (n,2) i32 with "eps" (n,), and "ep_num"
    (n,) as a fresh handle reports it.  A fresh copy on every call."""
    key = (dtype, variant)
    if key not in _CACHE:
        parts, blocks, r = [], {}, 0
        for name, fn in _BLOCKS:
            p = fn(dtype, variant)
            if len(p["step"]) % 2:                       # even blocks: tag pairs
                p = _cat([p, {k: v[-1:] for k, v in p.items()}])
            blocks[name] = slice(r, r + len(p["step"]))
            r += len(p["step"])
            parts.append(p)
        pad = (34 - r) % 64                              # n = 34 mod 64: even, ragged
        parts.append(_generic(pad, _rng("pad", dtype, variant), variant))
        blocks["pad"] = slice(r, r + pad)
        c = _cat(parts)
        for k in VEC:
            c[k] = np.ascontiguousarray(rn(c[k], dtype))
        c["blocks"] = blocks
        c["n"] = r + pad
        c["max_steps"] = max_steps_of(variant)
        if variant == "vectorized":
            c["target"][:] = [0.0, 0.0, 10.0]
        if variant != "moving":
            del c["motion"]
        if variant != "smooth":
            del c["motor"]
        if variant == "tag":
            c["pairs"] = np.arange(c["n"]) ^ 1
        if variant in OPTIONS:
            c["ep_num"] = np.ones(c["n"], np.int32)      # a fresh handle's
        if variant == "wind":
            c["wind"], c["wind_special"] = _wind_words(c, dtype)
            _wind_block_e(c, dtype)
        if variant == "airframe":
            c["airframe"] = _airframe_words(c, dtype)
        if variant == "waypoint":
            c["waypoint"], c["eps"] = _waypoint_words(c, dtype)
        _CACHE[key] = c
    c = _CACHE[key]
    return {k: (v.copy() if isinstance(v, np.ndarray) else
                (dict(v) if isinstance(v, dict) else v)) for k, v in c.items()}


def rows_of(c, names):
    m = np.zeros(c["n"], bool)
    for nm in names:
        m[c["blocks"][nm]] = True
    return m


AD = ("C_lanes", "A", "B", "C", "D", "pad")


# ---------------------------------------------------------------------------
# the oracle over a corpus
# ---------------------------------------------------------------------------
def oracle_step(variant, c, fault=None):
    """One step of the CPU oracle from corpus `c` (not modified).  Returns
    (state dict after the step, obs, rew, done).  gym / moving / vectorized:
    oracle.cref; smooth / tag / wind / waypoint / airframe: the NumPy
    restatements (the options' with seed SEED, gids = arange(n) and the
    corpus' ep_num; waypoint adds "reached" and "d" to the state dict).
    `fault` names one of a restatement's deliberately wrong forms, for
    tests/test_env_states_cpu.py."""
    from oracle import cref
    s = {k: np.ascontiguousarray(c[k].copy()) for k in VEC}
    s["step"] = c["step"].astype(np.int32).copy()
    a = c["action"]
    with np.errstate(all="ignore"):
        if variant == "gym":
            obs, rew, done = cref.gym_step(s, a)
        elif variant == "moving":
            s["motion"] = c["motion"].copy()
            obs, rew, done = cref.moving_step(s, a)
        elif variant == "smooth":
            from smooth_ref import smooth_step
            s["motor"] = c["motor"].copy()
            obs, rew, done = smooth_step(s, a, *SMOOTH)
        elif variant == "tag":
            from tag_ref import tag_step
            obs, rew, done, crash = tag_step(s, a, TAG[0], TAG[1])
            s["crash"] = crash
        elif variant == "wind":
            from wind_ref import wind_step
            s["wind"], s["ep_num"] = c["wind"].copy(), c["ep_num"]
            obs, rew, done = wind_step(s, a, OPTIONS["wind"], SEED, np.arange(c["n"]),
                                       fault=fault)
        elif variant == "waypoint":
            from waypoint_ref import waypoint_step
            s["waypoint"], s["ep_num"], s["eps"] = c["waypoint"].copy(), c["ep_num"], c["eps"]
            obs, rew, done, s["reached"], s["d"] = waypoint_step(
                s, a, OPTIONS["waypoint"], SEED, np.arange(c["n"]), fault=fault)
        elif variant == "airframe":
            from airframe_ref import airframe_step
            s["airframe"] = c["airframe"].copy()
            obs, rew, done = airframe_step(s, a, fault=fault)
        else:
            # the oracle's step counter is shared: one call per distinct step
            n = c["n"]
            obs = np.zeros((n, 12), np.float32)
            rew = np.zeros(n)
            done = np.zeros(n, bool)
            for st in np.unique(s["step"]):
                m = s["step"] == st
                sub = {k: np.ascontiguousarray(s[k][m]) for k in VEC[:4]}
                o, r, d, _ = cref.vec_step(sub, np.ascontiguousarray(a[m]), int(st))
                obs[m], rew[m], done[m] = o, r, d
                for k in VEC[:4]:
                    s[k][m] = sub[k]
            s["step"] = s["step"] + 1
    return s, obs, np.asarray(rew, np.float64), np.asarray(done, bool)


# ---------------------------------------------------------------------------
# the float bound:  |got - ref| <= gamma(c) * envelope
# ---------------------------------------------------------------------------
def unit_roundoff(dtype):
    return 2.0 ** -53 if dtype == "f64" else 2.0 ** -24


def rounding_counts(dtype, out_of_range, kernel=True, variant=None):
    """Roundings (in units of u = half an ulp, relative to the envelope)
    behind each state output of one side of a comparison.  See
    tests/test_env_states_gpu.py for the derivation.  `out_of_range` (n,)
    bool: rows with an angle on the library trig path.  `variant` matters
    for the gym options' kinds only: "wind" adds the drag impulse's roundings
    to vel, "airframe" the reciprocal products' to vel and omega."""
    K = 1.0 if (dtype == "f32" and kernel) else 0.0     # constants rounded to f32
    if kernel:
        # fast path: 1 ulp (f64) / 2 ulp (f32) from the correctly rounded
        # value (trig.h), so 1.5 / 2.5 ulp = 3u / 5u from the true one;
        # library path: the OpenCL C bound of 4 ulp = 8u that the device
        # library is built to (unverified)
        S = np.where(out_of_range, 8.0, 3.0 if dtype == "f64" else 5.0)
        tan = 2 * S + 2                                 # sth, cth, corrected quotient
    else:
        S = np.full(out_of_range.shape, 2.0)            # glibc / numpy: 1 ulp
        tan = np.full(out_of_range.shape, 2.0)
    vel = 3 * S + 6 + 2 * K
    omg = np.full(out_of_range.shape, 8 + 4 * K)
    if variant == "wind":
        # v' = v + ((k (w - v)) dt): the difference, x k, x dt (+K), the sum;
        # w and (S)k are exact casts
        vel = vel + 4 + K
    if variant == "airframe":
        # x (S)im where the gym's / kMass is exact; x (S)is on each torque
        vel = vel + 1
        omg = omg + 1
    pos = vel + 2 + K
    eul = S + tan + 6 + K
    rew = pos + 7 + K
    return {"vel": vel, "pos": pos, "euler": eul, "omega": omg, "rew": rew}


def bound_counts(dtype, out_of_range, both_cpu=False, variant=None):
    """c per row and output: kernel side + reference side.  The f64 oracle
    has the kernel's operations with 1 ulp library trig; against an f32
    kernel its whole error is below one f32 rounding."""
    ref = rounding_counts("f64", out_of_range, kernel=False, variant=variant)
    if both_cpu:
        return {k: 2 * ref[k] for k in ref}
    ker = rounding_counts(dtype, out_of_range, kernel=True, variant=variant)
    if dtype == "f64":
        return {k: ker[k] + ref[k] for k in ker}
    return {k: ker[k] + 1 for k in ker}


def envelopes(variant, c, tgt_new=None):
    """The value expressions of one step with every term replaced by its
    absolute value, from the pre-step corpus `c` (f64 numpy): dict of (n,3)
    arrays for vel / pos / euler / omega and (n,) "rew" (without the bonus and
    the f32-side terms, which the caller adds).  wind: |v| + k (|w| + |v|) dt
    stands where |v| does, w the f32 sum of the mean wind and the updated gust;
    airframe: the gained command, 1/m on the thrust terms, 1/s on the
    torques."""
    with np.errstate(all="ignore"):
        e = c["euler"]
        sph, cph = np.abs(np.sin(e[:, 0])), np.abs(np.cos(e[:, 0]))
        sth, cth = np.abs(np.sin(e[:, 1])), np.abs(np.cos(e[:, 1]))
        sps, cps = np.abs(np.sin(e[:, 2])), np.abs(np.cos(e[:, 2]))
        a = c["action"].astype(np.float32)
        if variant == "smooth":
            al = np.float32(SMOOTH[0])
            a = (np.float32(1.0) - al) * c["motor"] + al * a
        im = isc = 1.0
        if variant == "airframe":
            af = c["airframe"]
            a = af[:, 2:] * a
            im = (np.float32(1.0) / af[:, 0]).astype(np.float64)
            isc = (np.float32(1.0) / af[:, 1]).astype(np.float64)
        v0 = np.abs(c["vel"])
        if variant == "wind":
            w = np.abs((c["wind"][:, :3] + gust_after(c)).astype(np.float64))
            v0 = v0 + (float(np.float32(OPTIONS["wind"]["drag"])) * (w + v0)) * DT
        a0, a1, a2, a3 = (a[:, k] for k in range(4))
        T = np.abs((((a0 + a1) + a2) + a3).astype(np.float64))
        mphi = np.abs((((a0 + a1) - a2) - a3).astype(np.float64))
        mth = np.abs((((-a0 + a1) + a2) - a3).astype(np.float64))
        mpsi = np.abs((np.float32(0.01) * (((a0 - a1) + a2) - a3)).astype(np.float64))
        acc = np.stack([(cps * sth * cph + sps * sph) * T * im,
                        (sps * sth * cph + cps * sph) * T * im, G + (cth * cph) * T * im], 1)
        vel = v0 + acc * DT
        pos = np.abs(c["pos"]) + vel * DT
        w = np.abs(c["omega"])
        tth = sth / cth
        ed = np.stack([w[:, 0] + (sph * tth) * w[:, 1] + (cph * tth) * w[:, 2],
                       cph * w[:, 1] + sph * w[:, 2],
                       (sph / cth) * w[:, 1] + (cph / cth) * w[:, 2]], 1)
        eul = np.abs(e) + ed * DT
        wd = np.stack([(FACTOR * mphi * isc + abs(I3[1] - I3[2]) * w[:, 1] * w[:, 2]) / I3[0],
                       (FACTOR * mth * isc + abs(I3[2] - I3[0]) * w[:, 0] * w[:, 2]) / I3[1],
                       (mpsi * isc + abs(I3[0] - I3[1]) * w[:, 0] * w[:, 1]) / I3[2]], 1)
        omg = w + wd * DT
        if variant == "tag":
            other = pos[c["pairs"]]
        else:
            other = np.abs(c["target"] if tgt_new is None else tgt_new)
        d = np.sqrt(((pos + other) ** 2).sum(1))
    return {"vel": vel, "pos": pos, "euler": eul, "omega": omg, "rew": 0.01 * d}


def gamma(cnt, u):
    return cnt * u / (1.0 - cnt * u)


def same_nonfinite(got, ref):
    """NaN exactly where ref has NaN, infinities with ref's sign."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    return bool(np.array_equal(np.isnan(got), np.isnan(ref)) and
                np.array_equal(np.where(np.isinf(got), np.sign(got), 0.0),
                               np.where(np.isinf(ref), np.sign(ref), 0.0)))


def worst_ratio(got, ref, env, cnt, u):
    """max over the finite entries of |got - ref| / (u envelope), and the
    same divided by the count c (<= 1 passes; gamma's second-order term
    included).  cnt broadcasts over the columns."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    cnt = np.asarray(cnt, np.float64)
    if got.ndim == 2 and cnt.ndim == 1:
        cnt = cnt[:, None]
    cnt = np.broadcast_to(cnt, got.shape)
    fin = np.isfinite(ref) & np.isfinite(env)
    with np.errstate(all="ignore"):
        err = np.abs(got - ref)
        units = np.where(fin & (err > 0), err / (u * env), 0.0)
        rel = np.where(fin & (err > 0), err / (gamma(cnt, u) * env), 0.0)
    # a finite reference with a zero envelope is an exact zero
    rel = np.where(fin & (env == 0) & (err > 0), np.inf, rel)
    return float(np.max(units, initial=0.0)), float(np.max(rel, initial=0.0))


# ---------------------------------------------------------------------------
# exact self-consistency in the state dtype
# ---------------------------------------------------------------------------
def done_predicate(variant, dtype, pos_new, step_new, max_steps):
    """The reference's termination formula on the new position, in numpy of
    the state dtype: (pz < 0) | (sqrt((px^2 + py^2) + pz^2) > 50) | step >=
    max; tag: own crash flag and the pair's common end.  Returns (done,
    crash)."""
    f = ftype(dtype)
    p = np.asarray(pos_new, np.float64).astype(f)
    with np.errstate(all="ignore"):
        pn = np.sqrt((p[:, 0] * p[:, 0] + p[:, 1] * p[:, 1]) + p[:, 2] * p[:, 2])
        crash = (p[:, 2] < f(0)) | (pn > f(50))
    done = crash | (np.asarray(step_new) >= max_steps)
    if variant == "tag":
        done = done | done[np.arange(len(done)) ^ 1]
    return done, crash


def reward_exact(variant, dtype, pos_new, target, crash=None, dev_sq=None):
    """The reward the kernel must have produced, from the position it stored:
    every operation in numpy of the state dtype in physics_step_mixed's order
    (the source is compiled without FMA contraction), then the f32 cast and
    the variant's f32 terms."""
    f = ftype(dtype)
    p = np.asarray(pos_new, np.float64).astype(f)
    with np.errstate(all="ignore"):
        if variant == "tag":
            q = p[np.arange(len(p)) ^ 1]
            d3 = p - q
        else:
            d3 = p - np.asarray(target, np.float64).astype(f)
        d = np.sqrt((d3[:, 0] * d3[:, 0] + d3[:, 1] * d3[:, 1]) + d3[:, 2] * d3[:, 2])
        if variant == "vectorized":
            r = f(-0.01) * d
            r = np.where(d < f(1), r + f(1), r)
        elif variant == "tag":
            g = f(0.01) * -d
            g = np.where(d < f(np.float32(TAG[0])), g + f(1), g)
            r = np.where(np.arange(len(p)) % 2 == 0, g, -g)
        else:
            r = f(0.01) * -d
            r = np.where(d < f(bonus_edge(variant)), r + f(bonus_of(variant)), r)
        rf = r.astype(np.float32)
        if variant == "smooth" and SMOOTH[1] != 0:
            rf = rf - np.float32(SMOOTH[1]) * dev_sq
        if variant == "tag" and TAG[1] != 0:
            rf = np.where(crash, rf - np.float32(TAG[1]), rf).astype(np.float32)
    return rf.astype(np.float32)


def gust_after(c):
    """(n,3) f32: the wind corpus' gust after one step, wind_ref.gust_update
    on the step's own noise (three f32 roundings per element)."""
    import wind_ref
    o = OPTIONS["wind"]
    xi = wind_ref.gust_noise(SEED, np.arange(c["n"]), c["ep_num"], c["step"])
    with np.errstate(all="ignore"):
        return wind_ref.gust_update(c["wind"][:, 3:], xi,
                                    *wind_ref.gust_coefficients(o["gust_sigma"], o["gust_rate"]))


def reached_exact(dtype, pos_new, target):
    """The waypoint option's reach flag from the position the kernel stored
    and the waypoint the step started with: d < (S)R in numpy of the state
    dtype, d the reward's distance (NaN compares false)."""
    f = ftype(dtype)
    with np.errstate(all="ignore"):
        d3 = np.asarray(pos_new, np.float64).astype(f) - np.asarray(target, np.float64).astype(f)
        d = np.sqrt((d3[:, 0] * d3[:, 0] + d3[:, 1] * d3[:, 1]) + d3[:, 2] * d3[:, 2])
        return d < f(bonus_edge("waypoint"))


def option_exact_failures(variant, dtype, c, got):
    """What a step must leave in an option's words, exactly, given the
    position it stored: `got` holds "pos" and "target" after the step and the
    option's field.  Returns the names of the checks that fail.

      wind      the mean wind unchanged, the gust bitwise wind_ref.gust_update
                (f32 in both state dtypes), non-finite rows included
      airframe  the six words untouched
      waypoint  reached = d < (S)R from the stored position and the OLD
                waypoint; (j, q) advanced by one on those rows and untouched
                elsewhere; the new target bitwise waypoint_ref.waypoint cast to
                the state dtype, (0, 0, 1) where eps == 0, the old one on the
                other rows"""
    n, bad = c["n"], []
    if variant == "wind":
        if not same_bits_or_nan(got["wind"][:, :3], c["wind"][:, :3]).all():
            bad.append("mean wind")
        if not same_bits_or_nan(got["wind"][:, 3:], gust_after(c)).all():
            bad.append("gust")
    if variant == "airframe":
        if not same_bits_or_nan(got["airframe"], c["airframe"]).all():
            bad.append("airframe words")
    if variant == "waypoint":
        import waypoint_ref
        reached = reached_exact(dtype, got["pos"], c["target"])
        wp = c["waypoint"] + reached[:, None].astype(np.int32)
        if not np.array_equal(got["waypoint"], wp):
            bad.append("counters")
        tgt = c["target"].copy()
        tgt[reached] = rn(waypoint_ref.waypoint(SEED, np.arange(n)[reached], c["ep_num"][reached],
                                                wp[reached, 0], c["eps"][reached]), dtype)
        z = reached & (c["eps"] == 0)
        assert z.sum() >= 20 and (tgt[z] == [0.0, 0.0, 1.0]).all()
        if not same_bits_or_nan(np.asarray(got["target"], np.float64), tgt).all():
            bad.append("target")
    return bad


def smooth_dev_sq(c):
    d = c["action"].astype(np.float32) - c["motor"]
    return ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) + d[:, 3] * d[:, 3]


def same_bits_or_nan(a, b):
    """Elementwise: equal bit patterns, or both NaN (payloads are not part of
    the contract between numpy and the device)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    iv = {4: np.int32, 8: np.int64}[a.dtype.itemsize]
    return (a.view(iv) == b.view(iv)) | (np.isnan(a) & np.isnan(b))


# ---------------------------------------------------------------------------
# arbitrary-precision sin / cos
# ---------------------------------------------------------------------------
def mp_sincos(x, prec=240):
    """sin and cos of the exact float64 inputs by mpmath at `prec` bits (it
    widens its own working precision by the argument's exponent, so huge
    arguments are reduced exactly), each as a double-double (hi, lo):
    returns sh, sl, ch, cl.  Non-finite inputs give NaN."""
    import mpmath
    x = np.asarray(x, np.float64).ravel()
    out = np.full((4, len(x)), np.nan)
    with mpmath.workprec(prec):
        for i, xi in enumerate(x.tolist()):
            if not np.isfinite(xi):
                continue
            c, s = mpmath.cos_sin(mpmath.mpf(xi))
            sh, ch = float(s), float(c)
            out[0, i], out[1, i] = sh, float(s - sh)
            out[2, i], out[3, i] = ch, float(c - ch)
    return out


def ulp_error(got, hi, lo, dtype):
    """|got - true| in ulps of the true value in `dtype` (true = hi + lo)."""
    f = ftype(dtype)
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(hi).astype(f)).astype(np.float64)
        err = np.abs((got - hi) - lo) / ulp
    return np.where((hi == 0) & (lo == 0), np.where(got == 0, 0.0, np.inf), err)


def correctly_rounded(hi, lo, dtype):
    """RN(hi + lo) in `dtype` without double rounding, as float64."""
    f = ftype(dtype)
    with np.errstate(all="ignore"):
        c = np.asarray(hi, np.float64).astype(f)
        best, bd = c.astype(np.float64), np.abs((c.astype(np.float64) - hi) - lo)
        for to in (f(np.inf), f(-np.inf)):
            n = np.nextafter(c, to).astype(np.float64)
            d = np.abs((n - hi) - lo)
            best, bd = np.where(d < bd, n, best), np.minimum(d, bd)
    return best


def ulp_distance(got, hi, lo, dtype):
    """|got - RN(true)| in ulps of RN(true): what "within k ulp of the
    correctly rounded result" (trig.h) measures.  An integer wherever got and
    RN(true) share a binade."""
    f = ftype(dtype)
    cr = correctly_rounded(hi, lo, dtype)
    got = np.asarray(got, np.float64)
    with np.errstate(all="ignore"):
        ulp = np.spacing(np.abs(cr).astype(f)).astype(np.float64)
        return np.where(got == cr, 0.0, np.abs(got - cr) / ulp)


def trig_sweep(dtype, n_random=6000, n_log=2048):
    """Fast-range arguments for the sin / cos ulp tests: blocks A, C and D
    below 2^19, [5e5, 2^19), log-spaced magnitudes, both signs."""
    rng = _rng("trig_sweep", dtype, "-")
    p = _pio2(dtype)
    base = rn(np.arange(-16, 17) * p, dtype)
    a = np.concatenate([ulp_steps(base, k, dtype) for k in range(-3, 4)])
    fi = np.finfo(ftype(dtype))
    tiny = np.array([0.0, float(fi.smallest_subnormal), float(fi.tiny)])
    c = boundary_values(dtype)
    _, xw = worst_cancellation(dtype, 256)
    d = np.concatenate([xw, ulp_steps(xw, 1, dtype), ulp_steps(xw, -1, dtype)])
    lo = 1e-300 if dtype == "f64" else 1e-38
    lg = np.exp(np.linspace(np.log(lo), np.log(FAST), n_log))
    top = rng.uniform(5e5, FAST, n_random // 2)
    rnd = np.concatenate([rng.uniform(-4, 4, n_random), rng.uniform(-400, 400, n_random // 2),
                          rng.uniform(-5e5, 5e5, n_random // 2)])
    x = np.concatenate([a, tiny, c, d, lg, top, rnd])
    x = rn(np.concatenate([x, -x]), dtype)
    return x[np.abs(x) < FAST]
