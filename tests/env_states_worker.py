"""The env state corpus (tests/env_states.py) on the device: the helpers of
tests/test_env_states_gpu.py, and, run as a script (argv: variant dtype ws),
the body of its subprocess cases -- DRONERL_ROLLOUT_WS, which forces a rollout
kernel form, is read once per process.  ws = 0: the one-role rollout kernel
where the size rule picks a warp-specialised form; ws = 1: the
warp-specialised forms, for "gym" with the in-kernel policy too (that one
runs env_rollout_ws_kernel where supplied actions run the split-physics
form)."""
import sys

import numpy as np
import torch

import env_states as es

TD = {"f64": torch.float64, "f32": torch.float32}
K = 4
FIELDS = ("pos", "vel", "euler", "omega", "target", "current_step")
OPTION_FIELDS = ("wind", "waypoint", "airframe")


def new_batch(variant, dtype, c, auto_reset, **kw):
    """A batch of the corpus' size holding the corpus' state.  smooth runs at
    a non-neutral lag and penalty, tag at a non-zero crash penalty; the kinds
    of es.OPTIONS are the gym variant with the option's keywords."""
    from drone_rl_amd import DroneBatch
    if variant == "smooth":
        kw.update(motor_alpha=es.SMOOTH[0], rate_penalty=es.SMOOTH[1])
    if variant == "tag":
        kw.update(tag_radius=es.TAG[0], crash_penalty=es.TAG[1])
    if variant in es.OPTIONS:
        kw.update(es.OPTIONS[variant])
        variant = "gym"
    b = DroneBatch(c["n"], variant, dtype=TD[dtype], auto_reset=auto_reset, seed=es.SEED, **kw)
    load(b, c)
    return b


def load(b, c):
    for k in es.VEC:
        if k == "target" and b.variant == "vectorized":
            continue
        b.set(k, c[k])
    b.set("current_step", c["step"])
    if b.variant == "moving":
        b.set("motion", c["motion"])
    if b.variant == "smooth":
        b.set("motor", c["motor"])
    for k in OPTION_FIELDS:
        if k in c:
            b.set(k, c[k])
    if "waypoint" in c:
        b.set("eps", c["eps"])
    if "ep_num" in c:
        assert np.array_equal(b.get("ep_num").cpu().numpy(), c["ep_num"])


def fields(b):
    out = {k: b.get(k) for k in FIELDS}
    if b.variant != "vectorized":
        out["ep_num"] = b.get("ep_num")
        out["eps"] = b.get("eps")
    if b.variant == "moving":
        out["motion"] = b.get("motion")
    if b.variant == "smooth":
        out["motor"] = b.get("motor")
    for k, on in zip(OPTION_FIELDS, (b.wind_enabled, b.waypoints_enabled, b.airframe_enabled)):
        if on:
            out[k] = b.get(k)
    return out


def bits(t):
    """The bit pattern of a tensor / array as an integer tensor: -0 differs
    from +0, the infinities keep their sign, and a NaN is a NaN wherever it
    stands (so NaN rows count, which torch.equal would fail).  Every NaN is
    mapped to one pattern: IEEE 754 leaves the sign and payload of a NaN
    result open, and which operand's NaN an instruction passes on depends on
    the operand order the compiler chose for that kernel -- measured on the
    MI355X: the rollout kernels hand on -NaN in a few entries (yaw of rows
    with all angles non-finite, omega_z of the NaN-omega rows) where the step
    kernel hands on +NaN."""
    t = torch.as_tensor(t).contiguous()
    if t.dtype == torch.float32:
        return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int32)
    if t.dtype == torch.float64:
        return torch.where(torch.isnan(t), torch.full_like(t, float("nan")), t).view(torch.int64)
    return t


def same_bits(a, b):
    return torch.equal(bits(a).cpu(), bits(b).cpu())


def actions_for(c, seed=5):
    """(K, n, 4): the corpus' own action, then the random policy's."""
    from drone_rl_amd import random_actions
    n = c["n"]
    acts = torch.empty(K, n, 4, device="cuda")
    acts[0] = torch.from_numpy(c["action"]).cuda()
    for t in range(1, K):
        random_actions(n, seed=seed, step=t, out=acts[t])
    return acts


def step_run(b, acts):
    """K dr_step launches: stacked copies of obs, rew, done."""
    o, r, d = [], [], []
    for t in range(acts.shape[0]):
        so, sr, sd = b.step(acts[t])
        o.append(so.clone())
        r.append(sr.clone())
        d.append(sd.clone())
    return torch.stack(o), torch.stack(r), torch.stack(d)


def diff_report(a, b, limit=6):
    """Where two tensors' bit patterns differ: the count, and the first few
    (row, column, got, want)."""
    x, y = bits(a).cpu().reshape(len(a), -1), bits(b).cpu().reshape(len(b), -1)
    idx = (x != y).nonzero()
    fa = torch.as_tensor(a).cpu().reshape(len(a), -1)
    fb = torch.as_tensor(b).cpu().reshape(len(b), -1)
    first = [(int(r), int(c), fa[r, c].item(), fb[r, c].item()) for r, c in idx[:limit]]
    return f"{len(idx)} entries in {len(idx[:, 0].unique())} rows differ, first {first}"


def assert_same_run(got, want, fa, fb, what):
    for name, x, y in zip(("obs", "rew", "done"), got, want):
        for t in range(x.shape[0]):
            assert same_bits(x[t], y[t]), (what, name, t, diff_report(x[t], y[t]))
    assert fa.keys() == fb.keys()
    for k in fa:
        assert same_bits(fa[k], fb[k]), (what, k, diff_report(fa[k], fb[k]))


def nan_rows_not_done_early(c, done):
    """A row whose state holds a NaN / inf and whose step counter is more than
    K below the limit is never done inside the launch (tag: nor its
    partner)."""
    bad = np.zeros(c["n"], bool)
    for k in ("pos", "vel", "euler", "omega"):
        bad |= ~np.isfinite(c[k]).all(1)
    early = c["step"] < c["max_steps"] - K
    if "pairs" in c:
        p = c["pairs"]
        calm = early & early[p] & ~(c["pos"][:, 2] <= 1) & ~(c["pos"][p][:, 2] <= 1)
    else:
        calm = early
    m = bad & calm
    assert m.sum() >= 12
    d = done.cpu().numpy().astype(bool)
    assert not d[:, m].any()
    return int(m.sum())


def check_rollout(variant, dtype, what):
    """dr_rollout over K = 4 steps from the corpus with auto_reset, against K
    dr_step launches: every output of every step and every state field, bit
    for bit.  Block E's crashes and the time limits set to expire at steps 1
    and 2 reset inside the launch, block F's from non-finite and out-of-range
    angles."""
    c = es.corpus(dtype, variant)
    a = new_batch(variant, dtype, c, True)
    b = new_batch(variant, dtype, c, True)
    acts = actions_for(c)
    got = a.rollout(K, acts)
    want = step_run(b, acts)
    assert_same_run(got, want, fields(a), fields(b), what)
    d = want[2].cpu().numpy().astype(bool)
    f = c["blocks"]["F"]
    if variant != "vectorized":
        # resets inside the launch at steps 0 and 1, block F's among them
        assert d[0].sum() > 500 and d[1].sum() > 500
        assert d[0, f].sum() >= 8 and d[1, f].sum() >= 8
        ep = a.get("ep_num").cpu().numpy()
        assert (ep[d[:3].any(0)] >= 2).all()
    nan_rows_not_done_early(c, want[2])
    a.close()
    b.close()


def check_rollout_random(variant, dtype, what):
    """The in-kernel policy: actions_out are dr_random_actions', the outputs
    those of K dr_step launches on them."""
    from drone_rl_amd import random_actions
    c = es.corpus(dtype, variant)
    a = new_batch(variant, dtype, c, True)
    b = new_batch(variant, dtype, c, True)
    n = c["n"]
    acts_out = torch.empty(K, n, 4, device="cuda")
    got = a.rollout(K, None, seed=77, step0=1000, actions_out=acts_out)
    acts = torch.stack([random_actions(n, seed=77, step=1000 + t) for t in range(K)])
    assert same_bits(acts_out, acts), (what, "actions_out")
    want = step_run(b, acts)
    assert_same_run(got, want, fields(a), fields(b), what)
    nan_rows_not_done_early(c, want[2])
    a.close()
    b.close()


if __name__ == "__main__":
    variant, dtype, ws = sys.argv[1:4]
    check_rollout(variant, dtype, f"rollout ws={ws}")
    if variant == "gym" and ws == "1":
        check_rollout_random(variant, dtype, f"rollout_random ws={ws}")
    print("ok", *sys.argv[1:])
