"""KL control of the optimizer step on the GPU: the
gated Adam launch against the NumPy restatement tests/kl_ref.py with the
ungated kernel as its arithmetic, and PPOTrainer with target_kl and the
learning-rate schedules."""
import numpy as np
import pytest
import torch

import kl_ref
from kl_ref import f32

pytestmark = pytest.mark.gpu

S6, T0 = 6, 10                  # steps of a kernel-level iteration, Adam steps before it
STOP = kl_ref.stop_kl(0.02)     # f32(0.03)
NAN = float("nan")
TARGET = dict(target_kl=0.02)
ADAPT = dict(adaptive=True, desired_kl=0.01, lr_min=5e-4, lr_max=2e-3)

# (settings, six approx_kl values)
CASES = {
    "never_trips": (TARGET, [0.0, 0.001, 0.01, 0.02, 0.029, 0.0299]),
    "trips_at_0": (TARGET, [0.5, 0.0, 0.0, 0.0, 0.0, 0.0]),
    "trips_midway": (TARGET, [0.0, 0.01, 0.02, 0.031, 0.0, 0.001]),
    "equal_to_stop_kl": (TARGET, [0.0, STOP, STOP, 0.01, STOP, 0.0]),
    "nan_does_not_stop": (TARGET, [0.0, NAN, 0.01, NAN, 0.031, 0.0]),
    # /1.5, /1.5 into the lower clamp, held there, hold, kl 0 holds, NaN holds
    "adaptive_divide": (ADAPT, [0.021, 0.021, 0.021, 0.01, 0.0, NAN]),
    # *1.5, *1.5 into the upper clamp, held there, both bounds hold, /1.5
    "adaptive_multiply": (ADAPT, [0.004, 0.004, 0.004, 0.02, 0.005, 0.021]),
    "adaptive_with_target": (dict(ADAPT, **TARGET), [0.004, 0.021, 0.05, 0.004, 0.004, 0.0]),
}


def _opt(p, m, v, lr):
    from drone_rl_amd import ppo_kernels as K
    opt = K.ClipAdam(p.clone(), lr=lr)
    opt.m.copy_(m)
    opt.v.copy_(v)
    return opt


def _inputs(n, steps, seed):
    g = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g).cuda()
    m = (0.1 * torch.randn(n, generator=g)).cuda()
    v = (0.01 * torch.rand(n, generator=g)).cuda()
    # norms on both sides of max_grad_norm 0.5, so the clip is engaged or not
    grads = [(torch.randn(n, generator=g) * (0.2 if j % 2 else 2.0) / n ** 0.5).cuda()
             for j in range(steps)]
    return p, m, v, grads


def _control(settings, steps, lr0):
    from drone_rl_amd import ppo_kernels as K
    return K.KLControl(steps, "cuda", target_kl=settings.get("target_kl"),
                       adaptive=settings.get("adaptive", False),
                       desired_kl=settings.get("desired_kl", 0.01),
                       lr_min=settings.get("lr_min", 1e-6), lr_max=settings.get("lr_max", 1e-2),
                       lr=lr0)


def _slot_words(ctl):
    return ctl.slots.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("n", [1, 257, 524289])
def test_gated_step_follows_the_restatement(n, case):
    """One block, two blocks that must agree, and a length at which the
    grid-stride loop wraps past the launch's 2,048 blocks.  Applied steps are
    bitwise dr_clip_adam_sched at the restatement's step scalars, skipped
    steps leave params / moments / grads as they were, the slots are the
    restatement's."""
    settings, kls = CASES[case]
    adaptive = settings.get("adaptive", False)
    lr0 = 1e-3
    p, m, v, grads = _inputs(n, S6, seed=n % 1000)
    gated, ref = _opt(p, m, v, lr0), _opt(p, m, v, lr0)
    table = gated.schedule(T0 + 1, S6, lr=1.0 if adaptive else None)
    sched = table.cuda()
    ctl = _control(settings, S6, lr0)
    kl_dev = torch.tensor(kls, dtype=torch.float32).cuda()
    slots, applied = kl_ref.run(kls, lr0, **settings)
    for j in range(S6):
        g_in = grads[j].clone()
        g_gated, g_ref = grads[j].clone(), grads[j].clone()
        before = (gated.p.clone(), gated.m.clone(), gated.v.clone())
        gated.grad_norm.fill_(-1.0)
        gated.step_kl(g_gated, ctl, j, kl_dev[j:j + 1], sched)
        if applied[j] is None:
            for got, was in zip((gated.p, gated.m, gated.v), before):
                assert torch.equal(got, was), (j, "skipped step wrote the state")
            assert torch.equal(g_gated, g_in), (j, "skipped step scaled the gradient")
            # the norm is still written: the ungated kernel's on a scratch state
            scratch = _opt(*before, lr0)
            scratch.step_sched(g_ref, sched[0], 1.0)
            assert torch.equal(gated.grad_norm, scratch.grad_norm), j
            continue
        s0, s1 = kl_ref.step_scalars(table.numpy(), applied[j], adaptive)
        row = torch.tensor([s0, s1], dtype=torch.float32).cuda()
        ref.step_sched(g_ref, row, 1.0)
        for name, got, exp in (("p", gated.p, ref.p), ("m", gated.m, ref.m),
                               ("v", gated.v, ref.v), ("g", g_gated, g_ref),
                               ("norm", gated.grad_norm, ref.grad_norm)):
            assert torch.equal(got, exp), (j, name)
        assert not torch.equal(gated.p, before[0])
    want = np.stack([s.words() for s in slots])
    assert np.array_equal(_slot_words(ctl), want)
    assert torch.isfinite(gated.p).all()


def test_three_captured_steps_replayed_twice_equal_the_eager_calls():
    settings, kls, n, lr0 = dict(ADAPT, **TARGET), [0.004, 0.021, 0.031], 257, 1e-3
    p, m, v, grads = _inputs(n, 3, seed=9)
    eager, graphed = _opt(p, m, v, lr0), _opt(p, m, v, lr0)
    sched = eager.schedule(1, 3, lr=1.0).cuda()
    kl_dev = torch.tensor(kls, dtype=torch.float32).cuda()
    ge, gg = [g.clone() for g in grads], [g.clone() for g in grads]
    ce, cg = _control(settings, 3, lr0), _control(settings, 3, lr0)

    def steps(opt, ctl, gs):
        ctl.begin()
        for j in range(3):
            opt.step_kl(gs[j], ctl, j, kl_dev[j:j + 1], sched)

    for _ in range(2):
        steps(eager, ce, ge)
    torch.cuda.synchronize()
    cur, cs = torch.cuda.current_stream(), torch.cuda.Stream()
    cs.wait_stream(cur)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(cs), torch.cuda.graph(graph, stream=cs):
        steps(graphed, cg, gg)
    cur.wait_stream(cs)
    graph.replay()
    graph.replay()
    torch.cuda.synchronize()
    for name in ("p", "m", "v", "grad_norm"):
        assert torch.equal(getattr(eager, name), getattr(graphed, name)), name
    for a, b in zip(ge, gg):
        assert torch.equal(a, b)
    assert np.array_equal(_slot_words(ce), _slot_words(cg))
    # adaptive carried the rate over: the second pass began where the first ended
    slots1, _ = kl_ref.run(kls, lr0, **settings)
    slots2, _ = kl_ref.run(kls, slots1[-1].lr, **settings)
    assert np.array_equal(_slot_words(cg), np.stack([s.words() for s in slots2]))
    assert slots2[-1].stopped == 1 and slots2[-1].taken == 2


# ------------------------------------------------------------------ trainer
def _trainer(**kw):
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    return PPOTrainer(PPOConfig(**kw))


def _kls(tr):
    return tr.train_stats[:, 5].cpu().numpy().copy()


def _opt_state(tr):
    return {"flat": tr.policy.flat.detach().clone(), "m": tr.opt.m.clone(),
            "v": tr.opt.v.clone()}


def _same(a, b):
    for k in a:
        assert torch.equal(a[k], b[k]), k


def _taken_by_restatement(tr, **settings):
    slots, _ = kl_ref.run(_kls(tr), tr.opt.lr, **settings)
    return slots[-1].taken


STOP_CFG = dict(num_envs=256, n_steps=8, batch_size=2048, n_epochs=4, seed=7)


@pytest.fixture(scope="module")
def stop_probe():
    """The per-step KLs and stats rows of the first iteration without a
    target: one minibatch per epoch, four epochs, the default (256, 256) net."""
    tr = _trainer(**STOP_CFG)
    try:
        tr.learn_step()
        assert tr.train_stats.shape == (4, 8)
        return _kls(tr), tr.train_stats.clone()
    finally:
        tr.close()


def test_trainer_stops_at_a_known_step(stop_probe):
    k, rows = stop_probe
    assert k[0] == 0 < k[1]
    js = 2 if k[2] > k[1] else 1
    prev = float(k[:js].max())
    target = (prev + float(k[js])) / 3
    a = _trainer(**STOP_CFG, target_kl=target)
    b = _trainer(**dict(STOP_CFG, n_epochs=js))
    try:
        assert a.stop_kl == f32(1.5 * target) and prev < a.stop_kl < k[js]
        a.learn_step()
        b.learn_step()
        assert a.kl_state()["n_updates_taken"] == js
        assert a.opt.t == js == b.opt.t
        _same(_opt_state(a), _opt_state(b))
        assert torch.equal(a.train_stats[:js + 1], rows[:js + 1])
        w = a._kl.slots.cpu().numpy()
        assert list(w[:, 0]) == [0] * (js + 1) + [1] * (4 - js)
        # the mean that train() returns covers the rows up to the trip
        st = a.learn_step()
        assert torch.isfinite(st).all() and torch.isfinite(a.policy.flat).all()
        w = a._kl.slots.cpu().numpy()
        assert w[0, 0] == 0 and w[0, 1] == 0
        taken = a.kl_state()["n_updates_taken"]
        assert 0 <= taken <= 4 and a.opt.t == js + taken
        assert taken == _taken_by_restatement(a, target_kl=target)
        keep = a._kl.applied_mask().cpu()
        assert torch.allclose(st.cpu(), a.train_stats.cpu()[keep].mean(0), rtol=1e-5, atol=1e-7)
    finally:
        a.close()
        b.close()


MID_CFG = dict(num_envs=2048, n_steps=16, batch_size=8192, n_epochs=3, seed=5)


@pytest.mark.parametrize("net_arch,fused", [((256, 256), True), ((64, 64), True),
                                            ((260, 64), False)])
def test_trainer_stops_mid_epoch_graph_equals_eager(net_arch, fused):
    """Four minibatches x three epochs.  The captured loop and the eager one
    agree bitwise over three iterations, a stop falls inside an epoch, and the
    steps taken are the restatement's over the recorded KLs.  (260, 64) is
    refused by the fused path: the unfused loop goes through the same gate."""
    cfg = dict(MID_CFG, net_arch=net_arch)
    probe = _trainer(**cfg)
    try:
        assert probe.use_fused == fused
        probe.learn_step()
        k = _kls(probe)
    finally:
        probe.close()
    S = 12
    assert k.shape == (S,) and k[0] == 0
    records = [j for j in range(1, S) if j % 4 and k[j] > k[:j].max()]
    assert records, k
    js = records[-1] if len(records) < 3 else records[2]
    target = (float(k[:js].max()) + float(k[js])) / 3
    a, b = _trainer(**cfg, target_kl=target), _trainer(**cfg, target_kl=target)
    b.train_graph = False
    try:
        taken = []
        for it in range(3):
            sa, sb = a.learn_step(), b.learn_step()
            assert torch.equal(sa, sb) and torch.isfinite(sa).all()
            _same(_opt_state(a), _opt_state(b))
            assert torch.equal(a.train_stats, b.train_stats)
            ta = a.kl_state()["n_updates_taken"]
            assert ta == b.kl_state()["n_updates_taken"]
            assert ta == _taken_by_restatement(a, target_kl=target)
            assert a.opt.t == b.opt.t == sum(taken) + ta
            taken.append(ta)
        assert taken[0] == js
        assert any(0 < t < S and t % 4 for t in taken), taken
        if fused:
            assert a._tgraph is not None and b._tgraph is None
    finally:
        a.close()
        b.close()


def test_trainer_with_an_unreachable_target_is_the_plain_trainer():
    cfg = dict(num_envs=256, n_steps=8, batch_size=1024, n_epochs=2, seed=3)
    a, b = _trainer(**cfg, target_kl=1e9), _trainer(**cfg)
    try:
        assert b._kl is None and b._kl_host is None and b.stop_kl is None
        assert "kl_control" not in b.state_dict()
        o, c, h = b.opt, b.cfg, b.head
        assert b._graph_key("train") == (
            c.seed, b.rank, c.n_epochs, c.batch_size, c.clip_range, c.ent_coef, c.vf_coef,
            c.normalize_advantage, float(o.lr), o.b1, o.b2, o.eps, o.max_norm, float(h.clip),
            float(h.ent), float(h.vf), h.norm)
        assert a._graph_key("train")[:17] == b._graph_key("train")
        for _ in range(3):
            sa, sb = a.learn_step(), b.learn_step()
            assert torch.equal(sa, sb)
            _same(_opt_state(a), _opt_state(b))
            assert a.opt.t == b.opt.t
            assert torch.equal(a.train_stats, b.train_stats)
        assert a._tgraph is not None and b._tgraph is not None
        assert a.kl_state() == {"n_updates_taken": 4, "lr": 3e-4} == b.kl_state()
    finally:
        a.close()
        b.close()


ADAPT_CFG = dict(num_envs=256, n_steps=8, batch_size=2048, n_epochs=4, seed=7,
                 lr_schedule="adaptive")


@pytest.mark.parametrize("desired_kl,down", [(1e-9, True), (10.0, False)])
def test_adaptive_rate_moves_by_exact_factors(desired_kl, down):
    """desired_kl far below (above) any KL the run produces: the rate falls
    (rises) by 1.5 per step with a nonzero KL, inside the clamps, exactly as
    the restatement over the recorded KLs says; one capture serves all four
    iterations."""
    tr = _trainer(**ADAPT_CFG, desired_kl=desired_kl)
    try:
        assert tr.stop_kl is None and tr._kl_host is None      # no readback without a target
        lr, graph = f32(3e-4), None
        for it in range(4):
            tr.learn_step()
            k = _kls(tr)
            assert k[0] == 0
            slots, _ = kl_ref.run(k, lr, adaptive=True, desired_kl=desired_kl)
            want = slots[-1].lr
            steps = [s.lr for s in slots]
            assert steps[1] == steps[0]                       # kl == 0: hold
            for x, y in zip(steps[1:], steps[2:]):            # a move is one exact factor
                assert y in ((x, max(f32(x / f32(1.5)), f32(1e-6))) if down
                             else (x, min(f32(x * f32(1.5)), f32(1e-2))))
            assert f32(tr.kl_state()["lr"]) == want
            assert np.array_equal(tr._kl.slots.cpu().numpy().view(np.uint32),
                                  np.stack([s.words() for s in slots]))
            assert tr.opt.t == 4 * (it + 1)
            lr = want
            if it == 1:
                graph = tr._tgraph
                assert graph is not None
            elif it > 1:
                assert tr._tgraph is graph
        assert (f32(1e-6) <= lr < f32(3e-4)) if down else (f32(3e-4) < lr <= f32(1e-2))
        assert torch.isfinite(tr.policy.flat).all()
    finally:
        tr.close()


def test_adaptive_checkpoint_resumes_bitwise_with_the_saved_rate(tmp_path):
    cfg = dict(ADAPT_CFG, desired_kl=1e-9)
    a, b = _trainer(**cfg), _trainer(**cfg)
    c = _trainer(**dict(cfg, lr_schedule="constant"))
    try:
        assert c._kl is None
        for _ in range(2):
            a.learn_step()
        p = str(tmp_path / "ck.pt")
        a.save(p)
        sd = torch.load(p, map_location="cpu", weights_only=True)
        saved = sd["kl_control"]["lr"]
        assert sd["kl_control"]["lr_schedule"] == "adaptive" and 0 < saved < 3e-4
        assert f32(saved) == f32(a.kl_state()["lr"])
        a.learn_step()
        for x in (b, c):
            x.load(p)
            assert x._kl is not None and x._kl.adaptive and x.cfg.lr_schedule == "adaptive"
            assert f32(x.kl_state()["lr"]) == f32(saved)
            x.learn_step()
            _same(_opt_state(a), _opt_state(x))
            assert x.opt.t == a.opt.t and x.kl_state() == a.kl_state()
    finally:
        for t in (a, b, c):
            t.close()


def test_linear_schedule_follows_the_formula_with_one_capture():
    cfg = dict(num_envs=256, n_steps=8, batch_size=1024, n_epochs=2, seed=3)
    a, b = _trainer(**cfg, lr_schedule="linear"), _trainer(**cfg)
    try:
        assert a._kl is None                  # the rate travels through the Adam table alone
        per_iter, total = 256 * 8, 4 * 256 * 8
        logs, graphs = [], []

        def logger(d):
            logs.append(d)
            graphs.append(a._tgraph)

        a.learn(total, logger=logger)
        want = [3e-4 * max(0.0, 1.0 - (i + 1) * per_iter / total) for i in range(4)]
        assert [d["lr"] for d in logs] == want and want[-1] == 0.0
        assert [d["n_updates_taken"] for d in logs] == [4] * 4
        assert graphs[1] is not None and graphs[2] is graphs[1] and graphs[3] is graphs[1]
        # the same rates set by hand on a plain trainer: the same bits
        for lr in want:
            b.collect_rollouts()
            b.opt.lr = lr
            b.train()
        _same(_opt_state(a), _opt_state(b))
        assert a.opt.t == b.opt.t == 16
    finally:
        a.close()
        b.close()
