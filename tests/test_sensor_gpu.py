"""The sensor model on the device: dr_sensor_* against
the NumPy restatement bit for bit -- every output and every state word after
every step -- on synthetic observations and done patterns (the env is not
needed), under graph replay, and inside PPOTrainer."""
import numpy as np
import pytest
import torch

import trainer_checks as TC
from sensor_ref import CASES, STEPS, bits, case_inputs, make_ref

pytestmark = pytest.mark.gpu

SENTINEL = 777.0


def _model(inp, seed=7, env_id_offset=0):
    from drone_rl_amd import ppo_kernels as K
    return K.SensorModel(inp["n"], inp["od"], "cuda", columns=(inp["sigma"], inp["beta"],
                                                               inp["mirror"]),
                         delay=inp["delay"], seed=seed, env_id_offset=env_id_offset)


def _same_state(sm, ref, where):
    assert np.array_equal(sm.state.cpu().numpy(), ref.state()), (where, "state")
    assert np.array_equal(bits(sm.bias.cpu().numpy()), bits(ref.bias)), (where, "bias")
    assert np.array_equal(bits(sm.ring.cpu().numpy()), bits(ref.ring)), (where, "ring")


@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d-od%d-d%d_%d-%s%s-%s" % (
    c[0], c[1], c[2][0], c[2][1], "mir" if c[3] else "nomir", "-term" if c[4] else "", c[5]))
def test_device_equals_the_restatement_bitwise(case):
    inp = case_inputs(case)
    n, od = inp["n"], inp["od"]
    sm, ref = _model(inp), make_ref(inp)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = sm.reset(dev(inp["obs0"]))
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref.reset(inp["obs0"]))), "reset"
    _same_state(sm, ref, "reset")
    obs, dones = dev(inp["obs"]), dev(inp["dones"])
    term = None if inp["term"] is None else dev(inp["term"])
    to = torch.empty(n, od, dtype=torch.float32, device="cuda")
    for t in range(STEPS):
        if term is None:
            out = sm.step(obs[t], dones[t])
            want = ref.step(inp["obs"][t], inp["dones"][t])
        else:
            to.fill_(SENTINEL)
            out, _ = sm.step(obs[t], dones[t], term_obs=term[t], term_out=to)
            want, want_to = ref.step(inp["obs"][t], inp["dones"][t], inp["term"][t],
                                     np.full((n, od), SENTINEL, np.float32))
            got_to = to.cpu().numpy()
            assert np.array_equal(bits(got_to), bits(want_to)), (t, "terminal_out")
            # rows of envs that are not done keep the sentinel
            assert (got_to[inp["dones"][t] == 0] == SENTINEL).all()
        assert np.array_equal(bits(out.cpu().numpy()), bits(want)), (t, "out")
        _same_state(sm, ref, t)
    if inp["dones"].any():
        assert ref.ep.max() >= 1


def test_neutral_configuration_is_the_identity_bitwise():
    from drone_rl_amd import ppo_kernels as K
    n, od = 321, 15
    g = torch.Generator().manual_seed(4)
    sm = K.SensorModel(n, od, "cuda", columns=K.sensor_columns("gym", (0,) * 4, (0,) * 4))
    x = torch.randn(n, od, generator=g)
    x[0, :4] = torch.tensor([-0.0, 0.0, float("inf"), float("nan")])
    x[5, 12:] = -0.0
    same = lambda a, b: torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert same(sm.reset(x.cuda()).cpu(), x)
    for t in range(5):
        x = torch.randn(n, od, generator=g)
        x[t, 12:] = -0.0
        done = (torch.rand(n, generator=g) < 0.3).to(torch.uint8)
        out, to = sm.step(x.cuda(), done.cuda(), term_obs=(-x).cuda())
        assert same(out.cpu(), x)
        assert same(to.cpu()[done.bool()], (-x)[done.bool()])


def test_env_id_offset_slices_the_draws():
    inp = case_inputs((128, 15, (0, 4), True, True, "random"), seed=1)
    half = dict(inp, n=64)
    whole, part = _model(inp), _model(half, env_id_offset=64)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    assert torch.equal(whole.reset(dev(inp["obs0"]))[64:], part.reset(dev(inp["obs0"][64:])))
    for t in range(12):
        a, ta = whole.step(dev(inp["obs"][t]), dev(inp["dones"][t]), term_obs=dev(inp["term"][t]))
        b, tb = part.step(dev(inp["obs"][t, 64:]), dev(inp["dones"][t, 64:]),
                          term_obs=dev(inp["term"][t, 64:]))
        assert torch.equal(a[64:], b), t
        d = torch.from_numpy(inp["dones"][t, 64:]).bool()
        assert torch.equal(ta[64:][d], tb[d]), t
    assert torch.equal(whole.state[:, 64:], part.state)
    assert torch.equal(whole.bias[64:], part.bias) and torch.equal(whole.ring[:, 64:], part.ring)


def test_captured_steps_replayed_equal_eager_steps_bitwise():
    inp = case_inputs((4099, 15, (0, 4), True, True, "random"), seed=2)
    n, od, K8 = inp["n"], inp["od"], 8
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    obs, dones, term = dev(inp["obs"]), dev(inp["dones"]), dev(inp["term"])
    outs = []
    for graphed in (False, True):
        sm = _model(inp)
        sm.reset(dev(inp["obs0"]))
        sm.step(obs[0], dones[0], term_obs=term[0])        # eager once: lazy library init
        out = torch.zeros(K8, n, od, device="cuda")
        to = torch.full((K8, n, od), SENTINEL, device="cuda")

        def body():
            for t in range(K8):
                sm.step(obs[1 + t], dones[1 + t], term_obs=term[1 + t], obs_out=out[t],
                        term_out=to[t])
        if graphed:
            cur = torch.cuda.current_stream()
            cs = torch.cuda.Stream()
            cs.wait_stream(cur)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.stream(cs), torch.cuda.graph(g, stream=cs):
                body()
            cur.wait_stream(cs)
            g.replay()
        else:
            body()
        torch.cuda.synchronize()
        outs.append((out, to, sm.state.clone(), sm.bias.clone(), sm.ring.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert inp["dones"][1:9].any()


# ------------------------------------------------------------------ trainer
N, T = 256, 8
NOISE, BIAS, DELAY = (0.02, 0.05, 0.02, 0.1), (0.02, 0.0, 0.01, 0.0), (0, 2)


def _make(**cfg):
    def make():
        near_limit = cfg.get("bootstrap_timeouts", False)
        tr = TC.small_trainer(**dict(dict(num_envs=N, n_steps=T, batch_size=1024, obs_noise=NOISE,
                                          obs_bias=BIAS, obs_delay=DELAY), **cfg))
        if near_limit:
            # every env five steps short of the limit: the first rollout truncates
            tr.env.set("current_step", torch.full((N,), 195, dtype=torch.int32))
        return tr
    return make


def _plain(**cfg):
    """The same trainer built without the sensor model: a checkpoint enables it."""
    return lambda: TC.small_trainer(**dict(dict(num_envs=N, n_steps=T, batch_size=1024), **cfg))


@pytest.mark.parametrize("name,cfg,field,shape", [
    ("alone", {}, "pos", (N, 3)),
    ("normalize_obs", dict(normalize_obs=True), "pos", (N, 3)),
    ("bootstrap_timeouts", dict(bootstrap_timeouts=True), "pos", (N, 3)),
    ("rk4", dict(variant="rk4"), "quat", (N, 4)),
    ("wind", dict(drag=0.5, wind_speed=2.0, gust_sigma=0.5, gust_rate=0.1), "wind", (N, 6)),
])
def test_trainer_graph_equals_eager_and_resumes(tmp_path, name, cfg, field, shape):
    seen_trunc = []

    def at_save(sd):
        s = sd["sensor"]
        assert tuple(s["state"].shape) == (3, N) and tuple(s["ring"].shape)[:2] == (DELAY[1] + 1, N)
        assert tuple(sd["config"]["obs_noise"]) == NOISE and tuple(sd["config"]["obs_delay"]) == DELAY

    def per_iter(a, x):
        assert x.sensor is not None and x.cfg.sensor_on()
        assert x.sensor.key() == a.sensor.key()
        for k in ("state", "bias", "ring"):
            assert torch.equal(getattr(a.sensor, k), getattr(x.sensor, k)), k
        # what the policy saw of the last step is not the env's clean obs
        seen = a._raw_obs if a.vecnorm is not None else a.obs[T]
        assert seen.shape == a._clean_obs.shape and not torch.equal(seen, a._clean_obs)
        assert torch.isfinite(a.obs).all()
        assert torch.equal(a.obs, x.obs)
        if a.trunc is not None:
            seen_trunc.append(bool(a.trunc.any()))

    TC.graph_equals_eager_and_resumes(_make(**cfg), tmp_path, field=field, field_shape=shape,
                                      resume_fields=(field,), at_save=at_save, per_iter=per_iter,
                                      resume_into=(_plain(**cfg),))
    if "bootstrap_timeouts" in cfg:
        assert any(seen_trunc)


def test_graph_key_follows_each_setting():
    tr = _make()()
    try:
        keys = {tr._graph_key("rollout")}
        for change in ((lambda env: tr._enable_sensor((0.03,) + NOISE[1:], BIAS, DELAY)),
                       (lambda env: tr._enable_sensor(tr.cfg.obs_noise, (0.0, 0.0, 0.01, 0.0),
                                                      DELAY)),
                       (lambda env: tr._enable_sensor(tr.cfg.obs_noise, tr.cfg.obs_bias, (1, 2)))):
            _, k1 = TC.graph_key_changes(tr, change)
            assert k1 not in keys
            keys.add(k1)
        tr.learn_step()
        assert torch.isfinite(tr.policy.flat).all()
    finally:
        tr.close()


def test_trainer_with_the_defaults_has_no_sensor():
    tr = _plain()()
    try:
        assert tr.sensor is None and not tr.cfg.sensor_on()
        assert not hasattr(tr, "_clean_obs") and not hasattr(tr, "_term_seen")
        assert "sensor" not in tr.state_dict()
        # the rollout graph key of a trainer without the option: the values
        # it held before the option existed, nothing appended
        c = tr.cfg
        assert tr._graph_key("rollout") == \
            (tr.env.seed_value, c.seed, tr.rank, c.num_envs, c.n_steps) + \
            tuple(x for o in reversed(tr.env.option_state()) for x in o)
        tr.learn_step()
    finally:
        tr.close()


def test_sb3_zip_carries_the_settings(tmp_path):
    import zipfile
    from drone_rl_amd import sb3_zip
    a, b = _make()(), _plain()()
    try:
        a.learn_step()
        p = str(tmp_path / "dd.zip")
        a.save_sb3(p)
        with zipfile.ZipFile(p) as z:
            assert sb3_zip.SENSOR_MEMBER in set(z.namelist())
        b.load_sb3(p)
        assert b.sensor is not None and b.sensor.key() == a.sensor.key()
        assert (b.cfg.obs_noise, b.cfg.obs_bias, b.cfg.obs_delay) == (NOISE, BIAS, DELAY)
        b.learn_step()
        assert torch.isfinite(b.policy.flat).all()
    finally:
        a.close()
        b.close()
