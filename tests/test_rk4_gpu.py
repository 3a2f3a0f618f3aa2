"""The "rk4" env variant on the GPU: the gym env's task
on a unit-quaternion attitude advanced by one RK4 step.

The variant is this build's specification (the reference has none).  Every
operation of the law is one correctly rounded IEEE operation in a fixed order
(no trigonometric function, no fused multiply-add), so the kernels are
compared BITWISE with the NumPy restatement tests/rk4_ref.py: done, obs,
reward, terminal obs at every step and every state field at the end, in f64
and f32.  The one allowance: where both sides hold a NaN, its sign and payload
are not compared (IEEE 754 leaves them to the implementation).  Then every
layer above the step kernel: dr_rollout against K dr_step, state access,
masked reset, sharding, the trainer with checkpoints, and the facades."""
import ctypes

import numpy as np
import pytest
import torch

import rk4_ref
from rollout_parity import check_rollout, check_rollout_random
from subproc import run_worker
from trainer_checks import graph_equals_eager_and_resumes, small_trainer

pytestmark = pytest.mark.gpu
DT = {torch.float64: np.float64, torch.float32: np.float32}
MOTOR_MAX = 7.3575


def _batch(n, variant="rk4", **kw):
    from drone_rl_amd import DroneBatch
    return DroneBatch(n, variant, **kw)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize]) if a.dtype.kind == "f" else a


def _assert_same(got, want, what):
    """Bitwise, except that a NaN matches any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype)
    ok = _bits(got) == _bits(want)
    if got.dtype.kind == "f":
        ok |= np.isnan(got) & np.isnan(want)
    if not ok.all():
        bad = np.argwhere(~ok)
        i = tuple(bad[0])
        raise AssertionError(f"{what}: {len(bad)} of {ok.size} differ; first at {i}: "
                             f"{got[i]!r} != {want[i]!r}")


def _tumbling(n, rng, S):
    """Random tumbling states, every value exact in S."""
    s = {"pos": (rng.uniform(-0.5, 0.5, (n, 3)) + [0, 0, 1.0]).astype(S),
         "vel": rng.normal(0, 1, (n, 3)).astype(S),
         "quat": rk4_ref.random_unit_quat(rng, n, S),
         "omega": (5.0 * rng.normal(0, 1, (n, 3))).astype(S),
         "target": (rng.uniform(-1, 1, (n, 3)) + [0, 0, 1.0]).astype(S),
         "step": rng.integers(0, 7, n).astype(np.int32),
         "ep_num": rng.integers(1, 50, n).astype(np.int64),
         "eps": np.round(rng.uniform(0, 1, n), 1)}
    s["ep_num"][::5] = 1999                   # the curriculum bump at the next reset
    return s


def _upload(b, s):
    for k in ("pos", "vel", "omega", "target"):
        b.set(k, s[k].astype(np.float64))
    b.set("quat", s["quat"])
    b.set("current_step", s["step"])
    b.set("ep_num", s["ep_num"].astype(np.int32))
    b.set("eps", s["eps"])


def _assert_state(b, s, S, what):
    for k in ("pos", "vel", "omega", "target"):
        _assert_same(b.get(k).cpu().numpy().astype(S), s[k], f"{what} {k}")
    q = b.get("quat").cpu().numpy()
    assert q.dtype == S
    _assert_same(q, s["quat"], f"{what} quat")
    _assert_same(b.get("current_step").cpu().numpy(), s["step"], f"{what} step")
    _assert_same(b.get("ep_num").cpu().numpy(), s["ep_num"].astype(np.int32), f"{what} ep_num")
    _assert_same(b.get("eps").cpu().numpy(), s["eps"], f"{what} eps")


def _run_against_restatement(b, s, S, steps, rng, max_steps, acts=None):
    n = len(s["pos"])
    resets = 0
    for t in range(steps):
        a = rng.uniform(0, MOTOR_MAX, (n, 4)).astype(np.float32) if acts is None else acts[t]
        u = rng.uniform(0, 1, (n, 5))
        b.set_reset_uniforms(u)
        obs, rew, done = b.step(torch.from_numpy(a).cuda())
        ro, rr, rd, rt = rk4_ref.rk4_env_step(s, a, u, 0.02, max_steps)
        _assert_same(done.cpu().numpy().astype(bool), rd, f"step {t} done")
        _assert_same(rew.cpu().numpy(), rr, f"step {t} reward")
        _assert_same(obs.cpu().numpy(), ro, f"step {t} obs")
        _assert_same(b.term_obs.cpu().numpy()[rd], rt[rd], f"step {t} terminal obs")
        resets += int(rd.sum())
    return resets


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [321, 1])
def test_step_law_vs_restatement(dtype, n):
    """40 free-running steps from random tumbling states with random actions,
    host-uniform resets (the restatement sees the same draws), max_steps 7 so
    that crashes, the step limit and the curriculum bump all occur."""
    S = DT[dtype]
    rng = np.random.default_rng(10 + n)
    s = _tumbling(n, rng, S)
    b = _batch(n, dtype=dtype, rng="host", max_steps=7, keep_terminal_obs=True)
    assert b.obs_dim == 16
    _upload(b, s)
    _assert_state(b, s, S, "upload")
    resets = _run_against_restatement(b, s, S, 40, rng, 7)
    assert resets >= 5 * n
    _assert_state(b, s, S, "final")
    b.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_step_law_on_half_populated_waves(dtype, monkeypatch):
    """The same comparison on the 32-rows-per-wave instance of the step kernel
    (DRONERL_ROWS_PER_WAVE is read when the handle is created), n = 321: ten
    full half-waves and one lane."""
    monkeypatch.setenv("DRONERL_ROWS_PER_WAVE", "32")
    S = DT[dtype]
    n = 321
    rng = np.random.default_rng(77)
    s = _tumbling(n, rng, S)
    b = _batch(n, dtype=dtype, rng="host", max_steps=7, keep_terminal_obs=True, monitor=True)
    _upload(b, s)
    resets = _run_against_restatement(b, s, S, 16, rng, 7)
    assert resets >= 2 * n
    _assert_state(b, s, S, "final")
    b.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_edge_states_vs_restatement(dtype):
    """Gimbal lock, |omega| = 100 rad/s, z one ulp from the ground, |p| at the
    50-m limit, the target at the bonus radius, NaN and inf state, the last
    step before the limit: three steps against the restatement, bitwise."""
    from drone_rl_amd.env import euler_to_quat
    S = DT[dtype]
    hover = np.float32(9.81 / 4)
    tiny = np.nextafter(S(0), S(1))
    ident = [1.0, 0, 0, 0]
    rows = []     # (pos, vel, quat, omega, target, step, action)

    def row(pos=(0, 0, 1), vel=(0, 0, 0), quat=ident, omega=(0, 0, 0), target=(0, 0, 1), step=0,
            act=(hover,) * 4):
        rows.append((pos, vel, quat, omega, target, step, act))
    for yaw in (0.0, 1.0):
        row(quat=euler_to_quat([0.3, np.pi / 2, yaw]), omega=(1, -2, 0.5))
        row(quat=euler_to_quat([0.3, -np.pi / 2, yaw]), omega=(1, -2, 0.5))
    for k in range(3):
        w = [0.0, 0.0, 0.0]
        w[k] = 100.0
        row(omega=w, quat=(0.5, 0.5, 0.5, 0.5))
        row(omega=[-x for x in w], act=(0, MOTOR_MAX, 0, MOTOR_MAX))
    row(omega=(100 / 3 ** 0.5,) * 3, act=(MOTOR_MAX, 0, 0, 0))
    for z in (tiny, -tiny, 0.0, -0.0):
        row(pos=(0, 0, z), act=(0,) * 4)                    # falls: crash
        row(pos=(0, 0, z), act=(MOTOR_MAX,) * 4)            # climbs
    row(pos=(30, 40, 0.001), vel=(0, 0, 1))                 # |p| just past / at 50
    row(pos=(30, 0, 40))
    row(pos=(30, 0, 40), vel=(1, 0, 1))
    row(pos=(30, 0, 40), vel=(-1, 0, -1))
    row(pos=(np.nextafter(S(30), S(0)), 0, 40))
    for d in (0.05, np.nextafter(S(0.05), S(0)), np.nextafter(S(0.05), S(1))):
        row(target=(d, 0, 1))                               # the bonus radius
        row(target=(0, 0, 1 + d), vel=(0, 0, 0.001))
    nan, inf = np.nan, np.inf
    row(pos=(nan, 0, 1))
    row(pos=(0, 0, inf))
    row(pos=(0, 0, -inf))
    row(vel=(inf, 0, 0))
    row(vel=(0, nan, 0))
    row(quat=(nan, 0, 0, 0))
    row(quat=(inf, 0, 0, 0))
    row(omega=(0, inf, 0))
    row(omega=(nan, 0, 0))
    row(target=(nan, 0, 1))
    row(pos=(nan, 0, 1), step=198)                          # NaN ends at the limit only
    row(step=199)
    row(step=198)
    row(step=199, pos=(0, 0, -1))
    n = len(rows)
    s = {"pos": np.array([r[0] for r in rows], S), "vel": np.array([r[1] for r in rows], S),
         "quat": np.array([r[2] for r in rows], np.float64).astype(S),
         "omega": np.array([r[3] for r in rows], S), "target": np.array([r[4] for r in rows], S),
         "step": np.array([r[5] for r in rows], np.int32),
         "ep_num": np.full(n, 3, np.int64), "eps": np.full(n, 0.3)}
    s["ep_num"][::3] = 1999
    acts = np.array([r[6] for r in rows], np.float32)
    rng = np.random.default_rng(2)
    with np.errstate(all="ignore"):
        b = _batch(n, dtype=dtype, rng="host", keep_terminal_obs=True)
        _upload(b, s)
        _assert_state(b, s, S, "upload")
        resets = _run_against_restatement(b, s, S, 3, rng, 200, acts=[acts] * 3)
        assert resets >= 10
        _assert_state(b, s, S, "final")
    b.close()


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
@pytest.mark.parametrize("n", [321, 1000])
def test_rollout_is_bitwise_k_steps(dtype, n):
    """dr_rollout / dr_rollout_random (the one-role kernel, the 13 state words
    in registers) against K = 19 dr_step launches, Philox resets inside the
    launches (max_steps 7), over two back-to-back launches."""
    check_rollout("rk4", n, 19, dtype)
    check_rollout_random("rk4", n, 19, dtype)


@pytest.mark.parametrize("override", [dict(DRONERL_ROLLOUT_WS="1"),
                                      dict(DRONERL_ROWS_PER_WAVE="32", DRONERL_NT_LOADS="1")])
def test_rollout_under_launch_form_overrides(override):
    """DRONERL_ROLLOUT_WS=1 forces the warp-specialised rollout forms for the
    gym variant; this one has only the one-role kernel and must keep it.
    DRONERL_ROWS_PER_WAVE=32 with DRONERL_NT_LOADS=1 puts dr_step on its
    half-populated-wave, nontemporal-load instance (what large batches get);
    the rollout must still equal it bitwise.  The overrides are read once per
    process or handle, hence the subprocess."""
    run_worker("rollout_parity.py", "rk4", "f64", "321", "19", **override)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_state_access(dtype):
    """quat get / gather / set round trip in the state dtype; euler is derived
    on the host; the C call refuses DR_FIELD_EULER here and DR_FIELD_QUAT on
    the gym variant."""
    from drone_rl_amd import _lib
    from drone_rl_amd.env import euler_to_quat
    S = DT[dtype]
    n = 321
    rng = np.random.default_rng(3)
    b = _batch(n, dtype=dtype, seed=4)
    obs = b.reset()
    ident = np.tile(np.array([1, 0, 0, 0], S), (n, 1))
    _assert_same(b.get("quat").cpu().numpy(), ident, "reset quat")
    _assert_same(obs[:, 6:10].cpu().numpy(), ident.astype(np.float32), "reset obs quat")
    q = rk4_ref.random_unit_quat(rng, n, S)
    b.set("quat", q)
    assert b.get("quat").dtype == dtype
    _assert_same(b.get("quat").cpu().numpy(), q, "quat round trip")
    _assert_same(b.get_host("quat"), q, "quat host")
    ids = torch.tensor([5, 320, 0, 64, 63], dtype=torch.int32, device="cuda")
    _assert_same(b.gather("quat", ids).cpu().numpy(), q[[5, 320, 0, 64, 63]], "quat gather")
    # the other fields are untouched by the fourth word's array
    assert torch.equal(b.get("omega"), torch.zeros(n, 3, dtype=torch.float64, device="cuda"))
    # euler: derived
    e = np.stack([rng.uniform(-3, 3, n), rng.uniform(-1.5, 1.5, n), rng.uniform(-3, 3, n)], 1)
    b.set("euler", e)
    _assert_same(b.get("quat").cpu().numpy(), euler_to_quat(e).astype(S), "euler -> quat")
    tol = 1e-12 if S is np.float64 else 2e-5
    np.testing.assert_allclose(b.get("euler").cpu().numpy(), e, rtol=0, atol=tol)
    np.testing.assert_allclose(b.get_host("euler"), e, rtol=0, atol=tol)
    np.testing.assert_allclose(b.gather("euler", ids).cpu().numpy(), e[[5, 320, 0, 64, 63]],
                               rtol=0, atol=tol)
    # the C ABI
    L = _lib.lib()
    buf = torch.zeros(n, 3, dtype=torch.float64, device="cuda")
    fid = _lib.FIELDS["euler"]
    assert L.dr_get_state(b.handle, fid, buf.data_ptr(), None) == _lib.DR_ERR_UNSUPPORTED
    assert "DR_FIELD_QUAT" in _lib.last_error(b.handle)
    assert L.dr_set_state(b.handle, fid, buf.data_ptr(), None) == _lib.DR_ERR_UNSUPPORTED
    assert L.dr_gather_state(b.handle, fid, ids.data_ptr(), 5, buf.data_ptr(), None) == \
        _lib.DR_ERR_UNSUPPORTED
    assert L.dr_obs_dim(b.handle) == 16
    g = _batch(8, "gym")
    qb = torch.zeros(8, 4, dtype=torch.float64, device="cuda")
    for rc in (L.dr_get_state(g.handle, 12, qb.data_ptr(), None),
               L.dr_set_state(g.handle, 12, qb.data_ptr(), None),
               L.dr_gather_state(g.handle, 12, ids.data_ptr(), 1, qb.data_ptr(), None)):
        assert rc == _lib.DR_ERR_INVALID
    with pytest.raises(ValueError):
        g.get("quat")
    torch.cuda.synchronize()
    g.close()
    b.close()


def test_masked_reset():
    n = 321
    rng = np.random.default_rng(5)
    b = _batch(n, seed=7)
    b.reset()
    q = rk4_ref.random_unit_quat(rng, n)
    w = rng.normal(0, 1, (n, 3))
    b.set("quat", q)
    b.set("omega", w)
    mask = torch.from_numpy(rng.uniform(size=n) < 0.5)
    assert 0 < int(mask.sum()) < n
    obs = b.reset_masked(mask).cpu().numpy()
    m = mask.numpy()[:, None]
    want_q = np.where(m, np.array([1.0, 0, 0, 0]), q)
    _assert_same(b.get("quat").cpu().numpy(), want_q, "quat")
    _assert_same(b.get("omega").cpu().numpy(), np.where(m, 0.0, w), "omega")
    _assert_same(obs[:, 6:10], want_q.astype(np.float32), "obs quat")
    _assert_same(obs[:, 10:13], np.where(m, 0.0, w).astype(np.float32), "obs omega")
    b.close()


def test_sharded_equals_unsharded():
    """Two shards at env_id_offset 0 and 321 reproduce one batch of 642: the
    Philox reset and action streams are keyed by the global env id."""
    n = 321
    full = _batch(2 * n, seed=21, max_steps=7)
    full.reset()
    fo, fr, fd = full.rollout(19, None, seed=8, step0=3)
    for j in range(2):
        sh = _batch(n, seed=21, max_steps=7, env_id_offset=j * n)
        sh.reset()
        so, sr, sd = sh.rollout(19, None, seed=8, step0=3)
        sl = slice(j * n, (j + 1) * n)
        assert torch.equal(so, fo[:, sl]) and torch.equal(sr, fr[:, sl])
        assert torch.equal(sd, fd[:, sl])
        for k in ("pos", "quat", "target", "ep_num"):
            assert torch.equal(sh.get(k), full.get(k)[sl]), k
        sh.close()
    assert int(fd.sum()) > 2 * n
    full.close()


# ---- trainer, checkpoints, facades ------------------------------------------
def test_trainer_graph_and_checkpoint(tmp_path):
    """The trainer at obs width 16: the captured rollout graph is bitwise the
    eager rollout; a checkpoint carries `quat` (not `euler`) and resumes bit
    for bit."""
    def make():
        t = small_trainer(num_envs=256, batch_size=1024, variant="rk4")
        assert t.obs.shape[-1] == 16 and t.env.variant == "rk4"
        return t

    def at_save(sd):
        assert "euler" not in sd["env"]

    graph_equals_eager_and_resumes(make, tmp_path, field="quat", field_shape=(256, 4),
                                   resume_fields=("pos", "quat", "omega", "ep_num"),
                                   at_save=at_save)


def test_fused_step_matches_unfused_path_at_width_16():
    """tests/test_smooth_gpu.py's comparison and bounds (width 19) at obs
    width 16, arch (64, 64), m = 1000."""
    from drone_rl_amd import ppo_kernels as K
    from drone_rl_amd.policy import ActorCritic, FusedTrainStep, fusable
    arch, m, od = (64, 64), 1000, 16
    torch.manual_seed(1)
    pol = ActorCritic(od, 4, arch, device="cuda", seed=4)
    assert fusable(pol)
    with torch.no_grad():
        pol.flat.mul_(3.0)
    obs = torch.randn(m, od, device="cuda")
    fs = FusedTrainStep(pol, m)
    with torch.no_grad():
        mean, value, cache = fs.forward(obs)
        d = torch.distributions.Normal(mean, pol.log_std.exp())
        act = d.sample()
        aux = torch.stack([d.log_prob(act).sum(1) + 0.1 * torch.randn(m, device="cuda"),
                           torch.randn(m, device="cuda"), torch.randn(m, device="cuda")], 1)
    L = K.PPOLoss(m, "cuda", 0.2, 0.01, 0.5, True)
    g_mean, g_ls, g_v, st = L(mean, pol.log_std.detach(), value, act, aux=aux)
    ref = fs.backward(obs, cache, g_mean, g_v, g_ls).clone()
    st_ref = st.clone()
    head = K.HeadLossBackward(m, arch[-1], "cuda", 0.2, 0.01, 0.5, True)
    grad, st2 = fs.step(obs, act, aux, head)
    grad = grad.clone()
    for name, _, _ in pol.layout:
        lo, hi, _ = pol.offsets[name]
        scale = ref[lo:hi].abs().max().item() + 1e-12
        assert (grad[lo:hi] - ref[lo:hi]).abs().max().item() <= 2e-4 * scale + 1e-7, name
    assert torch.allclose(st2, st_ref, rtol=1e-4, atol=1e-6)
    grad2, _ = fs.step(obs, act, aux, head)
    assert torch.equal(grad, grad2)


def test_vec_env_facades():
    from drone_rl_amd.vec_env import BatchedDroneVecEnv, DroneVectorEnv
    v = BatchedDroneVecEnv(4, variant="rk4", seed=3)
    assert v.observation_space.shape == (16,)
    obs = v.reset()
    assert obs.shape == (4, 16) and (obs[:, 6:10] == np.float32([1, 0, 0, 0])).all()
    v.set_attr("current_step", 199, indices=[1, 3])
    act = np.array([[0, 3, 0, 3]] * 4, np.float32)          # a yaw torque
    obs, rew, done, infos = v.step(act)
    assert obs.shape == (4, 16) and list(done) == [False, True, False, True]
    for i in (1, 3):
        t = infos[i]["terminal_observation"]
        assert t.shape == (16,) and t[9] != 0 and t[6] < 1      # turned about body z
        assert (obs[i, 6:10] == np.float32([1, 0, 0, 0])).all()
        assert infos[i]["episode"]["l"] == 1
    assert "terminal_observation" not in infos[0]
    quat = v.get_attr("quat")
    assert len(quat) == 4 and quat[0].shape == (4,)
    assert (np.stack(quat).astype(np.float32) == obs[:, 6:10]).all()
    assert len(v.get_attr("euler")) == 4 and v.get_attr("euler")[0].shape == (3,)
    v.close()
    g = BatchedDroneVecEnv(4, variant="gym", seed=3)
    with pytest.raises(AttributeError):
        g.get_attr("quat")
    g.close()
    e = DroneVectorEnv(4, seed=3, variant="rk4")
    assert e.single_observation_space.shape == (16,) and e.observation_space.shape == (4, 16)
    o, _ = e.reset()
    assert o.shape == (4, 16)
    o, r, term, trunc, _ = e.step(act)
    assert o.shape == (4, 16) and not term.any()
    e.close()
