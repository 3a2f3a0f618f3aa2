"""VecNormalize inside PPOTrainer: the rollout's
buffers against the NumPy restatement fed the recorded raw env outputs, the
captured rollout against the eager one, and checkpoints."""
import numpy as np
import pytest
import torch

from vecnorm_ref import VecNormalizeRef, ulp_diff

pytestmark = pytest.mark.gpu

N, T, EPS = 256, 8, 1e-8


def _trainer(graph=True, **kw):
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    base = dict(num_envs=N, n_steps=T, batch_size=512, n_epochs=2, seed=3,
                normalize_obs=True, normalize_reward=True)
    base.update(kw)
    tr = PPOTrainer(PPOConfig(**base))
    tr.rollout_graph = graph
    return tr


def _state(tr):
    out = {"flat": tr.policy.flat.detach().clone(), "obs": tr.obs.clone(),
           "rewards": tr.rewards.clone(), "m": tr.opt.m.clone(), "v": tr.opt.v.clone()}
    if tr.vecnorm is not None:
        out.update(obs_rms=tr.vecnorm.obs_rms.clone(), ret_rms=tr.vecnorm.ret_rms.clone(),
                   returns=tr.vecnorm.returns.clone())
    return out


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert torch.equal(a[k], b[k]), k


def test_rollout_buffers_follow_the_restatement(monkeypatch):
    from drone_rl_amd import ppo_kernels as K
    rec = {"reset": [], "step": []}
    reset0, step0 = K.VecNormalize.reset, K.VecNormalize.step

    def reset(self, obs, out=None):
        rec["reset"].append(obs.cpu().numpy().copy())
        return reset0(self, obs, out=out)

    def step(self, obs, rew, done, term_obs=None, **kw):
        rec["step"].append((obs.cpu().numpy().copy(), rew.cpu().numpy().copy(),
                            done.cpu().numpy().copy()))
        return step0(self, obs, rew, done, term_obs, **kw)

    monkeypatch.setattr(K.VecNormalize, "reset", reset)
    monkeypatch.setattr(K.VecNormalize, "step", step)
    tr = _trainer(graph=False)
    try:
        od = tr.env.obs_dim
        tr.collect_rollouts()
        torch.cuda.synchronize()
        assert len(rec["reset"]) == 1 and len(rec["step"]) == T
        ref = VecNormalizeRef(N, od, gamma=tr.cfg.gamma, epsilon=EPS)
        differ = total = 0
        want = [ref.reset(rec["reset"][0])]
        rews = []
        for obs, rew, done in rec["step"]:
            o, r = ref.step(obs, rew, done)
            want.append(o)
            rews.append(r)
        for got, exp in ((tr.obs.cpu().numpy(), np.stack(want)),
                         (tr.rewards.cpu().numpy(), np.stack(rews))):
            u = ulp_diff(got, exp)
            assert u.max() <= 1
            differ += int((u != 0).sum())
            total += u.size
        assert differ <= 1e-3 * total
        o_ref, r_ref = ref.stats()
        o, r = tr.vecnorm.obs_rms.cpu().numpy(), tr.vecnorm.ret_rms.cpu().numpy()
        assert o[0] == o_ref[0] == 1e-4 + (T + 1) * N and r[0] == r_ref[0] == 1e-4 + T * N
        mean_ref, var_ref = o_ref[1:1 + od], o_ref[1 + od:]
        assert np.all(np.abs(o[1:1 + od] - mean_ref) <= 1e-12 * np.sqrt(var_ref + EPS))
        assert np.all(np.abs(o[1 + od:] - var_ref) <= 1e-12 * (var_ref + EPS))
        assert abs(r[1] - r_ref[1]) <= 1e-12 * np.sqrt(r_ref[2] + EPS)
        assert abs(r[2] - r_ref[2]) <= 1e-12 * (r_ref[2] + EPS)
        # the buffers hold normalised rewards; the monitor's running episode
        # return stays raw: envs that never ended carry the raw rewards' sum
        raw = np.stack([r for _, r, _ in rec["step"]])
        assert not np.array_equal(raw, tr.rewards.cpu().numpy())
        alive = ~np.stack([d for _, _, d in rec["step"]]).astype(bool).any(0)
        assert alive.any()
        ep_ret = tr.env.get("ep_return").cpu().numpy()
        assert np.allclose(ep_ret[alive], raw.sum(0)[alive], rtol=1e-5, atol=1e-6)
    finally:
        tr.close()


def test_captured_rollout_equals_eager_bitwise():
    a, b = _trainer(graph=False), _trainer(graph=True)
    try:
        for it in range(3):       # b: eager warm-up, capture + replay, replay
            a.learn_step()
            b.learn_step()
            torch.cuda.synchronize()
            _same(_state(a), _state(b))
        assert a._rgraph is None and b._rgraph is not None
    finally:
        a.close()
        b.close()


def test_resume_is_bitwise_and_a_checkpoint_enables_the_option(tmp_path):
    a = _trainer()
    b = _trainer()
    c = _trainer(normalize_obs=False, normalize_reward=False)
    try:
        assert c.vecnorm is None
        for _ in range(2):
            a.learn_step()
        p = str(tmp_path / "ck.pt")
        a.save(p)
        sd = torch.load(p, map_location="cpu", weights_only=True)
        assert "vecnorm" in sd and sd["config"]["normalize_obs"] is True
        a.learn_step()
        b.load(p)
        b.learn_step()
        # a trainer built without the option takes the checkpoint's
        c.load(p)
        assert c.vecnorm is not None and c.vecnorm.norm_obs and c.vecnorm.norm_reward
        assert c.cfg.normalize_obs and c.cfg.normalize_reward
        c.learn_step()
        torch.cuda.synchronize()
        _same(_state(a), _state(b))
        _same(_state(a), _state(c))
    finally:
        for t in (a, b, c):
            t.close()


def test_trainer_without_normalisation_has_no_vecnorm():
    tr = _trainer(normalize_obs=False, normalize_reward=False)
    try:
        assert tr.vecnorm is None
        assert not hasattr(tr, "_raw_obs") and not hasattr(tr, "_raw_rew")
        assert "vecnorm" not in tr.state_dict()
        tr.learn_step()
    finally:
        tr.close()


def test_sb3_zip_carries_the_statistics(tmp_path):
    import zipfile
    from drone_rl_amd import sb3_zip
    a = _trainer()
    b = _trainer(normalize_obs=False, normalize_reward=False)
    try:
        a.learn_step()
        p = str(tmp_path / "dd.zip")
        a.save_sb3(p)
        with zipfile.ZipFile(p) as z:
            assert {"dronerl_env_state.npz", sb3_zip.VECNORM_MEMBER} <= set(z.namelist())
        stats = (a.vecnorm.obs_rms.clone(), a.vecnorm.ret_rms.clone())
        b.load_sb3(p)
        assert b.vecnorm is not None
        # load_sb3's reset went through the normaliser: one more batch of N rows
        assert float(b.vecnorm.obs_rms[0]) == float(stats[0][0]) + N
        assert torch.equal(b.vecnorm.ret_rms, stats[1])
        assert torch.isfinite(b.vecnorm.obs_rms).all()
        b.learn_step()
        assert torch.isfinite(b.policy.flat).all()
    finally:
        a.close()
        b.close()


def test_bootstrap_timeouts_take_the_value_of_the_normalised_terminal_obs():
    tr = _trainer(graph=False, bootstrap_timeouts=True, n_epochs=1)
    try:
        # every env one step short of the limit: the first step truncates all
        tr.env.set("current_step", torch.full((N,), 199, dtype=torch.int32))
        tr.collect_rollouts()
        torch.cuda.synchronize()
        assert tr.trunc[0].bool().all() and tr.dones[1].bool().all()
        vn = tr.vecnorm
        assert torch.isfinite(tr.rewards).all()
        # envs that did not end again still hold step 0's terminal rows: the
        # normalised terminal obs, not the raw one
        keep = ~tr.dones[2:].bool().any(0)
        assert keep.any()
        assert (tr._term_norm.abs() <= vn.clip_obs).all()
        assert not torch.allclose(tr._term_norm[keep], tr.env.term_obs[keep], rtol=0.1, atol=0.1)
    finally:
        tr.close()
