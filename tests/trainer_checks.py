"""The trainer checks that every env variant and option repeats: the small
configurations, "the captured rollout graph is the eager rollout and a
checkpoint resumes bit for bit", and "the graph key follows the option".  The
option-specific asserts stay with the tests, passed in as hooks."""
import torch


def small_trainer(**cfg):
    """2048 envs x 16 steps, batch 4096, 2 epochs, (64, 64), seed 5, with
    `cfg` on top."""
    from drone_rl_amd.ppo import PPOConfig, PPOTrainer
    return PPOTrainer(PPOConfig(**dict(dict(num_envs=2048, n_steps=16, batch_size=4096,
                                            n_epochs=2, net_arch=(64, 64), seed=5), **cfg)))


def plain_trainer():
    """The plain gym trainer of the graph-key tests: 256 envs x 4 steps."""
    return small_trainer(num_envs=256, n_steps=4, batch_size=1024, n_epochs=1)


def graph_equals_eager_and_resumes(make, tmp_path, *, field, field_shape, resume_fields,
                                   at_save=None, per_iter=None, after=None, resume_into=None):
    """Two trainers from make(), one with the rollout graph off, agree bitwise
    over three learn_steps; the state_dict before the third carries `field`
    with `field_shape` (at_save(sd) checks the rest) and is saved; a fresh
    make() and every constructor in `resume_into` load it, hold the saved
    field, and after one learn_step equal the first trainer in the policy,
    `resume_fields` and num_timesteps.  per_iter(a, x) runs after every
    learn_step of a second trainer x, the resumed ones included; after(a, b)
    once the three iterations are done."""
    a, b = make(), make()
    b.rollout_graph = False
    path = tmp_path / "ck.pt"
    for it in range(3):
        if it == 2:
            sd = a.state_dict()
            assert field in sd["env"] and sd["env"][field].shape == field_shape
            if at_save is not None:
                at_save(sd)
            a.save(path)
        sa, sb = a.learn_step(), b.learn_step()
        assert torch.isfinite(sa).all() and torch.equal(sa, sb)
        for name in ("obs", "actions", "rewards", "dones", "adv"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (it, name)
        if per_iter is not None:
            per_iter(a, b)
    assert a._rgraph is not None and b._rgraph is None
    assert torch.isfinite(a.policy.flat).all()
    if after is not None:
        after(a, b)
    saved = torch.load(path, weights_only=True)["env"][field].to("cuda")
    for build in (make,) + tuple(resume_into or ()):
        c = build()
        c.load(path)
        assert torch.equal(c.env.get(field), saved)
        c.learn_step()
        assert torch.equal(a.policy.flat.detach(), c.policy.flat.detach())
        for k in resume_fields:
            assert torch.equal(a.env.get(k), c.env.get(k)), k
        assert a.num_timesteps == c.num_timesteps
        if per_iter is not None:
            per_iter(a, c)
        c.close()
    for t in (a, b):
        t.close()


def graph_key_changes(trainer, change):
    """change(trainer.env) must change the captured rollout graph's key.
    Returns the key before and after."""
    k0 = trainer._graph_key("rollout")
    change(trainer.env)
    k1 = trainer._graph_key("rollout")
    assert k1 != k0
    return k0, k1
