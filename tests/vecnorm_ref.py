"""NumPy f64 restatement of VecNormalize: the contract
the dr_vecnorm_* kernels are tested against.  np.mean / np.var per batch, the
RunningMeanStd update formula, the step order of the spec.  Also the shared
input generator of the vecnorm tests."""
import numpy as np


class RunningMeanStd:
    def __init__(self, shape=()):
        self.count = 1e-4
        self.mean = np.zeros(shape, np.float64)
        self.var = np.ones(shape, np.float64)

    def update(self, x):
        x = np.asarray(x, np.float64)
        bm, bv, bc = np.mean(x, axis=0), np.var(x, axis=0), x.shape[0]
        d = bm - self.mean
        tot = self.count + bc
        self.mean = self.mean + d * bc / tot
        self.var = (self.var * self.count + bv * bc + d * d * self.count * bc / tot) / tot
        self.count = tot


class VecNormalizeRef:
    def __init__(self, n, obs_dim, gamma=0.99, clip_obs=10.0, clip_reward=10.0, epsilon=1e-8,
                 norm_obs=True, norm_reward=True):
        self.n, self.obs_dim = n, obs_dim
        self.gamma, self.clip_obs, self.clip_reward, self.epsilon = (gamma, clip_obs,
                                                                     clip_reward, epsilon)
        self.norm_obs, self.norm_reward = norm_obs, norm_reward
        self.training = True
        self.obs_rms = RunningMeanStd((obs_dim,))
        self.ret_rms = RunningMeanStd(())
        self.returns = np.zeros(n, np.float64)

    def normalize_obs(self, obs):
        """f64 result before the cast (callers compare its f32 rounding)."""
        if not self.norm_obs:
            return np.asarray(obs, np.float64)
        y = (np.asarray(obs, np.float64) - self.obs_rms.mean) / \
            np.sqrt(self.obs_rms.var + self.epsilon)
        return np.clip(y, -self.clip_obs, self.clip_obs)

    def normalize_reward(self, rew):
        if not self.norm_reward:
            return np.asarray(rew, np.float64)
        y = np.asarray(rew, np.float64) / np.sqrt(self.ret_rms.var + self.epsilon)
        return np.clip(y, -self.clip_reward, self.clip_reward)

    def reset(self, obs):
        self.returns[:] = 0.0
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        return self.normalize_obs(obs).astype(np.float32)

    def step(self, obs, rew, done, term_obs=None, term_out=None):
        """Returns (obs_out, rew_out[, term_out]) as f32; term_out (given as
        the buffer to write into) keeps the rows of envs that are not done."""
        done = np.asarray(done).astype(bool)
        if self.training and self.norm_obs:
            self.obs_rms.update(obs)
        obs_out = self.normalize_obs(obs).astype(np.float32)
        if self.training and self.norm_reward:
            self.returns = self.returns * self.gamma + np.asarray(rew, np.float64)
            self.ret_rms.update(self.returns)
        rew_out = self.normalize_reward(rew).astype(np.float32)
        res = (obs_out, rew_out)
        if term_obs is not None:
            to = np.array(term_out, np.float32, copy=True)
            to[done] = self.normalize_obs(term_obs[done]).astype(np.float32)
            res = res + (to,)
        self.returns[done] = 0.0
        return res

    def stats(self):
        """(obs_rms f64[1 + 2 D], ret_rms f64[3]) in the C ABI's layout."""
        o = np.concatenate([[self.obs_rms.count], self.obs_rms.mean, self.obs_rms.var])
        r = np.array([self.ret_rms.count, float(self.ret_rms.mean), float(self.ret_rms.var)])
        return o, r


# ------------------------------------------------------------------- inputs
SENTINEL = np.float32(-777.25)


def make_sequence(n, d, seed, steps=6):
    """A reset and `steps` steps of raw inputs that exercise the spec: column
    scales 1e-3 .. 1e2, offsets up to 100 scales, outliers beyond 10 sigma on
    both sides, one column constant for one step (step 2), step 1 with no env
    done, step 3 with all done, the rest mixed."""
    rng = np.random.default_rng(seed)
    scale = 10.0 ** np.linspace(-3.0, 2.0, d)
    rng.shuffle(scale)
    offset = scale * rng.uniform(-100.0, 100.0, d)

    def obs_batch(k):
        x = rng.standard_normal((n, d)) * scale + offset
        # outliers beyond 10 sigma, both signs (every batch, a few rows)
        m = max(1, n // 64)
        rows = rng.integers(0, n, m)
        cols = rng.integers(0, d, m)
        sign = np.where(np.arange(m) % 2 == 0, 1.0, -1.0)
        x[rows, cols] = offset[cols] + sign * scale[cols] * rng.uniform(30.0, 60.0, m)
        if k == 2:
            x[:, d // 2] = offset[d // 2]
        return x.astype(np.float32)

    seq = {"reset": obs_batch(-1), "steps": []}
    for k in range(steps):
        rew = (rng.standard_normal(n) * 0.7 - 0.3)
        if k == 4 and n >= 2:
            # one reward far out on each side: two rows among all the returns
            # seen so far cannot lift their std to a tenth of this
            rew[0], rew[n - 1] = 1000.0, -1000.0
        if k == 1:
            done = np.zeros(n, np.uint8)
        elif k == 3:
            done = np.ones(n, np.uint8)
        else:
            done = (rng.uniform(size=n) < 0.3).astype(np.uint8)
        seq["steps"].append({"obs": obs_batch(k), "rew": rew.astype(np.float32), "done": done,
                             "term": obs_batch(100 + k)})
    return seq


def ulp_diff(a, b):
    """|a - b| in f32 units in the last place (a, b f32 arrays, finite)."""
    ia = np.asarray(a, np.float32).view(np.int32).astype(np.int64)
    ib = np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, np.int64(-2**31) - ia, ia)
    ib = np.where(ib < 0, np.int64(-2**31) - ib, ib)
    return np.abs(ia - ib)
