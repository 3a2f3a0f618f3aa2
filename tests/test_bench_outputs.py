"""bench.py's plain run and --dump-outputs: the plain run reports the headline
alone, the dump holds the last timed step's outputs (float32 / float64, at
most DUMP_BYTES_MAX) and is the same from run to run, and a run longer than
the resident actions reads them round."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import bench  # noqa: E402

BENCH = os.path.join(ROOT, "bench.py")


def _step_number_actions(monkeypatch):
    import drone_rl_amd

    def fake(n, seed, step, env_id_offset=0, out=None):
        return out.fill_(float(step))
    monkeypatch.setattr(drone_rl_amd, "random_actions", fake)


def test_resident_actions_one_draw_per_step_when_they_fit(monkeypatch):
    _step_number_actions(monkeypatch)
    at = bench.resident_actions(8, 25, 20, 0, "cpu")
    assert at(5, 20).shape == (20, 8, 4)
    assert at(5, 20)[:, 0, 0].tolist() == list(range(5, 25))
    assert at(24)[:, 3, 2].tolist() == [24.0]


def test_resident_actions_are_read_round_past_the_limit(monkeypatch):
    _step_number_actions(monkeypatch)
    monkeypatch.setattr(bench, "ACTION_BYTES_MAX", 7 * 8 * 16)      # 7 draws of 8 envs
    at = bench.resident_actions(8, 100, 4, 0, "cpu")
    for t in range(97):
        for k in (1, 3, 4):
            v = at(t, k)
            assert v.is_contiguous() and v.shape == (k, 8, 4)
            assert v[:, 0, 0].tolist() == [float((t + i) % 7) for i in range(k)], (t, k)


def test_dump_outputs_dtypes_and_seeded_sample(tmp_path, monkeypatch):
    g = torch.Generator().manual_seed(0)
    arr = {"obs": torch.randn(1000, 15, generator=g),
           "done": (torch.rand(1000, generator=g) < 0.1).to(torch.uint8),
           "state_pos": torch.randn(1000, 3, dtype=torch.float64, generator=g)}
    bench.dump_outputs(str(tmp_path / "all"), arr)
    got = {f[:-4]: np.load(tmp_path / "all" / f) for f in os.listdir(tmp_path / "all")}
    assert sorted(got) == ["done", "obs", "state_pos"]
    assert got["obs"].dtype == got["done"].dtype == np.float32
    assert got["state_pos"].dtype == np.float64
    for k, a in got.items():
        assert np.array_equal(a, arr[k].numpy().astype(a.dtype))
    # past the size limit: the same sampled envs every time, their numbers beside them
    per_env = 15 * 4 + 4 + 3 * 8 + 8
    monkeypatch.setattr(bench, "DUMP_BYTES_MAX", 100 * per_env)
    for d in ("s1", "s2"):
        bench.dump_outputs(str(tmp_path / d), arr)
    idx = np.load(tmp_path / "s1" / "env_index.npy")
    assert idx.dtype == np.float64 and len(idx) == 100 and np.all(np.diff(idx) > 0)
    assert np.array_equal(idx, np.load(tmp_path / "s2" / "env_index.npy"))
    total = sum(os.path.getsize(tmp_path / "s1" / f) - 128 for f in os.listdir(tmp_path / "s1"))
    assert total <= 100 * per_env
    assert np.array_equal(np.load(tmp_path / "s1" / "obs.npy"),
                          arr["obs"].numpy()[idx.astype(np.int64)])


def test_extra_without_full_is_refused():
    r = subprocess.run([sys.executable, BENCH, "--extra"], capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 2 and "--full" in r.stderr and not r.stdout.strip()


@pytest.mark.gpu
def test_plain_run_times_the_headline_alone_and_dumps_the_same_outputs_twice(tmp_path):
    lines = []
    for d in ("a", "b"):
        r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "40", "--warmup", "5",
                            "--envs", "4096", "--dump-outputs", str(tmp_path / d)],
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr[-3000:]
        out = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(out) == 1, r.stdout[-3000:]
        lines.append(json.loads(out[0]))
    d = lines[0]
    assert d["steps"] == 40 and d["roofline"]["launches"] == 2      # 32 + 8 steps
    assert d["unit"] == "env-steps/s" and d["higher_is_better"] is True and d["dtype"] == "f64"
    # ms_per_step is rounded to 1e-6 ms: half a unit of it over a step of at least 1e-4 ms
    assert d["ms_per_step"] > 1e-4
    assert d["value"] == pytest.approx(4096 * 1e3 / d["ms_per_step"], rel=5e-3)
    for leg in ("single_step", "cpu_baseline", "companion", "companion_rollout",
                "rollout_kernel", "ppo", "extra"):
        assert leg not in d
    assert "host_floor_us" not in d["roofline"]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(n + ".npy" for n in ("obs", "reward", "done", "state_pos", "state_vel",
                                                "state_euler", "state_omega"))
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and len(a) == 4096
        assert np.array_equal(a, b, equal_nan=True), n
    obs, pos = np.load(tmp_path / "a" / "obs.npy"), np.load(tmp_path / "a" / "state_pos.npy")
    assert obs.shape == (4096, 15) and np.isfinite(obs).all() and np.abs(obs).max() > 0
    assert pos.dtype == np.float64 and set(np.unique(np.load(tmp_path / "a" / "done.npy"))) <= {0, 1}
