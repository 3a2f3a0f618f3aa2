"""One runner for the tests whose body must be a process of its own: the
launch-form overrides (DRONERL_ROLLOUT_WS, DRONERL_ROWS_PER_WAVE,
DRONERL_NT_LOADS) are read once per process or handle."""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_worker(script, *args, timeout=100, **env_overrides):
    """Run tests/<script> with `args` under the environment overrides; it must
    exit 0 and print "ok"."""
    env = dict(os.environ, PYTHONPATH=ROOT, **env_overrides)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", script), *map(str, args)],
                       env=env, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "ok" in r.stdout
