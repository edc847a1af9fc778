"""bench.py --dump-outputs on the CPU test double (one rank, tiny model): the arrays a caller of the timed path receives
after its last step are written as float32 / float64 .npy files, and two runs with the same arguments write the same
values.  A plain run (no --full) reports every sub-record as null."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAUNCHER = os.path.join(ROOT, "tests", "_bench_gloo_double.py")


def _run(tmp_path, tag, extra=()):
    out = tmp_path / tag
    env = dict(os.environ, OMP_NUM_THREADS="2", CUDA_VISIBLE_DEVICES="", HIP_VISIBLE_DEVICES="")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "STYLEX_FORCE_DDP"):
        env.pop(k, None)
    cmd = [sys.executable, LAUNCHER, "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "2", "--image-size", "32",
           "--network-capacity", "2", "--fmap-max", "16", "--workdir", str(tmp_path / ("work_" + tag)),
           "--dump-outputs", str(out)] + list(extra)
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


@pytest.mark.timeout(900)
def test_bench_dump_outputs_are_written_and_reproducible(tmp_path):
    j, a = _run(tmp_path, "a")
    _, b = _run(tmp_path, "b")
    assert j["steps"] == 2 and j["ms_per_step"] > 0 and j["full"] is False
    for k in ("roofline", "cpu_baseline", "fp32_parity_mode", "bench_a", "frozen_nets"):
        assert j[k] is None, k
    names = sorted(f for f in os.listdir(a) if f.endswith(".npy"))
    assert names == ["D.npy", "G.npy", "S.npy", "encoder.npy", "losses.npy"], names
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert x.size > 0 and x.shape == y.shape, n
        np.testing.assert_array_equal(x, y, err_msg=n)
        total += os.path.getsize(a / n)
    assert total <= 64 << 20
    losses = np.load(a / "losses.npy")
    assert losses.shape == (5,) and np.isfinite(losses[:2]).all()
