"""bench.py's plain run on the GPU: one JSON line whose `steps` / `ms_per_step` describe the timed steps, none of the
--full keys, and --dump-outputs files that do not depend on how many untimed prewarm steps the run took."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_bench_line_and_repeatable_dump(tmp_path):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "7", "--warmup", "3", "--envs", "256"]
    lines = []
    for name, prewarm_ms in (("a", "0"), ("b", "20")):
        out = subprocess.run(cmd + ["--prewarm-ms", prewarm_ms, "--dump-outputs", str(tmp_path / name)],
                             capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        assert len(out.stdout.splitlines()) == 1, out.stdout
        lines.append(json.loads(out.stdout))
    for d in lines:
        assert d["steps"] == 7 and d["warmup"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0
        assert d["metric"] == "agent-steps/sec" and d["unit"] == "agent-steps/s" and d["higher_is_better"] is True
        assert "cpu_baseline" not in d and "other_configs" not in d
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert names == ["a_prior.npy", "done.npy", "dp.npy", "obs.npy", "p.npy", "reward.npy", "rows.npy"]
    for f in names:
        a, b = np.load(str(tmp_path / "a" / f)), np.load(str(tmp_path / "b" / f))
        assert a.dtype in (np.float32, np.float64) and a.shape[0] == 256 * 64
        assert np.array_equal(a, b), f
