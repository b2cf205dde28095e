"""bench.py's plain run end to end: the headline line, the dumped outputs, and none of what only --full measures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_plain_run_is_headline_only(dev, tmp_path):
    sys.path.insert(0, ROOT)
    import bench

    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--dump-outputs", str(tmp_path)]
    p = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [l for l in p.stdout.splitlines() if l.startswith("{")][-1]
    out = json.loads(line)
    for k in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "steps", "warmup", "n_gpus"):
        assert k in out, k
    assert out["steps"] == 3 and out["warmup"] == 1 and out["n_gpus"] == 1 and out["unit"] == "TOPS" and out["higher_is_better"] is True
    assert out["value"] > 0 and out["ms_per_step"] > 0
    for k in ("per_m", "per_m_g128", "roofline", "roofline_hbm", "llama7b", "cpu_baseline", "eager_ms_per_step", "step_us_median", "detail"):
        assert k not in out, k
    for M in bench.SWEEP_M:
        d = np.load(tmp_path / f"D_m{M}.npy")
        assert d.dtype == np.float32 and d.shape == (len(bench.dump_rows(M)), bench.N_FULL)
        assert np.isfinite(d).all() and np.abs(d).max() > 0
