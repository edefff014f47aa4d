"""bench.py end to end on the GPU at a small batch: a plain run prints the headline line only (and --dump-outputs),
--full adds the figures measured beside it."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("frontend", "frontend_qscan", "q_adapter", "pooled_classify", "dora_step_ms", "dora_step", "extra",
             "kernels", "roofline", "cpu_baseline")


def _bench(*argv):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--batch", "8", "--steps", "2",
                        "--warmup", "1", *argv], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_only(tmp_path):
    line = _bench("--dump-outputs", str(tmp_path))
    assert line["metric"] == "1s-strain segments/sec (encoder fwd)" and line["unit"] == "segments/s"
    assert line["higher_is_better"] is True and line["dtype"] == "bf16" and line["full"] is False
    assert (line["steps"], line["warmup"], line["n_gpus"]) == (2, 1, 1)
    assert line["value"] == pytest.approx(8 / line["ms_per_step"] * 1e3, rel=1e-9)
    assert not [k for k in FULL_ONLY if k in line]
    last = np.load(tmp_path / "last_token.npy")
    assert last.shape == (8, 384) and np.isfinite(last).all()


def test_full_run_adds_the_figures_beside_the_headline():
    line = _bench("--full", "--no-cpu-baseline", "--no-train", "--no-extra")
    assert line["full"] is True and line["value"] > 0
    for k in ("frontend", "frontend_qscan", "q_adapter", "pooled_classify", "kernels", "roofline"):
        assert line[k], k
    assert line["dora_step"] is None and line["extra"] is None and "cpu_baseline" not in line
