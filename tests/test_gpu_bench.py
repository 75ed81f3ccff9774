"""bench.py's plain run past the step where training on its resident windows would reach the ces loss's 0 * log(0)
(bench.REWIND_EVERY): every output of the last timed step stays finite, and the line carries the contract fields."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_long_plain_run_dumps_finite_outputs(dev, tmp_path):
    steps = 400                                   # > 2x the first non-finite step without the rewind (179)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "3",
           "--dump-outputs", str(tmp_path)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=240, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["steps"] == steps and line["ms_per_step"] > 0 and line["higher_is_better"] is True
    assert not {"roofline", "extra", "cpu_baseline"} & set(line)
    files = sorted(os.listdir(tmp_path))
    assert files == ["grads.npy", "params.npy", "per_slide_loss.npy", "risk.npy"]
    for f in files:
        x = np.load(tmp_path / f)
        assert x.dtype == np.float32 and x.size > 0 and np.isfinite(x).all(), f
