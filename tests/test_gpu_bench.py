"""bench.py as it is run for every change: a plain run prints the headline line without the --full measurements, --steps sets
the number of timed steps, and --dump-outputs writes what the last timed step computed."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_plain_run_line_and_dumped_outputs(tmp_path):
    out = tmp_path / "outputs"
    steps, warmup, batch = 3, 1, 32
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup), "--model", "160m",
           "--batch", str(batch), "--memory-size", "0", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in line, key
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["steps"] == steps and line["warmup"] == warmup
    assert line["ms_per_step"] > 0
    assert abs(line["value"] - batch * 1e3 / line["ms_per_step"]) <= 1e-2 * line["value"]
    for key in ("roofline", "kernels", "ddp_forecast", "teacher_cache", "secondary", "image_input", "cpu_baseline"):
        assert key not in line, f"{key} belongs behind --full"

    assert sorted(os.listdir(out)) == ["grad_norm.npy", "loss.npy", "lr.npy", "params_sample.npy"]
    total = 0
    for name in os.listdir(out):
        a = np.load(out / name)
        assert a.dtype in (np.float32, np.float64), (name, a.dtype)
        assert np.isfinite(a).all(), name
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(out / "params_sample.npy").size == 1 << 22
    loss = float(np.load(out / "loss.npy"))
    assert abs(loss - line["final_loss"]) <= 1e-4 * max(1.0, abs(loss))
