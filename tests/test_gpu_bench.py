"""GPU: a plain `bench.py` run (no --full) — one timed region of exactly --steps steps, the headline line without the
measurements that moved behind --full, and --dump-outputs writing what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_plain_run_times_the_given_steps_and_dumps_the_last_steps_outputs(tmp_path):
    argv = ["--steps", "3", "--warmup", "1", "--batch", "2", "--frames", "4", "--height", "64", "--width", "96",
            "--dump-outputs", str(tmp_path)]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + argv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-400:], r.stderr[-1500:])
    lines = [x for x in r.stdout.strip().splitlines() if x.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d["steps"] == 3 and d["warmup"] == 1 and d["repeats"]["n"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "clips/s" and d["value"] > 0 and d["ms_per_step"] > 0 and d["dtype"].startswith("f16")
    assert abs(d["value"] - 2 * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]          # clips/s and ms/step of the same region
    for key in ("roofline", "parity", "cpu_baseline", "bf16_mode", "fp16_mode", "eval_mode"):
        assert key not in d, key
    assert sorted(os.listdir(tmp_path)) == ["logits.npy", "loss.npy", "params_sample.npy"]
    loss, logits, params = (np.load(tmp_path / n) for n in ("loss.npy", "logits.npy", "params_sample.npy"))
    assert loss.dtype == np.float64 and loss.shape == () and abs(float(loss) - d["config"]["final_loss"]) <= 1e-4
    assert logits.dtype == np.float32 and logits.shape == (2, 70) and np.isfinite(logits).all()
    assert params.dtype == np.float32 and params.shape == (1 << 20,) and np.isfinite(params).all()
