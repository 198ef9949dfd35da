"""bench.py's plain run: the result line, exactly --steps timed steps, nothing beyond the headline figure, and --dump-outputs
giving the same outputs from run to run (same arguments -> same inputs; the timed path is deterministic)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(tmp_path, tag, steps, warmup):
    out = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", str(warmup),
           "--batch", "2", "--dump-outputs", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), out


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    res, out = _bench(tmp_path, "a", steps=2, warmup=1)
    assert res["steps"] == 2 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["unit"] == "slices/s" and res["higher_is_better"] is True and res["dtype"].startswith("bf16")
    assert res["ms_per_step"] > 0 and abs(res["value"] - 2 * 1e3 / res["ms_per_step"]) < 1e-2 * res["value"]
    for k in ("roofline", "cpu_baseline", "fp16_mode", "fp32s_parity_mode", "fp32_parity_mode", "fp8_25step", "ancestral_config3",
              "latency_b1"):
        assert k not in res, k                                      # the legs of --full only
    assert res["h2d_inclusive"] is None and res["box_during_untimed_replay"] is None
    got = {n: np.load(out / f"{n}.npy") for n in ("denoised", "noisy_input")}
    for n, a in got.items():
        assert a.dtype == np.float32 and a.shape == (2, 1, 512, 512) and np.isfinite(a).all(), n
    # another step count, same arguments otherwise: the same inputs, the same outputs bit for bit
    _, out2 = _bench(tmp_path, "b", steps=1, warmup=0)
    for n, a in got.items():
        assert np.array_equal(np.load(out2 / f"{n}.npy"), a), n
