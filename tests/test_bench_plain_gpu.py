"""A plain `python bench.py --gpus 1 --steps K --warmup W` does only what its headline needs: it sets up, warms up, times the K
steps, writes --dump-outputs and prints ONE JSON line - without the measurements and checks that `--full` adds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")
FULL_ONLY = ("value_over_90_steps", "value_sustained", "latency_ms_single_stream", "roofline", "roofline_neuron", "attention_gemm",
             "attention_gemm_roofline_frac", "config3_ann", "side_measurements", "cpu_baseline", "gpu_over_cpu", "headline_summary")


@pytest.mark.gpu
def test_plain_run_prints_the_headline_alone(tmp_path):
    out = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "20", "--warmup", "5", "--dump-outputs", str(tmp_path)],
                         capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    r = json.loads(lines[0])
    assert r["metric"] == "event-frames/sec fwd (1x10x2x288x384)" and r["unit"] == "samples/s" and r["higher_is_better"] is True
    assert r["dtype"] == "f16x2" and r["n_gpus"] == 1 and r["steps"] == 20 and r["warmup"] == 5
    assert r["value"] > 0 and abs(r["value"] - 20 / (r["ms_per_step"] * 20e-3)) < 1e-6 * r["value"]
    assert not [k for k in FULL_ONLY if k in r]
    # the last launch sequence of the timed region: 20 samples dealt to 2 streams of 10 -> one 10-sample sequence, four flow maps
    flows = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npy"))
    assert flows == [f"flow{i}.npy" for i in range(4)]
    for f in flows:
        a = np.load(tmp_path / f)
        assert a.dtype == np.float32 and a.shape[:2] == (10, 2) and np.isfinite(a).all()
