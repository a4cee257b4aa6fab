"""-m gpu: bench.py's plain line (`--gpus 1 --steps K --warmup W`, no --full) and --dump-outputs.  The plain line carries the headline
keys with `steps` = K and none of the --full sections; the dump holds the forecast fields of the last timed step as float32 .npy files,
finite, within the size bound, and equal in a second run with the same arguments (fixed inputs, weights and dropout seed)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(out_dir, steps, nb=4):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--nb", str(nb), "--dump-outputs", out_dir]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, f"rc {r.returncode}\n--- stdout\n{r.stdout[-3000:]}\n--- stderr\n{r.stderr[-6000:]}"
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_bench_line_and_dumped_outputs_repeat(tmp_path):
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    res = _plain_run(a, steps=3)
    assert res["metric"] == "sampled fields/sec (h-step rollout)" and res["unit"] == "fields/s" and res["higher_is_better"] is True
    assert res["dtype"] == "bf16" and res["steps"] == 3 and res["warmup"] == 1 and res["n_gpus"] == 1
    assert res["value"] > 0 and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(4 * 16 * 1e3 / res["ms_per_step"], rel=1e-3)  # value and ms_per_step describe the same steps
    for key in ("roofline", "hbm_kernels", "batch_curve", "config2_oisst", "train_step", "cpu_baseline"):
        assert key not in res, key

    names = sorted(os.listdir(a))
    assert names == sorted(f"t{i}_preds.npy" for i in range(1, 17)), names
    assert sum(os.path.getsize(os.path.join(a, n)) for n in names) <= 64_000_000
    _plain_run(b, steps=3)
    assert sorted(os.listdir(b)) == names
    for n in names:
        x, y = np.load(os.path.join(a, n)), np.load(os.path.join(b, n))
        assert x.dtype == np.float32 and x.shape == (4, 3, 221, 42), (n, x.dtype, x.shape)
        assert np.isfinite(x).all(), n
        assert np.array_equal(x, y), (n, float(np.abs(x - y).max()))
