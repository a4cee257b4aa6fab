"""The references of the per-segment ensemble metrics (dyf_trajectory_metrics), on the CPU:

  * tests/golden/trajmetrics_{a,b,c}.npz hold what the reference's own functions give per horizon step of a trajectory
    (tests/golden/make_golden_trajectory_metrics.py); the per-segment reference of the GPU tests, oracle/metrics.py applied to
    the slices preds[:, s] / targets[s], is pinned to them at the tolerance of tests/test_oracle_metrics.py;
  * where the reference checkout is present the fixtures regenerate bit for bit;
  * the key layout of the test epoch; header, ctypes table and ABI version.
"""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from oracle import metrics as om

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {"trajmetrics_a.npz": (5, 4, 2, 2, 7, 6), "trajmetrics_b.npz": (20, 3, 1, 3, 13, 9), "trajmetrics_c.npz": (1, 2, 2, 1, 5, 5)}

needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference/src"),
                                     reason="the reference checkout is only present in the build container")


@pytest.mark.parametrize("name", sorted(FILES))
def test_oracle_per_slice_matches_the_reference_curves(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        preds, targets, mse, ssr = z["preds"], z["targets"], z["mse"], z["ssr"]
    n, t = FILES[name][:2]
    assert preds.shape == FILES[name] and targets.shape == FILES[name][1:] and preds.dtype == targets.dtype == np.float32
    assert mse.shape == ssr.shape == (t,)
    assert os.path.getsize(os.path.join(GOLDEN, name)) < 1_000_000
    for s in range(t):
        ref = om.evaluate_ensemble_prediction(preds[:, s], targets[s])
        assert ref["mse"] == pytest.approx(float(mse[s]), rel=1e-6), s
        assert ref["ssr"] == pytest.approx(float(ssr[s]), rel=1e-6), s
        if n == 1:
            assert ref["ssr"] == 0.0 and float(ssr[s]) == 0.0
    if t > 1:  # the segments differ: a kernel that mixed them up would not pass
        assert len(set(np.round(mse, 6).tolist())) == t


@needs_reference
def test_trajectory_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DYF_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="4242")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_trajectory_metrics.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)
    for name in FILES:
        with np.load(os.path.join(tmp_path, name), allow_pickle=False) as x, np.load(os.path.join(GOLDEN, name), allow_pickle=False) as y:
            assert sorted(x.files) == sorted(y.files) == ["mse", "preds", "ssr", "targets"], name
            for k in x.files:
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (name, k)
                assert np.array_equal(x[k], y[k]), (name, k)


def test_test_epoch_key_layout():
    from dyffusion_amd.metrics import trajectory_metric_keys

    curves = {"ssr": np.array([1.0, 2.0, 6.0]), "crps": np.array([0.5, 0.25, 0.75]), "mse": np.array([4.0, 4.0, 1.0])}
    out = trajectory_metric_keys("50ens_mems/", curves, "")
    want = {"test/50ens_mems/avg/ssr": 3.0, "test/50ens_mems/avg/crps": 0.5, "test/50ens_mems/avg/mse": 3.0}
    for i in range(3):
        for m, v in curves.items():
            want[f"test/50ens_mems/t{i + 1}/{m}"] = float(v[i])
    assert out == want and len(out) == 12
    assert all(isinstance(v, float) for v in out.values())
    named = trajectory_metric_keys("50ens_mems/", curves, "test_hard")
    assert set(named) == {k.replace("test/", "test/test_hard/", 1) for k in want}
    assert named["test/test_hard/50ens_mems/avg/mse"] == 3.0 and named["test/test_hard/50ens_mems/t3/ssr"] == 6.0
    assert trajectory_metric_keys("", {"mse": np.array([2.0])}, "") == {"test/avg/mse": 2.0, "test/t1/mse": 2.0}
    assert trajectory_metric_keys("4ens_mems/", {}, "x") == {}


def test_header_binding_and_abi_version_agree():
    from dyffusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "dyffusion_hip.h")).read()
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", hdr, re.M) and _lib.DYF_ABI_VERSION == 9
    m = re.search(r"dyf_status\s+dyf_trajectory_metrics\s*\(([^;]*)\)\s*;", hdr)
    assert m, "dyf_trajectory_metrics is not declared in include/dyffusion_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10 and params[0].startswith("dyf_engine*") and params[-1].startswith("void* stream")
    rows = [s for s in _lib.SYMBOLS if s[0] == "dyf_trajectory_metrics"]
    assert len(rows) == 1 and len(rows[0][2]) == len(params)
    # int32 n_segments, int32 n_members, int64 n_points, int64 member_stride sit where the header has them
    import ctypes as C
    for i, p in enumerate(params):
        if p.startswith("int32_t"):
            assert rows[0][2][i] is C.c_int32, p
        if p.startswith("int64_t"):
            assert rows[0][2][i] is C.c_int64, p
