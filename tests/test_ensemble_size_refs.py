"""The references of the ensemble-size metrics (dyf_ensemble_size_metrics), on the CPU:

  * tests/golden/enssize_{a,b,c}.npz hold what the reference's own functions give for the ensembles of the first n members and
    for every member's own MSE (tests/golden/make_golden_ensemble_size.py); the per-prefix reference of the GPU tests
    (tests/ensemble_size_refs.py) is pinned to them at the tolerance of tests/test_trajectory_metrics_refs.py;
  * where the reference checkout is present the fixtures regenerate bit for bit;
  * header, ctypes table and ABI version; the host surface that needs no GPU: argument checks, names, the key layout.
"""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ensemble_size_refs as refs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {"enssize_a.npz": (6, 2, 2, 7, 6), "enssize_b.npz": (20, 1, 3, 13, 9), "enssize_c.npz": (1, 2, 1, 5, 5)}
KEYS = ["mse", "mse_per_mem", "mse_per_mem_mean", "preds", "ssr", "targets"]

needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference/src"),
                                     reason="the reference checkout is only present in the build container")


@pytest.mark.parametrize("name", sorted(FILES))
def test_prefix_reference_matches_the_reference_per_ensemble_size(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        assert sorted(z.files) == KEYS
        preds, targets, mse, ssr, per_mem, per_mem_mean = (z[k] for k in ("preds", "targets", "mse", "ssr", "mse_per_mem",
                                                                          "mse_per_mem_mean"))
    n = FILES[name][0]
    assert preds.shape == FILES[name] and targets.shape == FILES[name][1:] and preds.dtype == targets.dtype == np.float32
    assert mse.shape == ssr.shape == per_mem.shape == (n,) and per_mem_mean.shape == ()
    assert os.path.getsize(os.path.join(GOLDEN, name)) < 1_000_000
    ref = refs.prefix_reference(preds, targets)
    assert ref.shape == (4, n) and ref.dtype == np.float64
    assert ref[1, 0] == 0.0 and float(ssr[0]) == 0.0  # one member: zero spread, exactly
    assert ref[2, 0] == pytest.approx(float(np.mean(np.abs(preds[0].astype(np.float64) - targets))), rel=1e-12)  # crps[1]: MAE of member 0
    for k in range(n):
        assert ref[0, k] == pytest.approx(float(mse[k]), rel=1e-6), k
        assert ref[3, k] == pytest.approx(float(per_mem[k]), rel=1e-6), k
        if k > 0:
            assert ref[1, k] == pytest.approx(float(ssr[k]), rel=1e-6), k
    assert ref[3].mean() == pytest.approx(float(per_mem_mean), rel=1e-6)
    assert ref[0, 0] == pytest.approx(ref[3, 0], rel=1e-6)  # the one-member ensemble's mse is member 0's own
    if n > 2:  # the prefixes differ, and so do the members: a kernel that kept only the last value would not pass
        assert len(set(np.round(mse, 6).tolist())) == n and len(set(np.round(per_mem, 6).tolist())) == n


def test_segment_reference_is_the_prefix_reference_of_every_segment():
    rng = np.random.default_rng(3)
    truth = rng.normal(size=(3, 11)).astype(np.float32)
    preds = (truth[None] * 0.7 + 0.5 * rng.normal(size=(4, 3, 11))).astype(np.float32)
    seg = refs.segment_reference(preds, truth)
    assert seg.shape == (4, 3, 4)
    for s in range(3):
        assert np.array_equal(seg[:, s], refs.prefix_reference(preds[:, s][:, None], truth[s][None]))


@needs_reference
def test_ensemble_size_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DYF_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="4242")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_ensemble_size.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)
    for name in FILES:
        with np.load(os.path.join(tmp_path, name), allow_pickle=False) as x, np.load(os.path.join(GOLDEN, name), allow_pickle=False) as y:
            assert sorted(x.files) == sorted(y.files) == KEYS, name
            for k in x.files:
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (name, k)
                assert np.array_equal(x[k], y[k]), (name, k)


def test_header_binding_and_abi_version_agree():
    from dyffusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "dyffusion_hip.h")).read()
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", hdr, re.M) and _lib.DYF_ABI_VERSION == 9
    m = re.search(r"dyf_status\s+dyf_ensemble_size_metrics\s*\(([^;]*)\)\s*;", hdr)
    assert m, "dyf_ensemble_size_metrics is not declared in include/dyffusion_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 10 and params[0].startswith("dyf_engine*") and params[-1].startswith("void* stream")
    rows = [s for s in _lib.SYMBOLS if s[0] == "dyf_ensemble_size_metrics"]
    assert len(rows) == 1 and len(rows[0][2]) == len(params)
    for i, p in enumerate(params):  # int32 n_segments, int32 n_members, int64 n_points, int64 member_stride where the header has them
        if p.startswith("int32_t"):
            assert rows[0][2][i] is C.c_int32, p
        if p.startswith("int64_t"):
            assert rows[0][2][i] is C.c_int64, p
    assert sum(p.startswith("int32_t") for p in params) == 2 and sum(p.startswith("int64_t") for p in params) == 2


def test_per_member_metrics_ask_for_gpu_tensors():
    from dyffusion_amd.metrics import evaluate_ensemble_prediction_for_varying_members, evaluate_per_member_mse

    preds, targets = torch.zeros(3, 2, 5), torch.zeros(2, 5)
    for mean_over_samples in (True, False):
        with pytest.raises(ValueError, match="GPU tensors"):  # the request itself is served: only the tensors are in the wrong place
            evaluate_per_member_mse(preds, targets, engine=None, mean_over_samples=mean_over_samples)
    with pytest.raises(AssertionError):
        evaluate_per_member_mse(preds, torch.zeros(3, 5), engine=None)
    with pytest.raises(ValueError, match="GPU tensors"):
        evaluate_ensemble_prediction_for_varying_members(preds, targets, engine=None)
    with pytest.raises(AssertionError):
        evaluate_ensemble_prediction_for_varying_members(preds, torch.zeros(3, 5), engine=None)


class _StubEngine:
    """ensemble_size_metrics returns a fixed tensor: value = 1000 plane + 100 segment + member index."""

    def __init__(self):
        self.calls = []

    def ensemble_size_metrics(self, preds, targets, accum=None):
        preds, targets = list(preds), list(targets)
        self.calls.append((len(preds), tuple(preds[0].shape)))
        n = preds[0].shape[0]
        k, s, m = np.meshgrid(np.arange(4), np.arange(len(preds)), np.arange(n), indexing="ij")
        return torch.from_numpy((1000.0 * k + 100.0 * s + m).astype(np.float64))


def test_size_curve_key_layout():
    from dyffusion_amd.metrics import SIZE_ROWS, eval_ensemble_size_curves, trajectory_size_curve_keys

    assert SIZE_ROWS == refs.ROWS
    n = 4
    results = {"t1_preds": torch.zeros(n, 2, 5), "t1_targets": torch.zeros(2, 5), "t2_preds": torch.zeros(n, 2, 5),
               "t2_targets": torch.zeros(2, 5), "t3_preds": torch.zeros(n, 2, 5), "condition": torch.zeros(2, 1)}  # t3: no targets
    eng = _StubEngine()
    out = eval_ensemble_size_curves(results, eng, "val")
    assert eng.calls == [(2, (n, 2, 5))]  # both horizons as the segments of one call
    plane = {"mse": 0.0, "ssr": 1000.0, "crps": 2000.0}
    want = {}
    for k in (1, 2, 3):  # n = N stays with eval_ensemble_predictions
        for m, base in plane.items():
            want[f"val/{k}ens_mems/t1/{m}"] = base + (k - 1)
            want[f"val/{k}ens_mems/t2/{m}"] = base + 100.0 + (k - 1)
            want[f"val/{k}ens_mems/avg/{m}"] = base + 50.0 + (k - 1)
    assert out == want and all(isinstance(v, float) for v in out.values())
    assert eval_ensemble_size_curves({"t1_preds": torch.zeros(1, 2, 5), "t1_targets": torch.zeros(2, 5)}, _StubEngine(), "val") == {}
    # the test epoch's form of the same keys, from a (4, T, N) mean
    by_size = eng.ensemble_size_metrics([torch.zeros(3, 5)] * 2, [torch.zeros(5)] * 2).numpy()
    keys = trajectory_size_curve_keys(by_size, "test_hard")
    assert set(keys) == {f"test/test_hard/{k}ens_mems/{t}/{m}" for k in (1, 2) for t in ("t1", "t2", "avg") for m in plane}
    assert keys["test/test_hard/2ens_mems/t2/crps"] == 2101.0 and keys["test/test_hard/1ens_mems/avg/ssr"] == 1050.0
    assert set(trajectory_size_curve_keys(by_size, "")) == {k.replace("test/test_hard/", "test/", 1) for k in keys}


def test_experiment_flag_is_off_by_default():
    import inspect

    import dyffusion_amd as D

    p = inspect.signature(D.MultiHorizonForecastingDYffusion.__init__).parameters["ensemble_size_curves"]
    assert p.default is False
