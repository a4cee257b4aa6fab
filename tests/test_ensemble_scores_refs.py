"""The references of the grouped ensemble scores (dyf_ensemble_scores), on the CPU:

  * tests/golden/ensscores_{a,b,c}.npz hold what the reference's own functions give for mean_dims = None, per channel and per
    sample (tests/golden/make_golden_ensemble_scores.py); the float64 reference of the GPU tests (tests/ensemble_scores_refs.py)
    is pinned to them at the tolerance of tests/test_ensemble_size_refs.py;
  * where the reference checkout is present the fixtures regenerate bit for bit;
  * header, ctypes table and ABI version; the host surface that needs no GPU: the mean_dims map and its refusals, names, the key
    layout, the defaults of the new flags, the refusal of CPU tensors.
"""
import ctypes as C
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import ensemble_scores_refs as refs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
GOLDEN = os.path.join(ROOT, "tests", "golden")
FILES = {"ensscores_a.npz": (6, 2, 2, 7, 6), "ensscores_b.npz": (20, 1, 3, 13, 9), "ensscores_c.npz": (1, 3, 2, 5, 4)}
TAGS = ("all", "channel", "sample")
KEYS = sorted(["preds", "targets"] + [f"{m}_{t}" for m in ("mse", "ssr", "nll") for t in TAGS])

needs_reference = pytest.mark.skipif(not os.path.isdir("/root/reference/src"),
                                     reason="the reference checkout is only present in the build container")


@pytest.mark.parametrize("name", sorted(FILES))
def test_group_reference_matches_the_reference_per_mean_dims(name):
    with np.load(os.path.join(GOLDEN, name), allow_pickle=False) as z:
        assert sorted(z.files) == KEYS
        gold = {k: z[k] for k in z.files}
    preds, targets = gold["preds"], gold["targets"]
    n, b, c, h, w = FILES[name]
    assert preds.shape == FILES[name] and targets.shape == FILES[name][1:] and preds.dtype == targets.dtype == np.float32
    assert os.path.getsize(os.path.join(GOLDEN, name)) < 1_000_000
    shapes = {"all": ((1, 1, b * c * h * w), ()), "channel": ((b, c, h * w), (c,)), "sample": ((1, b, c * h * w), (b,))}
    for tag, (group_shape, want_shape) in shapes.items():
        ref = refs.group_reference(preds, targets, group_shape)
        assert ref.shape == (5, group_shape[1]) and ref.dtype == np.float64
        for i, m in enumerate(("mse", "ssr")):
            g = gold[f"{m}_{tag}"]
            assert g.shape == want_shape and g.dtype == np.float64
            assert ref[i] == pytest.approx(g.reshape(-1), rel=1e-6, abs=0.0), (tag, m)
        g = gold[f"nll_{tag}"].reshape(-1)
        if n == 1:  # var = 0: the reference's NLL is NaN, and so is ours; zero spread exactly
            assert np.all(np.isnan(g)) and np.all(np.isnan(ref[3])) and np.all(ref[1] == 0.0) and np.all(gold[f"ssr_{tag}"] == 0.0)
        else:
            assert ref[3] == pytest.approx(g, rel=1e-6, abs=0.0), tag
            assert np.all(np.abs(ref[4]) <= 1.0) and np.all(ref[4] > 0.3)  # the members follow the truth
    # the groups differ: a kernel that pooled everything, or mixed the groups up, would not pass
    if n > 1:
        assert len(set(np.round(gold["mse_channel"], 6).tolist())) == c and len(set(np.round(gold["nll_channel"], 6).tolist())) == c


def test_the_reference_is_what_it_says_on_small_cases():
    rng = np.random.default_rng(5)
    truth = rng.normal(size=(2, 3, 4)).astype(np.float32)
    preds = (truth[None] * 0.7 + 0.5 * rng.normal(size=(5, 2, 3, 4))).astype(np.float32)
    per_channel = refs.group_reference(preds, truth, (2, 3, 4))
    x, y = preds.astype(np.float64), truth.astype(np.float64)
    for g in range(3):
        mean, var = x[:, :, g].mean(axis=0), x[:, :, g].var(axis=0)
        assert per_channel[0, g] == pytest.approx(np.mean((mean - y[:, g]) ** 2), rel=1e-12)
        assert per_channel[1, g] == pytest.approx(np.sqrt(var.mean()) / np.sqrt(per_channel[0, g]), rel=1e-12)
        assert per_channel[3, g] == pytest.approx(np.mean(0.5 * np.log(2 * np.pi * var) + (y[:, g] - mean) ** 2 / (2 * var)), rel=1e-12)
        assert per_channel[4, g] == pytest.approx(np.corrcoef(mean.ravel(), y[:, g].ravel())[0, 1], rel=1e-12)
    seg = refs.segment_reference(preds, truth, (1, 3, 4))  # the two samples as two segments, per row of the (3, 4) field
    assert seg.shape == (5, 2, 3)
    assert np.array_equal(seg[:, 1], refs.group_reference(preds[:, 1], truth[1], (1, 3, 4)))
    assert np.array_equal(refs.segment_reference(preds, truth)[:, 0, 0], refs.pooled_reference(preds[:, 0], truth[0]))
    assert refs.nll_scale(preds, truth, (1, 3, 4)).shape == (2, 3)
    # constant targets, or constant ensemble means: NaN, as np.corrcoef
    assert np.isnan(refs.corr(preds, np.full_like(truth, 0.25))) and np.isnan(refs.corr(np.full_like(preds, 0.3), truth))


@needs_reference
def test_ensemble_scores_fixtures_regenerate_bit_identically(tmp_path):
    env = dict(os.environ, DYF_GOLDEN_OUT=str(tmp_path), PYTHONHASHSEED="4242")
    r = subprocess.run([sys.executable, os.path.join(GOLDEN, "make_golden_ensemble_scores.py")], env=env, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    assert sorted(os.listdir(tmp_path)) == sorted(FILES)
    for name in FILES:
        with np.load(os.path.join(tmp_path, name), allow_pickle=False) as x, np.load(os.path.join(GOLDEN, name), allow_pickle=False) as y:
            assert sorted(x.files) == sorted(y.files) == KEYS, name
            for k in x.files:
                assert x[k].dtype == y[k].dtype and x[k].shape == y[k].shape, (name, k)
                assert np.array_equal(x[k], y[k], equal_nan=True), (name, k)


def test_header_binding_and_abi_version_agree():
    from dyffusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "dyffusion_hip.h")).read()
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", hdr, re.M) and _lib.DYF_ABI_VERSION == 9
    m = re.search(r"dyf_status\s+dyf_ensemble_scores\s*\(([^;]*)\)\s*;", hdr)
    assert m, "dyf_ensemble_scores is not declared in include/dyffusion_hip.h"
    params = [p.strip() for p in m.group(1).split(",")]
    assert len(params) == 13 and params[0].startswith("dyf_engine*") and params[-1].startswith("void* stream")
    names = [p.split()[-1].lstrip("*") for p in params]
    assert names == ["engine", "n_segments", "preds_dev", "targets_dev", "n_members", "n_points", "member_stride", "n_outer", "n_groups",
                     "n_inner", "out_dev", "accum_dev", "stream"]
    rows = [s for s in _lib.SYMBOLS if s[0] == "dyf_ensemble_scores"]
    assert len(rows) == 1 and len(rows[0][2]) == len(params) and rows[0][1] is C.c_int
    for i, p in enumerate(params):
        if p.startswith("int32_t"):
            assert rows[0][2][i] is C.c_int32, p
        if p.startswith("int64_t"):
            assert rows[0][2][i] is C.c_int64, p
    assert [n for n, p in zip(names, params) if p.startswith("int32_t")] == ["n_segments", "n_members", "n_groups"]
    assert [n for n, p in zip(names, params) if p.startswith("int64_t")] == ["n_points", "member_stride", "n_outer", "n_inner"]
    assert "2^24 - 1" in hdr[m.start() - 3000:m.start()]  # the header states the grid limit


def test_mean_dims_map_to_outer_groups_inner():
    from dyffusion_amd.metrics import mean_dims_to_group_shape as f

    shape = (4, 3, 5, 7)
    assert f(shape, None) is None and f(shape, (0, 1, 2, 3)) is None and f(shape, (-1, 0, 2, 1)) is None and f((6,), 0) is None
    assert f(shape, (0, 2, 3)) == (1, 1, (4, 3, 35))           # per channel
    assert f(shape, (1, 2, 3)) == (0, 0, (1, 4, 105))          # per sample
    assert f(shape, (2, 3)) == (0, 1, (1, 12, 35))             # per sample and channel
    assert f(shape, (0, 1, 2)) == (3, 3, (60, 7, 1))           # the last axis: inner 1
    assert f(shape, (-4, -3, -2)) == (3, 3, (60, 7, 1))
    assert f(shape, 0) == (1, 3, (4, 105, 1)) and f(shape, ()) == (0, 3, (1, 420, 1))
    assert f(shape, (0, 3)) == (1, 2, (4, 15, 7)) and f(shape, [3]) == (0, 2, (1, 60, 7))
    for dims in ((1,), (2,), (1, 2), (0, 2), (1, 3)):  # the kept axes have a gap
        with pytest.raises(NotImplementedError, match="one contiguous run"):
            f(shape, dims)
    for dims in ((4,), (0, -5), (0, 0), (1, -3), (0.0,)):
        with pytest.raises(ValueError):
            f(shape, dims)


def test_cpu_tensors_and_mismatched_shapes_are_refused():
    from dyffusion_amd import metrics as M

    preds, targets = torch.zeros(3, 2, 4, 5), torch.zeros(2, 4, 5)
    calls = [lambda p, t: M.evaluate_ensemble_mse(p, t, None), lambda p, t: M.evaluate_ensemble_mse(p, t, None, mean_dims=(0, 2)),
             lambda p, t: M.evaluate_ensemble_spread_skill_ratio(p, t, None), lambda p, t: M.evaluate_ensemble_nll(p, t, None, mean_dims=(1, 2)),
             lambda p, t: M.evaluate_ensemble_crps(p, t, None), lambda p, t: M.evaluate_ensemble_crps(p, t, None, mean_over_samples=False),
             lambda p, t: M.evaluate_ensemble_corr(p, t, None), lambda p, t: M.evaluate_ensemble_scores(p, t, None),
             lambda p, t: M.evaluate_ensemble_scores([p, p], [t, t], None, mean_dims=(1, 2))]
    for call in calls:
        with pytest.raises(ValueError, match="GPU tensors"):
            call(preds, targets)
        with pytest.raises(AssertionError, match=r"predictions.shape\[1\]"):
            call(preds, torch.zeros(3, 4, 5))
    assert "ensemble" in M.evaluate_ensemble_nll.__doc__.lower() and "variance" in M.evaluate_ensemble_nll.__doc__


class _StubEngine:
    """ensemble_scores returns a fixed tensor: value = 1000 plane + 100 segment + group; ensemble_metrics three fixed floats."""

    def __init__(self):
        self.calls = []

    def ensemble_metrics(self, preds, targets):
        return (0.5, 0.25, 0.125)

    def ensemble_scores(self, preds, targets, group_shape=None, accum=None):
        preds, targets = list(preds), list(targets)
        self.calls.append((len(preds), tuple(preds[0].shape), group_shape))
        g = 1 if group_shape is None else group_shape[1]
        k, s, j = np.meshgrid(np.arange(5), np.arange(len(preds)), np.arange(g), indexing="ij")
        return torch.from_numpy((1000.0 * k + 100.0 * s + j).astype(np.float64))


class _CudaLike(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the stub engine never reads it."""

    @property
    def is_cuda(self):
        return True


def test_extended_and_per_channel_key_layout():
    from dyffusion_amd.metrics import SCORE_ROWS, eval_ensemble_predictions

    assert SCORE_ROWS == refs.ROWS == ("mse", "ssr", "crps", "nll", "corr")
    n = 4
    z = lambda *s: torch.zeros(*s).as_subclass(_CudaLike)  # noqa: E731
    results = {"t1_preds": z(n, 2, 3, 5, 6), "t1_targets": z(2, 3, 5, 6), "t2_preds": z(n, 2, 3, 5, 6), "t2_targets": z(2, 3, 5, 6),
               "t3_preds": z(n, 2, 3, 5, 6), "condition": z(2, 1)}  # t3: no targets
    base = {f"val/4ens_mems/{t}/{m}": v for t in ("t1", "t2", "avg") for m, v in (("mse", 0.5), ("ssr", 0.25), ("crps", 0.125))}
    eng = _StubEngine()
    assert eval_ensemble_predictions(results, eng, "val", infix="4ens_mems/") == base and eng.calls == []  # both flags off: as before
    ext = eval_ensemble_predictions(results, eng, "val", infix="4ens_mems/", extended=True)
    assert eng.calls == [(2, (n, 2, 3, 5, 6), None)]  # both horizons as the segments of one pooled call
    want = dict(base)
    for m, plane in (("nll", 3000.0), ("corr", 4000.0)):
        want.update({f"val/4ens_mems/t1/{m}": plane, f"val/4ens_mems/t2/{m}": plane + 100.0, f"val/4ens_mems/avg/{m}": plane + 50.0})
    assert ext == want and all(isinstance(v, float) for v in ext.values())
    eng.calls.clear()
    per_c = eval_ensemble_predictions(results, eng, "val", infix="4ens_mems/", per_channel=True)
    assert eng.calls == [(2, (n, 2, 3, 5, 6), (2, 3, 30))]  # ... and of one per-channel call: (B, C, H * W)
    want = dict(base)
    for j in range(3):
        for i, m in enumerate(SCORE_ROWS):
            want.update({f"val/4ens_mems/t1/c{j}/{m}": 1000.0 * i + j, f"val/4ens_mems/t2/c{j}/{m}": 1000.0 * i + 100.0 + j,
                         f"val/4ens_mems/avg/c{j}/{m}": 1000.0 * i + 50.0 + j})
    assert per_c == want
    eng.calls.clear()
    both = eval_ensemble_predictions(results, eng, "test", extended=True, per_channel=True)
    assert len(eng.calls) == 2 and len(both) == 9 + 6 + 45 and "test/t2/c2/corr" in both and "test/avg/nll" in both
    # horizons of another shape make a call of their own; targets without a channel axis are one channel
    results["t4_preds"], results["t4_targets"] = z(n, 2, 12), z(2, 12)
    eng.calls.clear()
    more = eval_ensemble_predictions(results, eng, "val", per_channel=True)
    assert eng.calls == [(2, (n, 2, 3, 5, 6), (2, 3, 30)), (1, (n, 2, 12), (1, 1, 24))]
    assert more["val/t4/c0/nll"] == 3000.0 and "val/t4/c1/nll" not in more
    assert more["val/avg/c0/nll"] == pytest.approx((3000.0 + 3100.0 + 3000.0) / 3) and more["val/avg/c1/nll"] == 3051.0


def test_new_flags_are_off_by_default():
    import dyffusion_amd as D
    from dyffusion_amd import metrics as M
    from dyffusion_amd.engine import HipEngine

    assert inspect.signature(D.MultiHorizonForecastingDYffusion.__init__).parameters["extended_metrics"].default is False
    p = inspect.signature(M.eval_ensemble_predictions).parameters
    assert p["extended"].default is False and p["per_channel"].default is False
    p = inspect.signature(HipEngine.ensemble_scores).parameters
    assert list(p) == ["self", "preds", "targets", "group_shape", "accum"] and p["group_shape"].default is None and p["accum"].default is None
    for name, args in (("evaluate_ensemble_mse", ["predictions", "targets", "engine", "mean_dims"]),
                       ("evaluate_ensemble_spread_skill_ratio", ["predictions", "targets", "engine", "skill_metric", "mean_dims"]),
                       ("evaluate_ensemble_nll", ["predictions", "targets", "engine", "mean_dims"]),
                       ("evaluate_ensemble_crps", ["predictions", "targets", "engine", "mean_over_samples"]),
                       ("evaluate_ensemble_corr", ["predictions", "targets", "engine"]),
                       ("evaluate_ensemble_scores", ["predictions", "targets", "engine", "mean_dims"])):
        assert list(inspect.signature(getattr(M, name)).parameters) == args, name
