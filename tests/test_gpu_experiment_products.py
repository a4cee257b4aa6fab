"""-m gpu: the forecast products and the rank histogram through MultiHorizonForecastingDYffusion (predict_products, keep_members,
rank_histogram) on the smallest pair the experiment tests use.  With the defaults every returned dict has exactly today's keys."""
import numpy as np
import pytest
import torch

from tests import ensemble_products_refs as refs
from tests.test_gpu_ensemble_size_metrics import _batches, _tiny_experiment

pytestmark = pytest.mark.gpu
N, T = 4, 3
SPEC = dict(mean=True, std=True, quantiles=(0.5,))
NAMES = ("mean", "std", "q0.5")


def _predict(exp):
    for batch in _batches(T):
        exp.predict_step(batch, 0)
    return exp.on_predict_epoch_end()


def test_defaults_keep_todays_keys():
    exp = _tiny_experiment(N, False)
    steps = [exp.evaluation_step(b, 0, split="predict", as_numpy=True) for b in _batches(T)]
    want = {f"t{k}_{w}" for k in range(1, T + 1) for w in ("preds", "targets")}
    assert all(set(s) == want for s in steps)
    out = _predict(_tiny_experiment(N, False))
    assert set(out) == want and out["t1_preds"].shape == (N, 5, 2, 19, 13) and out["t1_targets"].shape == (5, 2, 19, 13)
    exp = _tiny_experiment(N, False)
    for b in _batches(T):
        exp.validation_step(b, 0)
    val = exp.on_validation_epoch_end()
    assert set(val) == {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("mse", "ssr", "crps")}
    with pytest.raises(ValueError, match="keep_members"):
        _tiny_experiment(N, False, keep_members=False)


def test_predict_products_and_keep_members():
    out = _predict(_tiny_experiment(N, False, predict_products=SPEC))
    members = {f"t{k}_preds" for k in range(1, T + 1)}
    fields = {f"t{k}_preds_{name}" for k in range(1, T + 1) for name in NAMES}
    assert set(out) == members | fields | {f"t{k}_targets" for k in range(1, T + 1)}
    for k in range(1, T + 1):
        stack = out[f"t{k}_preds"]
        assert stack.shape == (N, 5, 2, 19, 13) and stack.dtype == np.float32
        got = {name: out[f"t{k}_preds_{name}"] for name in NAMES}
        assert all(isinstance(v, np.ndarray) and v.shape == (5, 2, 19, 13) and v.dtype == np.float32 for v in got.values())
        # the float64 reference of the members this very call returned, within the derived bounds
        used = refs.check_products({name: v.reshape(-1) for name, v in got.items()}, stack.reshape(N, -1), **SPEC)
        print(f"t{k}", {name: round(v, 3) for name, v in used.items()})
    # without the member stack: the same fields, bit for bit, under the same seed
    lean = _predict(_tiny_experiment(N, False, predict_products=SPEC, keep_members=False))
    assert set(lean) == fields | {f"t{k}_targets" for k in range(1, T + 1)}
    for key in fields:
        assert np.array_equal(lean[key].view(np.int32), out[key].view(np.int32)), key
    # the members of the defaults are the members of this run: the products changed nothing in the rollout
    plain = _predict(_tiny_experiment(N, False))
    assert all(np.array_equal(plain[key], out[key]) for key in members)


def test_rank_histogram_keys_of_the_validation_epoch():
    from dyffusion_amd.metrics import evaluate_rank_histogram

    exp = _tiny_experiment(N, False, rank_histogram=True)
    outs = [exp.validation_step(b, 0) for b in _batches(T)]
    got = exp.on_validation_epoch_end()
    base = {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("mse", "ssr", "crps")}
    assert set(got) == base | {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("rank_hist", "reliability_index")}
    indices = []
    for k in range(1, T + 1):
        preds = torch.cat([o[f"t{k}_preds"] for o in outs], dim=1)
        targets = torch.cat([o[f"t{k}_targets"] for o in outs], dim=0)
        hist, ri = got[f"val/{N}ens_mems/t{k}/rank_hist"], got[f"val/{N}ens_mems/t{k}/reliability_index"]
        assert isinstance(hist, np.ndarray) and hist.shape == (N + 1,) and hist.dtype == np.float64 and isinstance(ri, float)
        assert hist.sum() == pytest.approx(1.0, rel=1e-12)
        want = evaluate_rank_histogram(preds, targets, exp.model._engine)
        assert np.array_equal(hist, want["rank_hist"]) and ri == want["reliability_index"]
        ref = refs.frequencies(refs.histogram_reference(preds.reshape(N, -1).cpu().numpy(), targets.reshape(-1).cpu().numpy()))
        assert hist == pytest.approx(ref[0][0], rel=1e-12) and ri == pytest.approx(float(ref[1][0]), rel=1e-10)
        indices.append(ri)
    assert got[f"val/{N}ens_mems/avg/reliability_index"] == pytest.approx(sum(indices) / T, rel=1e-12)


def test_rank_histogram_keys_of_the_physical_systems_test_epoch():
    exp = _tiny_experiment(N, False, rank_histogram=True,
                           datamodule_config={"_target_": "src.datamodules.physical_systems_benchmark.PhysicalSystemsBenchmarkDataModule"})
    for b in _batches(T):
        exp.test_step(b, 0)
    got = exp.on_test_epoch_end()
    stem = f"test/{N}ens_mems/"
    extra = {f"{stem}{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("rank_hist", "reliability_index")}
    assert extra <= set(got) and len(got) == 12 + 8
    for t in ("t1", "t2", "t3", "avg"):
        assert got[f"{stem}{t}/rank_hist"].shape == (N + 1,) and got[f"{stem}{t}/rank_hist"].sum() == pytest.approx(1.0, rel=1e-12)
        assert isinstance(got[f"{stem}{t}/reliability_index"], float)
