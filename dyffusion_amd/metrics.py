"""On-device ensemble metrics: the surface of `src/utilities/evaluation.py` and of
`BaseExperiment._eval_ensemble_predictions` (`_base_experiment.py:617-640`) on GPU tensors, so the forecast stack never
makes the reference's `.cpu().numpy()` round trip.  The reductions run in `ensemble_metrics_kernel` (kernels.hip) through
`dyf_ensemble_metrics`, and per segment (`mean_over_samples=False`, the test epoch of the physical-systems benchmark) in
`trajectory_metrics_kernel` through `dyf_trajectory_metrics`; as a function of the ensemble size (the first n members, n = 1..N, and
every member's own MSE) in `ensemble_size_metrics_kernel` through `dyf_ensemble_size_metrics`.  There is no CPU fallback."""
from collections import defaultdict
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .engine import HipEngine

METRIC_ROWS = ("mse", "ssr", "crps")  # row order of the (3, T) tensors of HipEngine.trajectory_metrics
SIZE_ROWS = METRIC_ROWS + ("mse_per_mem",)  # plane order of the (4, T, N) tensors of HipEngine.ensemble_size_metrics


def evaluate_ensemble_prediction(predictions: Tensor, targets: Tensor, engine: HipEngine, mean_over_samples: bool = True,
                                 also_per_member_metrics: bool = False) -> Dict[str, object]:
    """evaluation.py:10-80 with ensemble_dim=0: predictions (n_members, n_samples, *), targets (n_samples, *), both on the
    engine's GPU -> {"ssr", "crps", "mse"}: host floats over all samples, or with `mean_over_samples=False` float64 device
    tensors of length n_samples (one value per sample, nothing synchronised).  `also_per_member_metrics=True` is refused here;
    `evaluate_per_member_mse` gives what it would add."""
    if also_per_member_metrics:
        raise NotImplementedError("also_per_member_metrics=True (the reference never passes it): see evaluate_per_member_mse")
    if predictions.shape[1] != targets.shape[0]:
        raise AssertionError(f"predictions.shape[1] ({predictions.shape[1]}) != targets.shape[0] ({targets.shape[0]})")
    if not predictions.is_cuda or not targets.is_cuda:
        raise ValueError("dyffusion_amd.metrics works on GPU tensors (the HIP engine computes them)")
    if not mean_over_samples:
        curves = engine.trajectory_metrics(predictions, targets)
        return {"ssr": curves[1], "crps": curves[2], "mse": curves[0]}
    mse, ssr, crps = engine.ensemble_metrics(predictions, targets)
    return {"ssr": ssr, "crps": crps, "mse": mse}


def evaluate_per_member_mse(predictions: Tensor, targets: Tensor, engine: HipEngine, mean_over_samples: bool = True) -> Dict[str, object]:
    """What `also_per_member_metrics=True` adds in the reference (evaluation.py:49-55): {"mse_per_mem": (n_members,), every member's
    own MSE over all axes, "mse_per_mem_mean"}: a float64 array and a float, or with `mean_over_samples=False` float64 device tensors
    and nothing synchronised (the mean over the equal-sized samples is the all-axes mean)."""
    if predictions.shape[1] != targets.shape[0]:
        raise AssertionError(f"predictions.shape[1] ({predictions.shape[1]}) != targets.shape[0] ({targets.shape[0]})")
    if not predictions.is_cuda or not targets.is_cuda:
        raise ValueError("dyffusion_amd.metrics works on GPU tensors (the HIP engine computes them)")
    if not mean_over_samples:
        per_mem = engine.ensemble_size_metrics(predictions, targets)[3].mean(dim=0)
        return {"mse_per_mem": per_mem, "mse_per_mem_mean": per_mem.mean()}
    per_mem = engine.ensemble_size_metrics([predictions], [targets])[3, 0].cpu().numpy()
    return {"mse_per_mem": per_mem, "mse_per_mem_mean": float(per_mem.mean())}


def evaluate_ensemble_prediction_for_varying_members(predictions: Tensor, targets: Tensor, engine: HipEngine) -> Dict[str, list]:
    """evaluation.py:145-156: {"ssr", "crps", "mse"} -> lists of N host floats, entry n - 1 the score of `predictions[:n]` over
    all samples.  One pass of `ensemble_size_metrics_kernel` over the stack, not N evaluations of its prefixes."""
    if predictions.shape[1] != targets.shape[0]:
        raise AssertionError(f"predictions.shape[1] ({predictions.shape[1]}) != targets.shape[0] ({targets.shape[0]})")
    if not predictions.is_cuda or not targets.is_cuda:
        raise ValueError("dyffusion_amd.metrics works on GPU tensors (the HIP engine computes them)")
    by_size = engine.ensemble_size_metrics([predictions], [targets])[:, 0].cpu().numpy()  # (4, N)
    return {m: [float(v) for v in by_size[SIZE_ROWS.index(m)]] for m in ("ssr", "crps", "mse")}


def eval_ensemble_size_curves(results: Dict[str, Tensor], engine: HipEngine, split: str = "val") -> Dict[str, float]:
    """The keys of `eval_ensemble_predictions` for the ensembles of the first n members, n = 1..N-1:
    `{split}/{n}ens_mems/t{k}/{m}` and `{split}/{n}ens_mems/avg/{m}` (what the reference logs when it is run with
    num_predictions = n on the same members).  Every `t{k}_preds` / `t{k}_targets` pair of equal shape is one segment of a single
    `ensemble_size_metrics` call; n = N stays with `eval_ensemble_predictions`."""
    groups: Dict[tuple, list] = {}
    for key in [k for k in results if k.endswith("preds")]:
        prefix = key.split("_")[0] if key != "preds" else ""
        tkey = f"{prefix}_targets" if prefix else "targets"
        if tkey in results:
            groups.setdefault((tuple(results[key].shape), tuple(results[tkey].shape)), []).append((prefix, key, tkey))
    out: Dict[str, float] = {}
    acc = defaultdict(list)
    for members in groups.values():
        by_size = engine.ensemble_size_metrics([results[k] for _, k, _ in members], [results[t] for _, _, t in members])
        by_size = by_size.cpu().numpy()  # (4, segments, N)
        for s, (prefix, _, _) in enumerate(members):
            for n in range(1, by_size.shape[2]):
                for m in ("ssr", "crps", "mse"):
                    v = float(by_size[SIZE_ROWS.index(m), s, n - 1])
                    out[f"{split}/{n}ens_mems/{prefix}/{m}"] = v
                    acc[f"{split}/{n}ens_mems/avg/{m}"].append(v)
    for k, v in acc.items():
        out[k] = float(sum(v) / len(v))
    return out


def eval_ensemble_predictions(results: Dict[str, Tensor], engine: HipEngine, split: str = "val",
                              infix: Optional[str] = None) -> Dict[str, float]:
    """_base_experiment.py:617-640: per-horizon metrics `{split}/{infix}t{k}/{m}` for every `t{k}_preds`/`t{k}_targets`
    pair of an evaluation step's output, plus their average over horizons `{split}/{infix}avg/{m}`."""
    infix = "" if infix is None else infix
    out: Dict[str, float] = {}
    acc = defaultdict(list)
    for key in [k for k in results if k.endswith("preds")]:
        prefix = key.split("_")[0] if key != "preds" else ""
        tkey = f"{prefix}_targets" if prefix else "targets"
        if tkey not in results:
            continue
        for m, v in evaluate_ensemble_prediction(results[key], results[tkey], engine).items():
            out[f"{split}/{infix}{prefix}/{m}"] = v
            acc[f"{split}/{infix}avg/{m}"].append(v)
    for k, v in acc.items():
        out[k] = float(sum(v) / len(v))
    return out


class TrajectoryMetricsAccumulator:
    """The test epoch of a PhysicalSystemsBenchmarkDataModule (forecasting_multi_horizon.py:231-279): every test instance gives
    the curves mse / ssr / crps over its T horizon steps, the epoch reports their mean over instances.  The sum of the curves
    stays on the device ((3, T) float64, added to by the kernel itself); `compute()` makes the only device-to-host copy."""

    def __init__(self, engine: HipEngine, by_size: bool = False):
        self._engine = engine
        self._by_size = by_size  # also the (4, T, N) sum of the ensemble-size curves (HipEngine.ensemble_size_metrics)
        self.reset()

    def reset(self) -> None:
        self._sum: Optional[Tensor] = None
        self._size_sum: Optional[Tensor] = None
        self.count = 0

    def update(self, preds_list: Sequence[Tensor], targets_list: Sequence[Tensor]) -> Tensor:
        """One instance: T (N, B, C, H, W) forecasts and their T (B, C, H, W) targets -> its (3, T) curves (device, float64)."""
        preds_list, targets_list = list(preds_list), list(targets_list)
        if self._sum is not None and len(preds_list) != self._sum.shape[1]:
            raise ValueError(f"{len(preds_list)} horizon steps, but the accumulated curves have {self._sum.shape[1]}")
        if self._sum is None:
            if not preds_list:
                raise ValueError("no segments")
            self._sum = torch.zeros(3, len(preds_list), dtype=torch.float64, device=preds_list[0].device)
        curves = self._engine.trajectory_metrics(preds_list, targets_list, accum=self._sum)
        if self._by_size:
            n = preds_list[0].shape[0]
            if self._size_sum is None:
                self._size_sum = torch.zeros(4, len(preds_list), n, dtype=torch.float64, device=preds_list[0].device)
            elif n != self._size_sum.shape[2]:
                raise ValueError(f"{n} members, but the accumulated ensemble-size curves have {self._size_sum.shape[2]}")
            self._engine.ensemble_size_metrics(preds_list, targets_list, accum=self._size_sum)
        self.count += 1
        return curves

    def compute(self) -> Dict[str, np.ndarray]:
        """{metric: (T,) float64 array}: the mean over the instances seen since the last reset ({} before the first update); with
        `by_size` also "by_size": the (4, T, N) mean of the ensemble-size curves (planes SIZE_ROWS)."""
        if self._sum is None or self.count == 0:
            return {}
        mean = self._sum.cpu().numpy() / float(self.count)
        out = {m: mean[i] for i, m in enumerate(METRIC_ROWS)}
        if self._size_sum is not None:
            out["by_size"] = self._size_sum.cpu().numpy() / float(self.count)
        return out


def trajectory_size_curve_keys(by_size: np.ndarray, test_set_name: str = "") -> Dict[str, float]:
    """`trajectory_metric_keys` for the ensembles of the first n members, n = 1..N-1, of a (4, T, N) "by_size" mean:
    `test/{set/}{n}ens_mems/avg/{m}` and `.../t{i}/{m}`."""
    out: Dict[str, float] = {}
    for n in range(1, by_size.shape[2]):
        out.update(trajectory_metric_keys(f"{n}ens_mems/", {m: by_size[SIZE_ROWS.index(m), :, n - 1] for m in ("ssr", "crps", "mse")},
                                          test_set_name))
    return out


def trajectory_metric_keys(stem: str, curves: Dict[str, np.ndarray], test_set_name: str = "") -> Dict[str, float]:
    """What the reference's `on_test_epoch_end` leaves in the logger for a PhysicalSystemsBenchmarkDataModule
    (forecasting_multi_horizon.py:262-279): `test/{set/}{stem}avg/{m}`, the curve's mean over horizons, and per horizon step
    `test/{set/}{stem}t{i}/{m}`, i = 1..T (the summary keys of save_arrays_as_line_plot, wandb_callbacks.py:141-146).  `stem` is
    the ensemble infix (`"{N}ens_mems/"`), `test_set_name` the datamodule's (empty: no `{set/}` level)."""
    split_name = f"{test_set_name}/" if len(test_set_name) > 0 else ""
    key_stem = f"test/{split_name}{stem}"
    out: Dict[str, float] = {}
    for m, v in curves.items():
        v = np.asarray(v, dtype=np.float64)
        out[f"{key_stem}avg/{m}"] = float(v.mean())
    for m, v in curves.items():
        for i, y in enumerate(np.asarray(v, dtype=np.float64), start=1):
            out[f"{key_stem}/t{i}/{m}".replace("//", "/")] = float(y)
    return out
