"""The float64 reference of the grouped ensemble scores (dyf_ensemble_scores): per group, oracle/metrics.py on the group's pooled
points for mse / ssr / crps, the reference's NLL expression (evaluation.py:129) and np.corrcoef of the ensemble mean with the
targets (evaluation.py:139-142).  Pinned to the reference's own numbers by tests/test_ensemble_scores_refs.py; shared by the GPU
tests."""
import warnings

import numpy as np

from oracle import metrics as om

ROWS = ("mse", "ssr", "crps", "nll", "corr")  # plane order of HipEngine.ensemble_scores


def nll_points(preds: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """Per point: 0.5 log(2 pi var) + (y - mean)^2 / (2 var) with the ensemble mean and population variance over axis 0, float64."""
    x, y = preds.astype(np.float64), targets.astype(np.float64)
    mean, var = x.mean(axis=0), x.var(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return 0.5 * np.log(2 * np.pi * var) + (y - mean) ** 2 / (2 * var)


def corr(preds: np.ndarray, targets: np.ndarray) -> float:
    """np.corrcoef of the ensemble mean with the targets over all points, float64 (NaN where either is constant)."""
    a, b = preds.astype(np.float64).mean(axis=0), targets.astype(np.float64)
    with warnings.catch_warnings(), np.errstate(divide="ignore", invalid="ignore"):
        warnings.simplefilter("ignore")
        return float(np.corrcoef(a.ravel(), b.ravel())[0, 1])


def pooled_reference(preds: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """preds (N, *pts), targets (*pts), any point shape -> (5,) float64 over all points.  oracle/metrics.py wants a sample axis:
    the points are handed over as (N, P, 1) / (P, 1)."""
    n = preds.shape[0]
    x, y = preds.reshape(n, -1, 1).astype(np.float64), targets.reshape(-1, 1).astype(np.float64)
    ref = om.evaluate_ensemble_prediction(x, y)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        nll = float(np.mean(nll_points(x, y)))
    return np.array([ref["mse"], ref["ssr"], ref["crps"], nll, corr(x, y)])


def group_reference(preds: np.ndarray, targets: np.ndarray, group_shape) -> np.ndarray:
    """preds (N, *pts), targets (*pts), group_shape = (outer, groups, inner) with product = the points -> (5, groups): the pooled
    reference of every group's points preds[:, :, g, :] of the row-major (outer, groups, inner) view."""
    outer, groups, inner = group_shape
    n = preds.shape[0]
    x, y = preds.reshape(n, outer, groups, inner), targets.reshape(outer, groups, inner)
    return np.stack([pooled_reference(x[:, :, g], y[:, g]) for g in range(groups)], axis=1)


def segment_reference(preds: np.ndarray, targets: np.ndarray, group_shape=None) -> np.ndarray:
    """preds (N, T, *pts), targets (T, *pts) -> (5, T, groups): group_reference of every segment (None: pooled, one group)."""
    t = preds.shape[1]
    if group_shape is None:
        group_shape = (1, 1, int(np.prod(targets.shape[1:], dtype=np.int64)))
    return np.stack([group_reference(preds[:, s], targets[s], group_shape) for s in range(t)], axis=1)


def nll_scale(preds: np.ndarray, targets: np.ndarray, group_shape=None) -> np.ndarray:
    """(T, groups): mean over a group's points of |nll_p| -- the scale of the NLL tolerance."""
    n, t = preds.shape[:2]
    if group_shape is None:
        group_shape = (1, 1, int(np.prod(targets.shape[1:], dtype=np.int64)))
    outer, groups, inner = group_shape
    a = np.abs(nll_points(preds.reshape(n, t, outer, groups, inner), targets.reshape(t, outer, groups, inner)))
    return a.mean(axis=(1, 3))
