"""The per-prefix reference of the ensemble-size metrics (dyf_ensemble_size_metrics): oracle/metrics.py applied to the ensembles
made of the first n members, n = 1..N, as the reference's evaluate_ensemble_prediction_for_varying_members slices them
(evaluation.py:145-156), and the reference's expression for every member's own MSE (evaluation.py:51-55).  Pinned to the
reference's own numbers by tests/test_ensemble_size_refs.py; shared by the GPU tests."""
import numpy as np

from oracle import metrics as om

ROWS = ("mse", "ssr", "crps", "mse_per_mem")  # plane order of HipEngine.ensemble_size_metrics


def mse_per_member(preds: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """(N,): np.mean((p - y)^2) over every axis but the members'."""
    diff = preds - targets
    return np.mean(diff ** 2, axis=tuple(range(1, preds.ndim)))


def prefix_reference(preds: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """preds (N, B, ...), targets (B, ...) -> (4, N) float64: rows mse, ssr, crps of preds[:n] at column n - 1, and mse_per_mem."""
    n = preds.shape[0]
    out = np.zeros((4, n))
    for k in range(1, n + 1):
        ref = om.evaluate_ensemble_prediction(preds[:k], targets)
        out[:3, k - 1] = [ref[m] for m in ROWS[:3]]
    out[3] = mse_per_member(preds, targets)
    return out


def segment_reference(preds: np.ndarray, targets: np.ndarray) -> np.ndarray:
    """preds (N, T, ...), targets (T, ...) -> (4, T, N): prefix_reference of every segment preds[:, s], targets[s] (the points of
    a segment are pooled, so a leading axis of one sample is added where the segment has a single axis)."""
    t = preds.shape[1]
    out = np.zeros((4, t, preds.shape[0]))
    for s in range(t):
        out[:, s] = prefix_reference(preds[:, s][:, None], targets[s][None])
    return out
