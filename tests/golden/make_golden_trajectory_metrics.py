"""Golden vectors of the per-segment ensemble metrics (dyf_trajectory_metrics): trajectories (N, T, B, C, H, W) with their targets
(T, B, C, H, W) and what the REFERENCE's own numpy functions (src/utilities/evaluation.py, imported through oracle/ref_import.py)
give per horizon step, the way its test_step calls them (evaluate_ensemble_prediction(..., mean_over_samples=False):
mean_dims = every axis but the first):

    mse   evaluate_ensemble_mse(preds, targets, mean_dims=(1, 2, 3, 4))
    ssr   evaluate_ensemble_spread_skill_ratio(preds, targets, skill_metric=sqrt(mse), mean_dims=(1, 2, 3, 4))

    python tests/golden/make_golden_trajectory_metrics.py      # writes trajmetrics_{a,b,c}.npz into tests/golden/ (or $DYF_GOLDEN_OUT)

The reference's CRPS goes through xskillscore, which is absent (oracle/metrics.py): it cannot be generated.  Data only;
tests/test_trajectory_metrics_refs.py regenerates the files and compares bit for bit.
"""
import os
import sys

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(_DIR, "..", "..")))
OUT = os.environ.get("DYF_GOLDEN_OUT") or _DIR

from oracle import ref_import  # noqa: E402

SHAPES = {"a": (5, 4, 2, 2, 7, 6), "b": (20, 3, 1, 3, 13, 9), "c": (1, 2, 2, 1, 5, 5)}  # (N, T, B, C, H, W)


def main():
    ref_import.activate()
    from src.utilities.evaluation import evaluate_ensemble_mse, evaluate_ensemble_spread_skill_ratio

    rng = np.random.default_rng(23)
    for name, shape in SHAPES.items():
        n, t = shape[:2]
        truth = rng.normal(size=shape[1:]).astype(np.float32)
        # the spread grows along the trajectory, as a forecast's does: every horizon step has its own mse and ssr
        scale = (0.4 + 0.15 * np.arange(1, t + 1)).reshape(1, t, 1, 1, 1, 1)
        preds = (truth[None] * 0.8 + 0.1 + scale * rng.normal(size=shape)).astype(np.float32)
        mean_dims = tuple(range(1, truth.ndim))
        mse = np.asarray(evaluate_ensemble_mse(preds, truth, mean_dims=mean_dims))
        ssr = np.asarray(evaluate_ensemble_spread_skill_ratio(preds, truth, skill_metric=np.sqrt(mse), mean_dims=mean_dims))
        assert mse.shape == ssr.shape == (t,)
        np.savez(os.path.join(OUT, f"trajmetrics_{name}.npz"), preds=preds, targets=truth, mse=mse, ssr=ssr)
        print(f"trajmetrics_{name}: mse {np.round(mse, 6).tolist()} ssr {np.round(ssr, 6).tolist()}")


if __name__ == "__main__":
    main()
