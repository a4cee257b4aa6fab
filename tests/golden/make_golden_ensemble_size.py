"""Golden vectors of the ensemble-size metrics (dyf_ensemble_size_metrics): ensemble stacks (N, B, C, H, W) with their targets
(B, C, H, W) and what the REFERENCE's own numpy functions (src/utilities/evaluation.py, imported through oracle/ref_import.py) give
for the ensembles made of the first n members, n = 1..N, the way evaluate_ensemble_prediction_for_varying_members slices them:

    mse[n-1]          evaluate_ensemble_mse(preds[:n], targets)
    ssr[n-1]          evaluate_ensemble_spread_skill_ratio(preds[:n], targets, skill_metric=sqrt(mse[n-1]))
    mse_per_mem       evaluate_ensemble_prediction(preds, targets, also_per_member_metrics=True)["mse_per_mem"]
    mse_per_mem_mean  ... ["mse_per_mem_mean"]

    python tests/golden/make_golden_ensemble_size.py      # writes enssize_{a,b,c}.npz into tests/golden/ (or $DYF_GOLDEN_OUT)

The reference's CRPS goes through xskillscore, which is absent (oracle/metrics.py): it cannot be generated, and for the one call of
evaluate_ensemble_prediction the imported module's evaluate_ensemble_crps is replaced by a stand-in that returns NaN.  Data only;
tests/test_ensemble_size_refs.py regenerates the files and compares bit for bit.
"""
import os
import sys

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(_DIR, "..", "..")))
OUT = os.environ.get("DYF_GOLDEN_OUT") or _DIR

from oracle import ref_import  # noqa: E402

SHAPES = {"a": (6, 2, 2, 7, 6), "b": (20, 1, 3, 13, 9), "c": (1, 2, 1, 5, 5)}  # (N, B, C, H, W)


def main():
    ref_import.activate()
    from src.utilities import evaluation as ev

    rng = np.random.default_rng(29)
    for name, shape in SHAPES.items():
        n = shape[0]
        truth = rng.normal(size=shape[1:]).astype(np.float32)
        # every member has its own spread and offset: the prefixes differ, and so do the members' own errors
        scale = (0.4 + 0.07 * np.arange(n)).reshape(n, 1, 1, 1, 1)
        offset = (0.1 - 0.02 * np.arange(n)).reshape(n, 1, 1, 1, 1)
        preds = (truth[None] * 0.8 + offset + scale * rng.normal(size=shape)).astype(np.float32)
        mse = np.array([ev.evaluate_ensemble_mse(preds[:k], truth) for k in range(1, n + 1)], dtype=np.float64)
        ssr = np.array([ev.evaluate_ensemble_spread_skill_ratio(preds[:k], truth, skill_metric=np.sqrt(mse[k - 1]))
                        for k in range(1, n + 1)], dtype=np.float64)
        crps = ev.evaluate_ensemble_crps
        ev.evaluate_ensemble_crps = lambda *a, **k: float("nan")  # xskillscore is absent: CRPS stays definitional
        try:
            full = ev.evaluate_ensemble_prediction(preds, truth, also_per_member_metrics=True)
        finally:
            ev.evaluate_ensemble_crps = crps
        per_mem = np.asarray(full["mse_per_mem"], dtype=np.float64)
        per_mem_mean = np.asarray(full["mse_per_mem_mean"], dtype=np.float64)
        assert mse.shape == ssr.shape == per_mem.shape == (n,) and per_mem_mean.shape == ()
        np.savez(os.path.join(OUT, f"enssize_{name}.npz"), preds=preds, targets=truth, mse=mse, ssr=ssr, mse_per_mem=per_mem,
                 mse_per_mem_mean=per_mem_mean)
        print(f"enssize_{name}: mse {np.round(mse, 6).tolist()} ssr {np.round(ssr, 6).tolist()}")


if __name__ == "__main__":
    main()
