"""Golden vectors of the grouped ensemble scores (dyf_ensemble_scores): ensemble stacks (N, B, C, H, W) with their targets
(B, C, H, W) and what the REFERENCE's own numpy functions (src/utilities/evaluation.py, imported through oracle/ref_import.py) give
for mean_dims = None ("all"), (0, 2, 3) ("channel": one value per channel) and (1, 2, 3) ("sample": one value per sample):

    mse_{all,channel,sample}   evaluate_ensemble_mse(preds, targets, mean_dims)
    ssr_{all,channel,sample}   evaluate_ensemble_spread_skill_ratio(preds, targets, mean_dims=mean_dims)
    nll_{all,channel,sample}   evaluate_ensemble_nll(preds.mean(0), np.var(preds, axis=0), targets, mean_dims)
                               (the mean and the variance that evaluation.py:42,76 compute for it; one member: var = 0, NaN)

    python tests/golden/make_golden_ensemble_scores.py      # writes ensscores_{a,b,c}.npz into tests/golden/ (or $DYF_GOLDEN_OUT)

Not generated: the reference's CRPS goes through xskillscore, which is absent (oracle/metrics.py), so CRPS stays definitional; and
the reference's evaluate_ensemble_corr calls np.corrcoef(x.reshape(1, -1), y.reshape(1, -1), rowvar=False), which raises under numpy
2.2.6 (ValueError: with rowvar=False the first (1, P) array is transposed before the second is stacked on it, and their
dimensions no longer match), so the correlation stays definitional too: np.corrcoef of the two flattened fields
(tests/ensemble_scores_refs.py).  Data only; tests/test_ensemble_scores_refs.py regenerates the files and compares bit for bit.
"""
import os
import sys

import numpy as np

_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(_DIR, "..", "..")))
OUT = os.environ.get("DYF_GOLDEN_OUT") or _DIR

from oracle import ref_import  # noqa: E402

SHAPES = {"a": (6, 2, 2, 7, 6), "b": (20, 1, 3, 13, 9), "c": (1, 3, 2, 5, 4)}  # (N, B, C, H, W)
MEAN_DIMS = {"all": None, "channel": (0, 2, 3), "sample": (1, 2, 3)}


def main():
    ref_import.activate()
    from src.utilities import evaluation as ev

    rng = np.random.default_rng(31)
    for name, shape in SHAPES.items():
        n, c = shape[0], shape[2]
        truth = rng.normal(size=shape[1:]).astype(np.float32)
        # every channel has its own spread and offset: the per-channel scores differ
        scale = (0.5 + 0.2 * np.arange(c)).reshape(1, 1, c, 1, 1)
        offset = (0.1 - 0.15 * np.arange(c)).reshape(1, 1, c, 1, 1)
        preds = (truth[None] * 0.8 + offset + scale * rng.normal(size=shape)).astype(np.float32)
        arrays = {"preds": preds, "targets": truth}
        with np.errstate(divide="ignore", invalid="ignore"):
            mean, var = preds.mean(axis=0), np.var(preds, axis=0)
            for tag, dims in MEAN_DIMS.items():
                arrays[f"mse_{tag}"] = np.asarray(ev.evaluate_ensemble_mse(preds, truth, mean_dims=dims), dtype=np.float64)
                arrays[f"ssr_{tag}"] = np.asarray(ev.evaluate_ensemble_spread_skill_ratio(preds, truth, mean_dims=dims), dtype=np.float64)
                arrays[f"nll_{tag}"] = np.asarray(ev.evaluate_ensemble_nll(mean, var, truth, mean_dims=dims), dtype=np.float64)
        for tag, want in (("all", ()), ("channel", (c,)), ("sample", (shape[1],))):
            assert arrays[f"mse_{tag}"].shape == arrays[f"ssr_{tag}"].shape == arrays[f"nll_{tag}"].shape == want
        np.savez(os.path.join(OUT, f"ensscores_{name}.npz"), **arrays)
        print(f"ensscores_{name}: mse {np.round(arrays['mse_channel'], 6).tolist()} ssr {np.round(arrays['ssr_channel'], 6).tolist()} "
              f"nll {np.round(arrays['nll_channel'], 6).tolist()} nll_all {float(arrays['nll_all']):.6f}")


if __name__ == "__main__":
    main()
