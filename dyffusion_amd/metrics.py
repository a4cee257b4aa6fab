"""On-device ensemble metrics: the surface of `src/utilities/evaluation.py` and of
`BaseExperiment._eval_ensemble_predictions` (`_base_experiment.py:617-640`) on GPU tensors, so the forecast stack never
makes the reference's `.cpu().numpy()` round trip.  The reductions run in `ensemble_metrics_kernel` (kernels.hip) through
`dyf_ensemble_metrics`, and per segment (`mean_over_samples=False`, the test epoch of the physical-systems benchmark) in
`trajectory_metrics_kernel` through `dyf_trajectory_metrics`; as a function of the ensemble size (the first n members, n = 1..N, and
every member's own MSE) in `ensemble_size_metrics_kernel` through `dyf_ensemble_size_metrics`; per variable, per sample or over any
other contiguous run of kept axes (`mean_dims`), together with the Gaussian NLL and the correlation, in `ensemble_scores_kernel`
through `dyf_ensemble_scores`.  The forecast fields themselves (mean, spread, quantiles, exceedance probabilities per grid point) come
from `ensemble_products_kernel` through `dyf_ensemble_products`, the rank histogram from `rank_histogram_kernel` through
`dyf_rank_histogram`.  The multivariate side -- the energy score over whole fields or channels and the member-distance matrix -- comes
from `energy_score_kernel` through `dyf_energy_score`; the scores by spatial scale -- radially binned power spectra and the log-spectral
distances, spectral spread-skill ratio and coherence derived from them -- from `power_spectrum_kernel` through `dyf_power_spectrum`.
There is no CPU fallback."""
import math
from collections import defaultdict
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .engine import HipEngine

METRIC_ROWS = ("mse", "ssr", "crps")  # row order of the (3, T) tensors of HipEngine.trajectory_metrics
SIZE_ROWS = METRIC_ROWS + ("mse_per_mem",)  # plane order of the (4, T, N) tensors of HipEngine.ensemble_size_metrics
SCORE_ROWS = ("mse", "ssr", "crps", "nll", "corr")  # plane order of the (5, T, G) tensors of HipEngine.ensemble_scores
ENERGY_ROWS = ("es", "es_fair", "dist_target", "dist_pair")  # plane order of the (4, T, G) tensors of HipEngine.energy_score


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


def mean_dims_to_group_shape(shape: Sequence[int], mean_dims) -> Optional[Tuple[int, int, Tuple[int, int, int]]]:
    """`mean_dims` (axes of `targets`, as numpy takes them: None, an int or a sequence, negatives from the end) on a target of
    `shape` -> None when every axis is averaged, else (a, b, (outer, groups, inner)): the kept axes must be ONE contiguous run
    [a..b], which is the row-major view outer = prod(shape[:a]), groups = prod(shape[a:b+1]), inner = prod(shape[b+1:]) of
    `HipEngine.ensemble_scores`.  Kept axes with a gap are refused (NotImplementedError)."""
    nd = len(shape)
    if mean_dims is None:
        return None
    dims = (mean_dims,) if isinstance(mean_dims, int) else tuple(mean_dims)
    for d in dims:
        if not isinstance(d, int) or not -nd <= d < nd:
            raise ValueError(f"mean_dims {mean_dims!r}: axis {d!r} is out of bounds for targets of dimension {nd}")
    averaged = {d % nd for d in dims}
    if len(averaged) != len(dims):
        raise ValueError(f"mean_dims {mean_dims!r}: repeated axis")
    kept = [d for d in range(nd) if d not in averaged]
    if not kept:
        return None
    a, b = kept[0], kept[-1]
    if kept != list(range(a, b + 1)):
        raise NotImplementedError(f"mean_dims {mean_dims!r} keeps the axes {kept} of targets: the kept axes must be one contiguous run "
                                  "[a..b] (outer = prod(shape[:a]), groups = prod(shape[a:b+1]), inner = prod(shape[b+1:]))")
    return a, b, (math.prod(shape[:a]), math.prod(shape[a:b + 1]), math.prod(shape[b + 1:]))


def _scores(predictions, targets, engine: HipEngine, mean_dims) -> Dict[str, object]:
    """One `ensemble_scores` call -> {score: host float | float64 device tensor}, in SCORE_ROWS order.  `predictions` /
    `targets` are one (N, B, ...) / (B, ...) pair, or equally long lists of such pairs of one shape (several horizons): those go
    through as the segments of the one call and lead the result's shape."""
    many = not torch.is_tensor(predictions)
    plist, tlist = (list(predictions), list(targets)) if many else ([predictions], [targets])
    if many and (len(plist) != len(tlist) or not plist):
        raise ValueError(f"{len(plist)} prediction horizons but {len(tlist)} target horizons")
    for p, t in zip(plist, tlist):
        if p.shape[1] != t.shape[0]:
            raise AssertionError(f"predictions.shape[1] ({p.shape[1]}) != targets.shape[0] ({t.shape[0]})")
        if not p.is_cuda or not t.is_cuda:
            raise ValueError("dyffusion_amd.metrics works on GPU tensors (the HIP engine computes them)")
    shape = tuple(tlist[0].shape)
    grouped = mean_dims_to_group_shape(shape, mean_dims)
    if grouped is None:
        pooled = engine.ensemble_scores(plist, tlist)[:, :, 0].cpu().numpy()  # (5, T)
        return {m: (pooled[i] if many else float(pooled[i, 0])) for i, m in enumerate(SCORE_ROWS)}
    a, b, group_shape = grouped
    out = engine.ensemble_scores(plist, tlist, group_shape=group_shape)  # (5, T, G)
    out = out.reshape(5, len(plist), *shape[a:b + 1]) if many else out.reshape(5, *shape[a:b + 1])
    return {m: out[i] for i, m in enumerate(SCORE_ROWS)}


def evaluate_ensemble_scores(predictions, targets, engine: HipEngine, mean_dims=None) -> Dict[str, object]:
    """All five scores of evaluation.py's `mean_dims` surface in one pass of `ensemble_scores_kernel`: {"mse", "ssr", "crps", "nll",
    "corr"}.  predictions (n_members, n_samples, *), targets (n_samples, *), on the engine's GPU.  `mean_dims` are the axes of
    `targets` to average over, as in the reference: None or all axes gives host floats; otherwise the kept axes must be one
    contiguous run [a..b] (`mean_dims_to_group_shape`; (0, 2, 3) on (B, C, H, W) is per channel, (1, 2, 3) per sample) and every
    score is a float64 device tensor of shape targets.shape[a:b+1], nothing synchronised; other sets raise NotImplementedError.
    Lists of equally shaped horizons go through as the segments of one call and give a leading axis (host arrays when pooled).
    "corr" is the correlation over the points of a group, which the reference only has for all axes."""
    return _scores(predictions, targets, engine, mean_dims)


def evaluate_ensemble_mse(predictions, targets, engine: HipEngine, mean_dims=None):
    """evaluation.py:133-136: the MSE of the ensemble mean over `mean_dims` (see `evaluate_ensemble_scores`)."""
    return _scores(predictions, targets, engine, mean_dims)["mse"]


def evaluate_ensemble_spread_skill_ratio(predictions, targets, engine: HipEngine, skill_metric=None, mean_dims=None):
    """evaluation.py:99-120: sqrt(mean over `mean_dims` of the members' population variance) / skill, the skill being the RMSE of the
    ensemble mean over the same axes unless `skill_metric` (a number, or anything that broadcasts against the result) is given."""
    s = _scores(predictions, targets, engine, mean_dims)
    if skill_metric is None:
        return s["ssr"]
    if torch.is_tensor(s["ssr"]):
        return s["ssr"] * torch.sqrt(s["mse"]) / torch.as_tensor(skill_metric, dtype=torch.float64, device=s["ssr"].device)
    spread = s["ssr"] * np.sqrt(s["mse"])
    return spread / (skill_metric.cpu().numpy() if torch.is_tensor(skill_metric) else skill_metric)


def evaluate_ensemble_nll(predictions, targets, engine: HipEngine, mean_dims=None):
    """evaluation.py:123-130: the Gaussian negative log-likelihood 0.5 log(2 pi var) + (y - mean)^2 / (2 var), averaged over
    `mean_dims`.  It takes the ENSEMBLE (n_members, n_samples, *): the kernel computes the ensemble mean and the population variance
    (np.var over the members, evaluation.py:76) that the reference's function is handed.  One member has var = 0: NaN, as numpy."""
    return _scores(predictions, targets, engine, mean_dims)["nll"]


def evaluate_ensemble_crps(predictions, targets, engine: HipEngine, mean_over_samples: bool = True):
    """evaluation.py:83-96: the ensemble CRPS over all axes (a host float), or with `mean_over_samples=False` per sample: a float64
    device tensor (n_samples,), nothing synchronised."""
    nd = targets.dim() if torch.is_tensor(targets) else targets[0].dim()
    return _scores(predictions, targets, engine, None if mean_over_samples else tuple(range(1, nd)))["crps"]


def evaluate_ensemble_corr(predictions, targets, engine: HipEngine):
    """evaluation.py:139-142: the Pearson correlation of the ensemble mean with the targets over all points (a host float; NaN
    where either is constant, as np.corrcoef)."""
    return _scores(predictions, targets, engine, None)["corr"]


def ensemble_products(preds, engine: HipEngine, **spec) -> Dict[str, Tensor]:
    """The forecast fields of an ensemble, reduced over the members on the device: {name: tensor} with the names and keyword
    arguments of `HipEngine.ensemble_products` (`mean`, `std`, `min`, `max`, `quantiles`, `exceed`).  `preds` (N, ...) gives fields
    of shape (...); a list of T such tensors gives (T, ...) per name."""
    fields, names = engine.ensemble_products(preds, **spec)
    return {name: (fields[k] if torch.is_tensor(preds) else fields[:, k]) for k, name in enumerate(names)}


def rank_histogram_frequencies(bins):
    """Bins (..., N + 1) of `HipEngine.rank_histogram` (a float64 tensor or array) -> (frequencies, reliability index): the bins
    divided by their sum, and sum_i |f_i - 1 / (N + 1)|, 0 for a flat histogram (NaN where no point counted)."""
    freq = bins / bins.sum(-1, keepdims=True) if isinstance(bins, np.ndarray) else bins / bins.sum(dim=-1, keepdim=True)
    return freq, abs(freq - 1.0 / bins.shape[-1]).sum(-1)


def evaluate_rank_histogram(predictions, targets, engine: HipEngine, mean_dims=None) -> Dict[str, object]:
    """The rank histogram of the targets among the members: {"rank_hist": frequencies (..., N + 1), "reliability_index": sum_i |f_i -
    1 / (N + 1)|}.  predictions (n_members, n_samples, *), targets (n_samples, *), on the engine's GPU; `mean_dims` as in
    `evaluate_ensemble_scores`: None or all axes pools every point (a host array and a float), otherwise the kept axes lead the
    result (float64 device tensors, nothing synchronised).  Lists of equally shaped horizons go through as the segments of one
    call and give a leading axis."""
    many = not torch.is_tensor(predictions)
    plist, tlist = (list(predictions), list(targets)) if many else ([predictions], [targets])
    if many and (len(plist) != len(tlist) or not plist):
        raise ValueError(f"{len(plist)} prediction horizons but {len(tlist)} target horizons")
    for p, t in zip(plist, tlist):
        if p.shape[1] != t.shape[0]:
            raise AssertionError(f"predictions.shape[1] ({p.shape[1]}) != targets.shape[0] ({t.shape[0]})")
        if not p.is_cuda or not t.is_cuda:
            raise ValueError("dyffusion_amd.metrics works on GPU tensors (the HIP engine computes them)")
    shape = tuple(tlist[0].shape)
    grouped = mean_dims_to_group_shape(shape, mean_dims)
    if grouped is None:
        bins = engine.rank_histogram(plist, tlist)[:, 0].cpu().numpy()  # (T, N + 1)
        freq, ri = rank_histogram_frequencies(bins)
        return {"rank_hist": freq if many else freq[0], "reliability_index": ri if many else float(ri[0])}
    a, b, group_shape = grouped
    bins = engine.rank_histogram(plist, tlist, group_shape=group_shape)  # (T, G, N + 1)
    bins = bins.reshape(len(plist), *shape[a:b + 1], bins.shape[-1])
    freq, ri = rank_histogram_frequencies(bins if many else bins[0])
    return {"rank_hist": freq, "reliability_index": ri}


def eval_rank_histograms(results: Dict[str, Tensor], engine: HipEngine, split: str = "val", infix: Optional[str] = None) -> Dict[str, object]:
    """`{split}/{infix}t{k}/rank_hist` (a float64 array (N + 1,) of frequencies) and `.../t{k}/reliability_index` (a float) for every
    `t{k}_preds` / `t{k}_targets` pair of an evaluation step's output, and `{split}/{infix}avg/...`, their means over the horizons;
    horizons of equal shape are the segments of one `rank_histogram` call."""
    infix = "" if infix is None else infix
    shapes: Dict[tuple, list] = {}
    for prefix, key, tkey in _horizon_pairs(results):
        shapes.setdefault((tuple(results[key].shape), tuple(results[tkey].shape)), []).append((prefix, key, tkey))
    out: Dict[str, object] = {}
    hists, indices = [], []
    for members in shapes.values():
        bins = engine.rank_histogram([results[k] for _, k, _ in members], [results[t] for _, _, t in members])[:, 0].cpu().numpy()
        freq, ri = rank_histogram_frequencies(bins)
        for s, (prefix, _, _) in enumerate(members):
            out[f"{split}/{infix}{prefix}/rank_hist"] = freq[s]
            out[f"{split}/{infix}{prefix}/reliability_index"] = float(ri[s])
            hists.append(freq[s])
            indices.append(float(ri[s]))
    if hists and all(h.shape == hists[0].shape for h in hists):
        out[f"{split}/{infix}avg/rank_hist"] = np.mean(hists, axis=0)
    if indices:
        out[f"{split}/{infix}avg/reliability_index"] = float(sum(indices) / len(indices))
    return out


def _energy_inputs(predictions, targets, per_channel: bool):
    """(prediction list, target list, lists were given, (outer, groups, inner)) for the energy score of (N, B, C, *spatial) forecasts:
    one vector per sample (the whole field), or per sample and channel."""
    many = not torch.is_tensor(predictions)
    plist, tlist = (list(predictions), list(targets)) if many else ([predictions], [targets])
    if many and (len(plist) != len(tlist) or not plist):
        raise ValueError(f"{len(plist)} prediction horizons but {len(tlist)} target horizons")
    for p, t in zip(plist, tlist):
        if p.shape[1] != t.shape[0]:
            raise AssertionError(f"predictions.shape[1] ({p.shape[1]}) != targets.shape[0] ({t.shape[0]})")
        if not p.is_cuda or not t.is_cuda:
            raise ValueError("dyffusion_amd.metrics works on GPU tensors (the HIP engine computes them)")
    return plist, tlist, many, _field_group_shape(tuple(tlist[0].shape), per_channel)


def _field_group_shape(tshape: Sequence[int], per_channel: bool) -> Tuple[int, int, int]:
    """(B, 1, C * spatial) or (B, C, spatial) of targets (B, C, *spatial); without a channel axis (at most two axes) the one channel
    is everything behind the sample axis."""
    b = tshape[0]
    c = tshape[1] if per_channel and len(tshape) >= 3 else 1
    return b, c, math.prod(tshape) // (b * c)


def evaluate_ensemble_energy_score(predictions, targets, engine: HipEngine, per_channel: bool = False) -> Dict[str, object]:
    """The energy score of an ensemble of fields, the multivariate CRPS: {"es", "es_fair", "dist_target", "dist_pair"} (ENERGY_ROWS)
    in one pass of `energy_score_kernel`.  predictions (n_members, B, C, *spatial), targets (B, C, *spatial), on the engine's GPU.
    Every sample's whole field is one vector and the scores are means over the samples: host floats; with `per_channel` every
    (sample, channel) is a vector and each score is a float64 device tensor (C,), nothing synchronised.  es = E||x - y|| - (N - 1) /
    (2 N) E||x - x'|| (1 / N^2 weights, as the engine's CRPS), es_fair divides the pair sum by N (N - 1) instead.  Lists of equally
    shaped horizons go through as the segments of one call and give a leading axis (host arrays when not per channel)."""
    plist, tlist, many, group_shape = _energy_inputs(predictions, targets, per_channel)
    out = engine.energy_score(plist, tlist, group_shape=group_shape)  # (4, T, G)
    if per_channel:
        return {m: (out[i] if many else out[i, 0]) for i, m in enumerate(ENERGY_ROWS)}
    host = out[:, :, 0].cpu().numpy()
    return {m: (host[i] if many else float(host[i, 0])) for i, m in enumerate(ENERGY_ROWS)}


def evaluate_member_distances(predictions, targets, engine: HipEngine, per_channel: bool = False) -> Dict[str, Tensor]:
    """The ensemble-diversity diagnostics behind the energy score, as float64 device tensors (nothing synchronised): {"member_dist":
    (N,) every member's Euclidean distance to the truth (its multivariate skill), "pair_dist": (N, N) the distances between the
    members (symmetric, zero diagonal: which members collapsed onto each other, which is the outlier)}, means over the samples of
    the whole-field distances; with `per_channel` (C, N) and (C, N, N).  Inputs as `evaluate_ensemble_energy_score`; lists of
    horizons give a leading axis."""
    plist, tlist, many, group_shape = _energy_inputs(predictions, targets, per_channel)
    _, mats = engine.energy_score(plist, tlist, group_shape=group_shape, members=True, pairs=True)
    out = {}
    for k, v in mats.items():  # (T, G, ...)
        v = v if per_channel else v[:, 0]
        out[k] = v if many else v[0]
    return out


def eval_energy_scores(results: Dict[str, Tensor], engine: HipEngine, split: str = "val", infix: Optional[str] = None) -> Dict[str, float]:
    """`{split}/{infix}t{k}/es` and `.../es_fair` (whole-field energy scores, means over the samples) for every `t{k}_preds` /
    `t{k}_targets` pair of an evaluation step's output, their means over the horizons `{split}/{infix}avg/...`, and per channel j of
    (B, C, ...) targets `{split}/{infix}t{k}/c{j}/es`; horizons of equal shape are the segments of one `energy_score` call each."""
    infix = "" if infix is None else infix
    shapes: Dict[tuple, list] = {}
    for prefix, key, tkey in _horizon_pairs(results):
        shapes.setdefault((tuple(results[key].shape), tuple(results[tkey].shape)), []).append((prefix, key, tkey))
    out: Dict[str, float] = {}
    acc = defaultdict(list)
    for (_, tshape), members in shapes.items():
        plist, tlist = [results[k] for _, k, _ in members], [results[t] for _, _, t in members]
        field = engine.energy_score(plist, tlist, group_shape=_field_group_shape(tshape, False)).cpu().numpy()  # (4, segments, 1)
        per_c = engine.energy_score(plist, tlist, group_shape=_field_group_shape(tshape, True)).cpu().numpy()  # (4, segments, C)
        for s, (prefix, _, _) in enumerate(members):
            for m in ("es", "es_fair"):
                v = float(field[ENERGY_ROWS.index(m), s, 0])
                out[f"{split}/{infix}{prefix}/{m}"] = v
                acc[f"{split}/{infix}avg/{m}"].append(v)
            for j in range(per_c.shape[2]):
                out[f"{split}/{infix}{prefix}/c{j}/es"] = float(per_c[0, s, j])
    for k, v in acc.items():
        out[k] = float(sum(v) / len(v))
    return out


SPECTRUM_ROWS = ("spread", "mean", "target", "error")  # plane order of the (S, C, 4, n_bins + 1) tensor of HipEngine.power_spectrum


def spectrum_diagnostics(planes: Tensor, n_members: int) -> Dict[str, Tensor]:
    """What follows from the four spectra `planes` (..., 4, n_bins + 1) of `HipEngine.power_spectrum` (last column: the totals), all
    float64 on the planes' device, nothing synchronised: the planes themselves (..., n_bins) and "total" (..., 4); "members" = spread +
    mean, the mean power spectrum of the single members (exact: the anomalies sum to zero; a sum of positives); "spread_fair" = spread
    N / (N - 1) (NaN for one member); "wavenumber" = arange(n_bins); "spectral_ssr"[k] = sqrt((N + 1) / N spread_fair / error), the
    spread-skill ratio per scale; "coherence"[k] = (mean + target - error) / (2 sqrt(mean target)), the real coherence of ensemble
    mean and truth per shell; "lsd" / "lsd_ens_mean" (...): the log-spectral distances in dB, sqrt(mean_k (10 log10(P / target))^2)
    over the bins 1 .. n_bins - 1 with positive target power, P = members / P = mean."""
    n_bins = planes.shape[-1] - 1
    out = {name: planes[..., i, :n_bins] for i, name in enumerate(SPECTRUM_ROWS)}
    out["total"] = planes[..., n_bins]
    out["members"] = out["spread"] + out["mean"]
    out["spread_fair"] = out["spread"] * (n_members / (n_members - 1.0) if n_members > 1 else float("nan"))
    out["wavenumber"] = torch.arange(n_bins, device=planes.device)
    out["spectral_ssr"] = torch.sqrt((n_members + 1.0) / n_members * out["spread_fair"] / out["error"])
    out["coherence"] = (out["mean"] + out["target"] - out["error"]) / (2.0 * torch.sqrt(out["mean"] * out["target"]))
    target = out["target"][..., 1:]
    use = target > 0
    for key, power in (("lsd", out["members"]), ("lsd_ens_mean", out["mean"])):
        db = 10.0 * torch.log10(power[..., 1:] / torch.where(use, target, torch.ones_like(target)))
        out[key] = torch.sqrt(torch.where(use, db * db, torch.zeros_like(db)).sum(-1) / use.sum(-1))
    return out


def evaluate_power_spectrum(predictions, targets, engine: HipEngine, window: str = "none") -> Dict[str, object]:
    """The ensemble's scores by spatial scale, in one pass of `power_spectrum_kernel`: the radially binned power spectra "spread",
    "mean", "target", "error" per channel and everything `spectrum_diagnostics` derives from them, plus the int "n_bins".
    predictions (n_members, B, C, H, W), targets (B, C, H, W), on the engine's GPU: spectra (C, n_bins), "total" (C, 4), "lsd" (C,);
    lists of equally shaped horizons go through as the segments of one call and give a leading axis.  `window` "hann" tapers the
    (non-periodic) fields.  Everything stays on the device in float64; nothing is synchronised until the caller reads."""
    many = not torch.is_tensor(predictions)
    res = engine.power_spectrum(predictions, targets, window=window)
    n = (predictions[0] if many else predictions).shape[0]
    out: Dict[str, object] = spectrum_diagnostics(res["planes"] if many else res["planes"][0], n)
    out["n_bins"] = res["n_bins"]
    return out


def eval_power_spectra(outputs: Sequence[Dict[str, Tensor]], engine: HipEngine, split: str = "val", infix: Optional[str] = None,
                       window: str = "none") -> Dict[str, float]:
    """`{split}/{infix}t{k}/lsd`, `.../lsd_ens_mean` (the log-spectral distances of the channel-mean spectra), their means over the
    horizons `{split}/{infix}avg/...` and per channel j `{split}/{infix}t{k}/c{j}/lsd`, for every `t{k}_preds` / `t{k}_targets` pair of
    an epoch's evaluation-step outputs.  The spectra of every batch are added on the device, weighted by the batch's samples (the
    horizons of one batch are the segments of one `power_spectrum` call); the host reads once, at the end."""
    infix = "" if infix is None else infix
    pairs = list(_horizon_pairs(outputs[0]))
    total, samples, n = None, 0, None
    for o in outputs:
        plist, tlist = [o[k] for _, k, _ in pairs], [o[t] for _, _, t in pairs]
        planes = engine.power_spectrum(plist, tlist, window=window)["planes"]  # (horizons, C, 4, n_bins + 1), the mean over the batch
        b, n = tlist[0].shape[0], plist[0].shape[0]
        total = planes * float(b) if total is None else total + planes * float(b)
        samples += b
    mean = total / float(samples)
    pooled, per_c = spectrum_diagnostics(mean.mean(dim=1), n), spectrum_diagnostics(mean, n)
    host = torch.cat([pooled["lsd"][:, None], pooled["lsd_ens_mean"][:, None], per_c["lsd"]], dim=1).cpu().numpy()  # (horizons, 2 + C)
    out: Dict[str, float] = {}
    for s, (prefix, _, _) in enumerate(pairs):
        out[f"{split}/{infix}{prefix}/lsd"], out[f"{split}/{infix}{prefix}/lsd_ens_mean"] = float(host[s, 0]), float(host[s, 1])
        for j in range(host.shape[1] - 2):
            out[f"{split}/{infix}{prefix}/c{j}/lsd"] = float(host[s, 2 + j])
    out[f"{split}/{infix}avg/lsd"], out[f"{split}/{infix}avg/lsd_ens_mean"] = float(host[:, 0].mean()), float(host[:, 1].mean())
    return out


def _horizon_pairs(results: Dict[str, Tensor]):
    """(prefix, predictions key, targets key) of every `t{k}_preds` / `t{k}_targets` pair, in the order of `results`."""
    for key in [k for k in results if k.endswith("preds")]:
        prefix = key.split("_")[0] if key != "preds" else ""
        tkey = f"{prefix}_targets" if prefix else "targets"
        if tkey in results:
            yield prefix, key, tkey


def _eval_extended(results: Dict[str, Tensor], engine: HipEngine, stem: str, extended: bool, per_channel: bool) -> Dict[str, float]:
    """The keys that `extended` / `per_channel` add to `eval_ensemble_predictions`; horizons of equal shape are the segments of one
    `ensemble_scores` call per flag."""
    shapes: Dict[tuple, list] = {}
    for prefix, key, tkey in _horizon_pairs(results):
        shapes.setdefault((tuple(results[key].shape), tuple(results[tkey].shape)), []).append((prefix, key, tkey))
    out: Dict[str, float] = {}
    acc = defaultdict(list)
    for (_, tshape), members in shapes.items():
        plist, tlist = [results[k] for _, k, _ in members], [results[t] for _, _, t in members]
        if extended:
            pooled = engine.ensemble_scores(plist, tlist).cpu().numpy()  # (5, segments, 1)
            for s, (prefix, _, _) in enumerate(members):
                for m in ("nll", "corr"):
                    v = float(pooled[SCORE_ROWS.index(m), s, 0])
                    out[f"{stem}{prefix}/{m}"] = v
                    acc[f"{stem}avg/{m}"].append(v)
        if per_channel:  # targets (B, C, ...); without a channel axis (at most two axes) the one channel is everything
            b, c = (tshape[0], tshape[1]) if len(tshape) >= 3 else (1, 1)
            per_c = engine.ensemble_scores(plist, tlist, group_shape=(b, c, math.prod(tshape) // (b * c))).cpu().numpy()
            for s, (prefix, _, _) in enumerate(members):
                for j in range(c):
                    for i, m in enumerate(SCORE_ROWS):
                        v = float(per_c[i, s, j])
                        out[f"{stem}{prefix}/c{j}/{m}"] = v
                        acc[f"{stem}avg/c{j}/{m}"].append(v)
    for k, v in acc.items():
        out[k] = float(sum(v) / len(v))
    return out


def eval_ensemble_predictions(results: Dict[str, Tensor], engine: HipEngine, split: str = "val", infix: Optional[str] = None,
                              extended: bool = False, per_channel: bool = False) -> Dict[str, float]:
    """_base_experiment.py:617-640: per-horizon metrics `{split}/{infix}t{k}/{m}` for every `t{k}_preds`/`t{k}_targets`
    pair of an evaluation step's output, plus their average over horizons `{split}/{infix}avg/{m}`.  `extended` adds
    `{split}/{infix}t{k}/nll` and `/corr` with their `avg`; `per_channel` adds `{split}/{infix}t{k}/c{j}/{m}` for the five scores
    of SCORE_ROWS and every channel j of (B, C, ...) targets, and `{split}/{infix}avg/c{j}/{m}` (both from `ensemble_scores_kernel`;
    the keys above keep their values and their kernel)."""
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
    if extended or per_channel:
        out.update(_eval_extended(results, engine, f"{split}/{infix}", extended, per_channel))
    return out


class TrajectoryMetricsAccumulator:
    """The test epoch of a PhysicalSystemsBenchmarkDataModule (forecasting_multi_horizon.py:231-279): every test instance gives
    the curves mse / ssr / crps over its T horizon steps, the epoch reports their mean over instances.  The sum of the curves
    stays on the device ((3, T) float64, added to by the kernel itself); `compute()` makes the only device-to-host copy."""

    def __init__(self, engine: HipEngine, by_size: bool = False, rank_histogram: bool = False, energy_score: bool = False):
        self._engine = engine
        self._energy_score = energy_score  # also the (4, T, 1) sum of the whole-field energy scores (HipEngine.energy_score)
        self._by_size = by_size  # also the (4, T, N) sum of the ensemble-size curves (HipEngine.ensemble_size_metrics)
        self._rank_histogram = rank_histogram  # also the (T, 1, N + 1) sum of the pooled rank histograms (HipEngine.rank_histogram)
        self.reset()

    def reset(self) -> None:
        self._sum: Optional[Tensor] = None
        self._size_sum: Optional[Tensor] = None
        self._hist_sum: Optional[Tensor] = None
        self._energy_sum: Optional[Tensor] = None
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
        if self._rank_histogram:
            n = preds_list[0].shape[0]
            if self._hist_sum is None:
                self._hist_sum = torch.zeros(len(preds_list), 1, n + 1, dtype=torch.float64, device=preds_list[0].device)
            elif n + 1 != self._hist_sum.shape[2]:
                raise ValueError(f"{n} members, but the accumulated rank histograms have {self._hist_sum.shape[2] - 1}")
            self._engine.rank_histogram(preds_list, targets_list, accum=self._hist_sum)
        if self._energy_score:  # one vector per sample of the instance: its whole field
            if self._energy_sum is None:
                self._energy_sum = torch.zeros(4, len(preds_list), 1, dtype=torch.float64, device=preds_list[0].device)
            self._engine.energy_score(preds_list, targets_list, group_shape=_field_group_shape(tuple(targets_list[0].shape), False),
                                      accum=self._energy_sum)
        self.count += 1
        return curves

    def compute(self) -> Dict[str, np.ndarray]:
        """{metric: (T,) float64 array}: the mean over the instances seen since the last reset ({} before the first update); with
        `by_size` also "by_size": the (4, T, N) mean of the ensemble-size curves (planes SIZE_ROWS); with `rank_histogram` also
        "rank_hist": the (T, N + 1) frequencies of the rank histograms summed over the instances; with `energy_score` also "es": the
        (T,) mean of the instances' whole-field energy scores."""
        if self._sum is None or self.count == 0:
            return {}
        mean = self._sum.cpu().numpy() / float(self.count)
        out = {m: mean[i] for i, m in enumerate(METRIC_ROWS)}
        if self._size_sum is not None:
            out["by_size"] = self._size_sum.cpu().numpy() / float(self.count)
        if self._hist_sum is not None:
            out["rank_hist"] = rank_histogram_frequencies(self._hist_sum[:, 0].cpu().numpy())[0]
        if self._energy_sum is not None:
            out["es"] = self._energy_sum[ENERGY_ROWS.index("es"), :, 0].cpu().numpy() / float(self.count)
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
