"""Time the on-device forecast products (HipEngine.ensemble_products: mean + std + the 5 / 50 / 95 % quantiles per grid point, one
launch over every horizon) against the torch expressions they replace, on the same tensors in the same process, at the Navier-Stokes
evaluation shapes (N, B, 3, 221, 42): N = 20 (validation) and 50 (test), B = eval_batch_size 4, the 16 horizons as the segments of
one call.
  products        one ensemble_products call: five planes per segment
  torch           per horizon `p.mean(0)`, `p.std(0, unbiased=False)`, `torch.quantile(p, q, dim=0)`
  torch_moments   per horizon the two moments only (what the quantiles cost torch shows in the difference)
  products_moments the same two planes from ensemble_products
  rank_histogram  one rank_histogram call, pooled, against targets drawn beside the members
  torch_rank_histogram per horizon `torch.bincount((p < t).sum(0).flatten(), minlength=N + 1)`: the same bins but for the tied points
Times are HIP events around the calls, warm; the ways alternate call by call and each runs until it has `--window` seconds of timed
work (at least a second); the median, the extremes and the count are reported.  GB/s = the bytes a call must move -- every prediction
read once, every plane written once; for the histograms every prediction and target read once -- over the median, beside the
8.0 TB/s HBM peak: the time is a call's (the launches and the pointer-table upload), not a kernel's.  The same bytes are charged to
the torch side so the columns compare.
usage: python tools/bench_ensemble_products.py [--window 1.5] [--out profiles/ensemble_products_bench.json]   -> one JSON line per shape"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyffusion_amd as D  # noqa: E402
from bench_ensemble_scores import HBM_PEAK_GB_S, measure  # noqa: E402
from dyffusion_amd.engine import net_config  # noqa: E402

QUANTILES = (0.05, 0.5, 0.95)
SHAPES = [  # name, N, segments (horizons), (B, C, H, W)
    ("ns_val", 20, 16, (4, 3, 221, 42)),
    ("ns_test", 50, 16, (4, 3, 221, 42)),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.5, help="seconds of timed work per way and shape (at least 1)")
    ap.add_argument("--shapes", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_products_bench.json"))
    a = ap.parse_args()
    if a.window < 1.0:
        raise SystemExit("--window must be at least a second")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_products needs the GPU: nothing is measured without one")
    cfg = net_config(in_channels=1, cond_channels=0, out_channels=1, dim=8, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False)
    rows = []
    for name, n, segs, (b, c, h, w) in SHAPES:
        if name not in a.shapes:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        preds = [0.6 * torch.randn(n, b, c, h, w, generator=g, device="cuda") + 0.1 for _ in range(segs)]
        targets = [0.6 * torch.randn(b, c, h, w, generator=g, device="cuda") + 0.1 for _ in range(segs)]
        q = torch.tensor(QUANTILES, device="cuda")
        points = b * c * h * w

        def torch_all():
            return [(p.mean(0), p.std(0, unbiased=False), torch.quantile(p, q, dim=0)) for p in preds]

        def torch_moments():
            return [(p.mean(0), p.std(0, unbiased=False)) for p in preds]

        def torch_hist():
            return [torch.bincount((p < t[None]).sum(0).flatten(), minlength=n + 1) for p, t in zip(preds, targets)]

        ways = {"products": lambda: eng.ensemble_products(preds, quantiles=QUANTILES),
                "torch": torch_all,
                "products_moments": lambda: eng.ensemble_products(preds),
                "torch_moments": torch_moments,
                "rank_histogram": lambda: eng.rank_histogram(preds, targets),
                "torch_rank_histogram": torch_hist}
        planes = {"products": 5, "torch": 5, "products_moments": 2, "torch_moments": 2, "rank_histogram": 1, "torch_rank_histogram": 1}
        # the two sides compute the same fields
        fields, names = eng.ensemble_products(preds, quantiles=QUANTILES)
        old = torch.stack([torch.cat([m[None], s[None], qs]) for m, s, qs in torch_all()])
        worst = {nm: float((fields[:, k] - old[:, k]).abs().max()) for k, nm in enumerate(names)}
        bins = eng.rank_histogram(preds, targets)[:, 0]
        # fp32 draws do tie now and then: a tied point's weight is split over its bins here and sits in one bin there
        tied = sum(int((p == t[None]).any(0).sum()) for p, t in zip(preds, targets))
        hist_diff = float((bins - torch.stack(torch_hist()).to(torch.float64)).abs().max())
        times = measure(ways, a.window)
        row = {"shape": name, "device": torch.cuda.get_device_name(0), "members": n, "segments": segs, "field_shape": [b, c, h, w],
               "planes": names, "window_s": a.window, "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "worst_abs_diff_products_vs_torch": worst,
               "rank_histogram_vs_torch_bincount": {"worst_abs_bin_diff": hist_diff, "tied_points": tied,
                                                    "bins_sum_to_points": bool(torch.all(bins.sum(1) == float(points)))}}
        for k, v in times.items():
            med = statistics.median(v)
            nbytes = 4.0 * points * segs * (n + planes[k])
            row[k] = {"calls": len(v), "bytes": nbytes, "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "gb_per_s": round(nbytes / med / 1e6, 1), "share_of_hbm_peak": round(nbytes / med / 1e6 / HBM_PEAK_GB_S, 4)}
        for ours, theirs in (("products", "torch"), ("products_moments", "torch_moments"), ("rank_histogram", "torch_rank_histogram")):
            row[f"{theirs}_over_{ours}"] = round(row[theirs]["ms_median"] / row[ours]["ms_median"], 3)
            row[f"{ours}_faster_with_disjoint_ranges"] = row[ours]["ms_max"] < row[theirs]["ms_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del preds, targets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_ensemble_products.py", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
