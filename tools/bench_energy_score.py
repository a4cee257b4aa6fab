"""Time the on-device energy score (HipEngine.energy_score: the whole-field score of every horizon, one call, the member stack read in
place) against the torch route it replaces, on the same tensors in the same process:
  energy_score    one energy_score call over all horizons, group_shape (B, 1, C * H * W): es / es_fair / dist_target / dist_pair
  energy_score_matrices  the same call with members=True, pairs=True (the (T, 1, N) and (T, 1, N, N) matrices as well)
  torch           per horizon: permute-copy (N, B, C, H, W) -> (B, N, C * H * W), `torch.cdist(x, x)`, the norms to the target, the means
Shapes: the Navier-Stokes test shape (N = 50, 3 x 221 x 42, B = eval_batch_size 4, 16 horizons) and N = 256 on the same fields (4
horizons).  Times are HIP events around the calls, warm (two untimed calls per way and shape first); the ways alternate call by call and
each runs until it has `--window` seconds of timed work (at least a second); the median, the extremes and the count are reported.
Neither side's result is read back inside the timed region; the torch route's permuted copy and (B, N, N) matrix are allocated inside
it, as a user's would be.  torch.cdist picks its matrix-multiply (Gram) form at these sizes: the difference of the two es values is
reported, with the float64 direct-difference cdist as the yardstick for both.
usage: python tools/bench_energy_score.py [--window 1.5] [--out profiles/energy_score_bench.json]   -> one JSON line per shape"""
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
from bench_ensemble_scores import measure  # noqa: E402
from dyffusion_amd.engine import net_config  # noqa: E402

SHAPES = [  # name, N, segments (horizons), (B, C, H, W)
    ("ns_test", 50, 16, (4, 3, 221, 42)),
    ("n256", 256, 4, (4, 3, 221, 42)),
]


def torch_route(preds, targets, dtype=None, mode="use_mm_for_euclid_dist_if_necessary"):
    """(es, es_fair) per horizon, the way a user computes them today."""
    out = []
    for p, t in zip(preds, targets):
        n, b = p.shape[0], p.shape[1]
        x = p.reshape(n, b, -1).permute(1, 0, 2).contiguous()  # the full copy
        y = t.reshape(b, 1, -1)
        if dtype is not None:
            x, y = x.to(dtype), y.to(dtype)
        pair = torch.cdist(x, x, compute_mode=mode).sum(dim=(1, 2))
        dist = (x - y).norm(dim=-1).mean(dim=1)
        out.append(torch.stack([(dist - pair / (2.0 * n * n)).mean(), (dist - pair / (2.0 * n * (n - 1))).mean()]))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.5, help="seconds of timed work per way and shape (at least 1)")
    ap.add_argument("--shapes", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "energy_score_bench.json"))
    a = ap.parse_args()
    if a.window < 1.0:
        raise SystemExit("--window must be at least a second")
    if not torch.cuda.is_available():
        raise SystemExit("bench_energy_score needs the GPU: nothing is measured without one")
    cfg = net_config(in_channels=1, cond_channels=0, out_channels=1, dim=8, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False)
    rows = []
    for name, n, segs, (b, c, h, w) in SHAPES:
        if name not in a.shapes:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        targets = [torch.randn(b, c, h, w, generator=g, device="cuda") for _ in range(segs)]
        preds = [t[None] * 0.7 + 0.6 * torch.randn(n, b, c, h, w, generator=g, device="cuda") + 0.1 for t in targets]
        gs = (b, 1, c * h * w)
        ways = {"energy_score": lambda: eng.energy_score(preds, targets, group_shape=gs),
                "energy_score_matrices": lambda: eng.energy_score(preds, targets, group_shape=gs, members=True, pairs=True),
                "torch": lambda: torch_route(preds, targets)}
        # the two sides compute the same scores: both against the float64 direct-difference cdist
        exact = torch_route(preds[:1], targets[:1], torch.float64, "donot_use_mm_for_euclid_dist")[0]
        ours = eng.energy_score(preds[:1], targets[:1], group_shape=gs)[:2, 0, 0]
        theirs = torch_route(preds[:1], targets[:1])[0].to(torch.float64)
        rel = lambda v: [float(abs(v[k] - exact[k]) / abs(exact[k])) for k in range(2)]  # noqa: E731
        times = measure(ways, a.window)
        row = {"shape": name, "device": torch.cuda.get_device_name(0), "members": n, "segments": segs, "field_shape": [b, c, h, w],
               "vector_points": c * h * w, "window_s": a.window,
               "rel_err_vs_float64_cdist": {"planes": ["es", "es_fair"], "energy_score": rel(ours), "torch": rel(theirs)}}
        for k, v in times.items():
            med = statistics.median(v)
            nbytes = 4.0 * b * c * h * w * segs * (n + 1)  # every prediction and target read once
            row[k] = {"calls": len(v), "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "gb_per_s_of_the_inputs": round(nbytes / med / 1e6, 1)}
        row["torch_over_energy_score"] = round(row["torch"]["ms_median"] / row["energy_score"]["ms_median"], 3)
        row["energy_score_faster_with_disjoint_ranges"] = row["energy_score"]["ms_max"] < row["torch"]["ms_min"]
        row["torch_faster_with_disjoint_ranges"] = row["torch"]["ms_max"] < row["energy_score"]["ms_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del preds, targets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_energy_score.py", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
