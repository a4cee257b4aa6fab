"""Time the grouped ensemble scores (HipEngine.ensemble_scores: five scores per (segment, group) in one pass) against the loop they
replace, on the same tensors in the same process, at the benchmark's own evaluation shapes: Navier-Stokes (N, B, 3, 221, 42) and
OISST (N, B, 1, 60, 60) with N = num_predictions 20 (validation) and 50 (test) and B = eval_batch_size 4 / 6 of the shipped
configs, the horizons (16 / 7) as the segments of one call.
  grouped       one ensemble_scores call per shape: per channel (B, C, H W) and per sample (1, B, C H W)
  pooled        the same call with one group per segment (what the nll / corr keys cost)
  slice_loop    what a user does without it: per horizon and per group one `.contiguous()` slice of the stack (channel c: preds[:, :, c];
                sample b: preds[:, b]; a view where the slice is already contiguous) and one blocking ensemble_metrics call -- three
                of the five scores
  trajectory    one trajectory_metrics call on the same segments: three scores, pooled -- the kernel the per-point expressions come from
Times are HIP events around the calls, warm; the ways alternate call by call and each runs until it has `--window` seconds of timed
work (at least a second); the median, the extremes and the count are reported.  GB/s = the bytes of every prediction and every target read once
over the median, beside the 8.0 TB/s HBM peak: the time is a call's (two launches, the pointer-table upload), not a kernel's.
usage: python tools/bench_ensemble_scores.py [--window 1.5] [--out profiles/ensemble_scores_bench.json]   -> one JSON line per shape"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import dyffusion_amd as D  # noqa: E402
from dyffusion_amd.engine import net_config  # noqa: E402

HBM_PEAK_GB_S = 8000.0
SHAPES = [  # name, N, segments (horizons), (B, C, H, W)
    ("ns_val", 20, 16, (4, 3, 221, 42)),
    ("ns_test", 50, 16, (4, 3, 221, 42)),
    ("oisst_val", 20, 7, (6, 1, 60, 60)),
    ("oisst_test", 50, 7, (6, 1, 60, 60)),
]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def measure(ways, window):
    """Alternate the ways call by call; a way leaves the rotation once it has run `window` seconds in all (at least three calls)."""
    for fn in ways.values():  # warm every shape and way
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    full = set()
    t0 = time.perf_counter()
    while len(full) < len(ways):
        for k, fn in ways.items():
            if k in full:
                continue
            times[k].append(timed(fn))
            if len(times[k]) >= 3 and sum(times[k]) >= window * 1e3:
                full.add(k)
        if time.perf_counter() - t0 > 60.0 * len(ways):
            raise SystemExit("the timing windows did not fill within a minute per way")
    return times


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.5, help="seconds of timed work per way and shape (at least 1)")
    ap.add_argument("--shapes", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ensemble_scores_bench.json"))
    a = ap.parse_args()
    if a.window < 1.0:
        raise SystemExit("--window must be at least a second")
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_scores needs the GPU: nothing is measured without one")
    cfg = net_config(in_channels=1, cond_channels=0, out_channels=1, dim=8, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False)
    rows = []
    for name, n, segs, (b, c, h, w) in SHAPES:
        if name not in a.shapes:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        targets = [torch.randn(b, c, h, w, generator=g, device="cuda") for _ in range(segs)]
        preds = [t[None] * 0.7 + 0.6 * torch.randn(n, b, c, h, w, generator=g, device="cuda") + 0.1 for t in targets]
        points = b * c * h * w
        nbytes = 4.0 * points * segs * (n + 1)
        per_channel, per_sample = (b, c, h * w), (1, b, c * h * w)

        def channel_loop():
            return [eng.ensemble_metrics(p[:, :, j].contiguous(), t[:, j].contiguous()) for p, t in zip(preds, targets) for j in range(c)]

        def sample_loop():
            return [eng.ensemble_metrics(p[:, i:i + 1].contiguous(), t[i:i + 1].contiguous()) for p, t in zip(preds, targets) for i in range(b)]

        ways = {"grouped_per_channel": lambda: eng.ensemble_scores(preds, targets, group_shape=per_channel),
                "slice_loop_per_channel": channel_loop,
                "grouped_per_sample": lambda: eng.ensemble_scores(preds, targets, group_shape=per_sample),
                "slice_loop_per_sample": sample_loop,
                "pooled": lambda: eng.ensemble_scores(preds, targets),
                "trajectory": lambda: eng.trajectory_metrics(preds, targets)}
        # the two sides compute the same numbers
        got = eng.ensemble_scores(preds, targets, group_shape=per_channel)[:3].cpu()          # (3, segs, C)
        old = torch.tensor(channel_loop(), dtype=torch.float64).reshape(segs, c, 3).permute(2, 0, 1)
        worst_c = float(((got - old).abs() / old.abs()).max())
        got = eng.ensemble_scores(preds, targets, group_shape=per_sample)[:3].cpu()
        old = torch.tensor(sample_loop(), dtype=torch.float64).reshape(segs, b, 3).permute(2, 0, 1)
        worst_s = float(((got - old).abs() / old.abs()).max())
        times = measure(ways, a.window)
        row = {"shape": name, "device": torch.cuda.get_device_name(0), "members": n, "segments": segs, "target_shape": [b, c, h, w],
               "bytes": nbytes, "window_s": a.window, "hbm_peak_gb_per_s": HBM_PEAK_GB_S,
               "worst_rel_diff_grouped_vs_slice_loop": {"per_channel": worst_c, "per_sample": worst_s}}
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"calls": len(v), "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                      "gb_per_s": round(nbytes / med / 1e6, 1), "share_of_hbm_peak": round(nbytes / med / 1e6 / HBM_PEAK_GB_S, 4)}
        for kind in ("per_channel", "per_sample"):
            row[f"slice_loop_over_grouped_{kind}"] = round(row[f"slice_loop_{kind}"]["ms_median"] / row[f"grouped_{kind}"]["ms_median"], 3)
            row[f"grouped_{kind}_faster_with_disjoint_ranges"] = row[f"grouped_{kind}"]["ms_max"] < row[f"slice_loop_{kind}"]["ms_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del preds, targets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_ensemble_scores.py", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
