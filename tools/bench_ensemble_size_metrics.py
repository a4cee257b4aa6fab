"""Time the metrics as a function of the ensemble size (HipEngine.ensemble_size_metrics: every prefix preds[:n], n = 1..N, in one
pass) against what it replaces, on the same tensors in the same process, at the Navier-Stokes test shape by default: 50 members,
64 horizon steps, 4 x 3 x 221 x 42 points.
  (a) by_size          one ensemble_size_metrics call (list of segments; also timed on the (N, S, ...) tensor in place)
  (b) whole_ensemble   one trajectory_metrics call: n = N only
  (c) prefix_loop      N trajectory_metrics calls on preds[:n], n = 1..N: the only way to the curves without (a)
Times are HIP events around the calls, warm, median of the repeats (the ways alternate); GB/s = the bytes of every prediction and
every target once over that time.  (b) and (c) run code that this tool does not exercise otherwise: they are the yardstick.
usage: python tools/bench_ensemble_size_metrics.py [--members 50] [--segments 64] [--points 4 3 221 42] [--repeats 9]   -> one JSON line"""
import argparse
import json
import os
import re
import statistics
import subprocess
import sys

import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
import dyffusion_amd as D  # noqa: E402
from dyffusion_amd.engine import net_config  # noqa: E402


def sclk_mhz():
    """Current shader clock as rocm-smi shows it (-1 where it cannot be read)."""
    try:
        out = subprocess.run(["rocm-smi", "--showclocks"], capture_output=True, text=True, timeout=20).stdout
    except (OSError, subprocess.TimeoutExpired):
        return -1
    m = re.search(r"sclk clock level: \d+: \((\d+)Mhz\)", out)
    return int(m.group(1)) if m else -1


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=50)
    ap.add_argument("--segments", type=int, default=64)
    ap.add_argument("--points", type=int, nargs="+", default=[4, 3, 221, 42])
    ap.add_argument("--repeats", type=int, default=9)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_ensemble_size_metrics needs the GPU: nothing is measured without one")
    n, s, shape = a.members, a.segments, tuple(a.points)
    cfg = net_config(in_channels=1, cond_channels=0, out_channels=1, dim=8, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False)
    g = torch.Generator(device="cuda").manual_seed(0)
    targets = [torch.randn(*shape, generator=g, device="cuda") for _ in range(s)]
    preds = [t[None] * 0.7 + 0.6 * torch.randn(n, *shape, generator=g, device="cuda") + 0.1 for t in targets]
    strided_p, strided_t = torch.stack(preds, dim=1), torch.stack(targets, dim=0)  # (N, S, ...), (S, ...): the in-place layout
    prefixes = [[p[:k] for p in preds] for k in range(1, n + 1)]  # views: contiguous, nothing is copied
    points = targets[0].numel()
    nbytes = 4.0 * points * s * (n + 1)

    def by_size():
        return eng.ensemble_size_metrics(preds, targets)

    def by_size_strided():
        return eng.ensemble_size_metrics(strided_p, strided_t)

    def whole_ensemble():
        return eng.trajectory_metrics(preds, targets)

    def prefix_loop():
        return [eng.trajectory_metrics(p, targets) for p in prefixes]

    ways = {"by_size": by_size, "by_size_strided": by_size_strided, "whole_ensemble": whole_ensemble, "prefix_loop": prefix_loop}
    got = by_size()[:3].cpu()                                    # (3, S, N)
    old = torch.stack(prefix_loop(), dim=2).cpu()                # (3, S, N)
    diff = (got - old).abs() / old.abs().clamp_min(1e-300)
    diff[1, :, 0] = (got[1, :, 0] - old[1, :, 0]).abs()          # ssr of one member: 0 against 0
    worst = float(diff.max())
    for fn in ways.values():  # warm
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():
            times[k].append(timed(fn))
    clk = sclk_mhz()
    groups = min(-(-points // (256 if n <= 64 else 64)), 64)
    row = {"device": torch.cuda.get_device_name(0), "sclk_mhz_after": clk, "members": n, "segments": s, "points_per_segment": points,
           "bytes": nbytes, "repeats": a.repeats, "worst_rel_diff_by_size_vs_prefix_loop": worst,
           "workspace_bytes": 8 * 4 * n * groups * s}
    for k, v in times.items():
        med = statistics.median(v)
        row[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "gb_per_s": round(nbytes / med / 1e6, 1)}
    row["by_size_over_whole_ensemble"] = round(row["by_size"]["ms_median"] / row["whole_ensemble"]["ms_median"], 3)
    row["by_size_faster_than_prefix_loop_with_disjoint_ranges"] = row["by_size"]["ms_max"] < row["prefix_loop"]["ms_min"]
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
