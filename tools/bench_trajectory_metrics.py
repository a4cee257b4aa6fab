"""Time the per-segment ensemble metrics of a test trajectory (HipEngine.trajectory_metrics: two launches, no host round trip)
against the per-horizon way (one HipEngine.ensemble_metrics call per segment, each ending in a stream synchronise) on the same
tensors in the same process, at the Navier-Stokes test shape by default: 50 members, 64 horizon steps, 4 x 3 x 221 x 42 points.
Times are HIP events around the calls, warm, median of the repeats (the two ways alternate); GB/s = the bytes the metrics need
(every prediction and every target once) over that time.
usage: python tools/bench_trajectory_metrics.py [--members 50] [--segments 64] [--points 4 3 221 42] [--repeats 9]   -> one JSON line"""
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
        raise SystemExit("bench_trajectory_metrics needs the GPU: nothing is measured without one")
    n, s, shape = a.members, a.segments, tuple(a.points)
    cfg = net_config(in_channels=1, cond_channels=0, out_channels=1, dim=8, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False)
    g = torch.Generator(device="cuda").manual_seed(0)
    targets = [torch.randn(*shape, generator=g, device="cuda") for _ in range(s)]
    preds = [t[None] * 0.7 + 0.6 * torch.randn(n, *shape, generator=g, device="cuda") + 0.1 for t in targets]
    strided_p, strided_t = torch.stack(preds, dim=1), torch.stack(targets, dim=0)  # (N, S, ...), (S, ...): the in-place layout
    points = targets[0].numel()
    nbytes = 4.0 * points * s * (n + 1)

    def one_call():
        return eng.trajectory_metrics(preds, targets)

    def one_call_strided():
        return eng.trajectory_metrics(strided_p, strided_t)

    def per_horizon():
        return [eng.ensemble_metrics(p, t) for p, t in zip(preds, targets)]

    ways = {"trajectory_metrics": one_call, "trajectory_metrics_strided": one_call_strided, "ensemble_metrics_per_segment": per_horizon}
    got = one_call().cpu()
    old = torch.tensor(per_horizon(), dtype=torch.float64).T  # (3, S)
    worst = float(((got - old).abs() / old.abs()).max())
    for fn in ways.values():  # warm
        fn()
        fn()
    torch.cuda.synchronize()
    times = {k: [] for k in ways}
    for _ in range(a.repeats):
        for k, fn in ways.items():
            times[k].append(timed(fn))
    clk = sclk_mhz()
    row = {"device": torch.cuda.get_device_name(0), "sclk_mhz_after": clk, "members": n, "segments": s, "points_per_segment": points,
           "bytes": nbytes, "repeats": a.repeats, "worst_rel_diff_between_the_two_ways": worst}
    for k, v in times.items():
        med = statistics.median(v)
        row[k] = {"ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4), "gb_per_s": round(nbytes / med / 1e6, 1)}
    print(json.dumps(row), flush=True)


if __name__ == "__main__":
    main()
