"""Time the on-device radial power spectra (HipEngine.power_spectrum: spread / mean / target / error shells of every horizon in one call,
the member stack read in place) against the torch route it replaces, on the same tensors in the same process:
  power_spectrum  one power_spectrum call over all horizons
  torch           per horizon: `mean(0)`, the subtractions, `torch.fft.rfft2` of the anomalies, the mean, the target and the error,
                  `abs() ** 2` with the half-spectrum weights, `index_add_` into the shells by the same bin map (atomics: not repeatable)
Shapes: the Navier-Stokes validation shape (N = 50, 3 x 221 x 42, B = eval_batch_size 4, 16 horizons) and the OISST one (N = 50, 1 x
60 x 60, B = 6, 7 horizons), the shapes of tools/bench_ensemble_scores.py.  Times are HIP events around the calls, warm (two untimed
calls per way and shape first); the ways alternate call by call and each runs until it has `--window` seconds of timed work (at least a
second); the median, the extremes and the count are reported.  Neither side's result is read back inside the timed region.  Where
`torch.fft` does not work on the device the engine's time is reported alone, and the row says so.  `share_of_fp32_matrix_peak` is the
column DFT's 2 x 4 H^2 (W / 2 + 1) flop per field (padded tiles not counted) over the median time, against 157.3 TFLOP/s.
usage: python tools/bench_power_spectrum.py [--window 1.5] [--out profiles/power_spectrum_bench.json]   -> one JSON line per shape"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dyffusion_amd as D  # noqa: E402
from bench_ensemble_scores import measure  # noqa: E402
from dyffusion_amd.engine import net_config  # noqa: E402

SHAPES = [  # name, N, segments (horizons), (B, C, H, W)
    ("ns_val", 50, 16, (4, 3, 221, 42)),
    ("oisst_val", 50, 7, (6, 1, 60, 60)),
]
FP32_MATRIX_PEAK = 157.3e12


def half_bin_map(h, w):
    """(bins (H, W // 2 + 1) with the corners sent to n_bins, weights (W // 2 + 1,)) by the integer rule of include/dyffusion_hip.h."""
    big, wh = max(h, w), w // 2 + 1
    ky, kx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(wh, dtype=np.int64), indexing="ij")
    kyf = np.minimum(ky, h - ky)
    num, den = 4 * big * big * (kx * kx * h * h + kyf * kyf * w * w), h * h * w * w
    k = np.floor(np.sqrt(num / (4.0 * den)) + 0.5).astype(np.int64)
    k += ((2 * k + 1) ** 2 * den <= num)
    k -= ((k > 0) & ((2 * k - 1) ** 2 * den > num))
    weights = np.full(wh, 2.0)
    weights[0] = 1.0
    if w % 2 == 0:
        weights[-1] = 1.0
    return np.minimum(k, big // 2 + 1), weights


def torch_route(preds, targets, bins, weights, n_bins):
    """(horizons, C, 4, n_bins + 1) float64: shells and, last, the corners -- what a user computes by hand today."""
    out = []
    for p, t in zip(preds, targets):
        n, b, c, h, w = p.shape
        mean = p.mean(0)
        fields = torch.cat([p - mean, mean[None], t[None], (mean - t)[None]])  # (N + 3, B, C, H, W)
        power = (torch.fft.rfft2(fields).abs() ** 2 * weights).to(torch.float64) / float(h * w) ** 2
        planes = torch.cat([power[:n].mean(0, keepdim=True), power[n:]]).mean(1)  # (4, C, H, Wh)
        shells = torch.zeros(4, c, n_bins + 1, dtype=torch.float64, device=p.device)
        shells.index_add_(2, bins, planes.reshape(4, c, -1))
        out.append(shells.permute(1, 0, 2))
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=float, default=1.5, help="seconds of timed work per way and shape (at least 1)")
    ap.add_argument("--shapes", nargs="*", default=[s[0] for s in SHAPES])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "power_spectrum_bench.json"))
    a = ap.parse_args()
    if a.window < 1.0:
        raise SystemExit("--window must be at least a second")
    if not torch.cuda.is_available():
        raise SystemExit("bench_power_spectrum needs the GPU: nothing is measured without one")
    cfg = net_config(in_channels=1, cond_channels=0, out_channels=1, dim=8, with_time_emb=True, upsample_dims=(64, 64), dropout=0.0)
    eng = D.HipEngine(cfg, cfg, 16, 16, max_batch=1, use_graph=False)
    rows = []
    for name, n, segs, (b, c, h, w) in SHAPES:
        if name not in a.shapes:
            continue
        g = torch.Generator(device="cuda").manual_seed(0)
        targets = [torch.randn(b, c, h, w, generator=g, device="cuda") for _ in range(segs)]
        preds = [t[None] * 0.7 + 0.6 * torch.randn(n, b, c, h, w, generator=g, device="cuda") + 0.1 for t in targets]
        n_bins = max(h, w) // 2 + 1
        bins_np, weights_np = half_bin_map(h, w)
        bins = torch.from_numpy(bins_np.reshape(-1)).cuda()
        weights = torch.from_numpy(weights_np).float().cuda()
        ways = {"power_spectrum": lambda: eng.power_spectrum(preds, targets)}
        row = {"shape": name, "device": torch.cuda.get_device_name(0), "members": n, "segments": segs, "field_shape": [b, c, h, w],
               "n_bins": n_bins, "window_s": a.window}
        try:
            theirs = torch_route(preds[:1], targets[:1], bins, weights, n_bins)
            torch.cuda.synchronize()
            ways["torch"] = lambda: torch_route(preds, targets, bins, weights, n_bins)
        except RuntimeError as err:  # no FFT back end for the device in this torch build
            row["torch"] = f"torch.fft.rfft2 is unavailable on the device ({str(err).splitlines()[0][:120]}): the engine's time alone"
            theirs = None
        if theirs is not None:  # both sides compute the same shells (the last column is total on our side, the corners on theirs)
            ours = eng.power_spectrum(preds[:1], targets[:1])["planes"][..., :n_bins]
            row["max_rel_difference_of_the_two_sides"] = float(((ours - theirs[..., :n_bins]).abs() / ours.abs()).max())
        times = measure(ways, a.window)
        for k, v in times.items():
            med = statistics.median(v)
            row[k] = {"calls": len(v), "ms_median": round(med, 4), "ms_min": round(min(v), 4), "ms_max": round(max(v), 4)}
        flop = 2.0 * 4.0 * h * h * (w // 2 + 1) * (n + 3) * b * c * segs
        row["column_dft_gflop"] = round(flop / 1e9, 3)
        row["share_of_fp32_matrix_peak"] = round(flop / (row["power_spectrum"]["ms_median"] * 1e-3) / FP32_MATRIX_PEAK, 4)
        if "torch" in times:
            row["torch_over_power_spectrum"] = round(row["torch"]["ms_median"] / row["power_spectrum"]["ms_median"], 3)
            row["power_spectrum_faster_with_disjoint_ranges"] = row["power_spectrum"]["ms_max"] < row["torch"]["ms_min"]
            row["torch_faster_with_disjoint_ranges"] = row["torch"]["ms_max"] < row["power_spectrum"]["ms_min"]
        rows.append(row)
        print(json.dumps(row), flush=True)
        del preds, targets
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/bench_power_spectrum.py", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
