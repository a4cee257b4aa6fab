#!/usr/bin/env python
"""What does the deterministic training mode cost, and what does it buy?  For one configuration, prints ONE JSON line with
  * the time of a training step (p_losses + backward, dropout on, both loss terms) with the mode off and on, the two alternating
    in one process (median and range of `--reps` steps each),
  * the run-to-run distance of the default mode's gradients between two identical steps (same weights, inputs and dropout seed):
    max over parameters of |g1 - g2| / |g1| (a parameter whose true gradient is zero, such as a conv bias in front of a BatchNorm, holds
    rounding noise only and reads ~1), and the same ratio over the whole gradient,
  * the same distance with the mode on, which must be 0.

    python tools/train_determinism.py --config ns    [--rows 32] [--precision 32]   # NS shapes: unet_simple dim 64 @ 256^2
    python tools/train_determinism.py --config oisst [--rows 64] --precision 16     # OISST shapes: unet.Unet dim 64, mults (1, 2, 4)
    python tools/train_determinism.py --small                                       # the 23x11 test pair (dim 64 @ 64^2), 3 rows

Needs an MI355X.  Imports neither the oracle nor the reference.
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dyffusion_amd as D  # noqa: E402
from tools.precision_drift import random_state  # noqa: E402


def make(config, rows, precision):
    """(DYffusion in train mode, the arguments of one p_losses call) of `config`."""
    g = torch.Generator().manual_seed(3)
    common = dict(interpolate_before_t1=True, lambda_reconstruction=1.0, lambda_reconstruction2=0.5, loss_function="l1", max_batch=rows,
                  use_graph=False, train_precision=precision)
    if config in ("ns", "small"):
        hw, up, h = ((221, 42), [256, 256], 16) if config == "ns" else ((23, 11), [64, 64], 4)
        kw = dict(dim=64, with_time_emb=True, outer_sample_mode="bilinear", upsample_dims=up, dropout=0.15)
        F = D.UNet(num_input_channels=3, num_output_channels=3, num_conditional_channels=2, spatial_shape=hw, **kw)
        I = D.UNet(num_input_channels=6, num_output_channels=3, num_conditional_channels=2, spatial_shape=hw, **kw)
        F.load_state_dict(random_state(F, 0))
        I.load_state_dict(random_state(I, 1))
        m = D.DYffusion(F, D.InterpolatorHandle(I, h), timesteps=h, forward_conditioning="none", schedule="before_t1_only", **common)
        batch = dict(xt_last=torch.randn(rows, 3, *hw, generator=g).cuda(), condition=torch.randn(rows, 3, *hw, generator=g).cuda(),
                     t=torch.randint(0, h, (rows,), generator=g).cuda(), static_condition=torch.rand(rows, 2, *hw, generator=g).cuda())
    else:
        kw = dict(dim=64, dim_mults=(1, 2, 4), with_time_emb=True)
        F = D.Unet(num_input_channels=1, num_output_channels=1, num_conditional_channels=1, block_dropout=0.3, attn_dropout=0.1, **kw)
        I = D.Unet(num_input_channels=2, num_output_channels=1, num_conditional_channels=0, block_dropout=0.6, block_dropout1=0.2,
                   attn_dropout=0.6, **kw)
        F.load_state_dict(random_state(F, 0, 0.5))
        I.load_state_dict(random_state(I, 1, 0.5))
        m = D.DYffusion(F, D.InterpolatorHandle(I, 7), timesteps=7, forward_conditioning="data+noise", additional_interpolation_steps=25,
                        **common)
        batch = dict(xt_last=torch.randn(rows, 1, 60, 60, generator=g).cuda(), condition=torch.randn(rows, 1, 60, 60, generator=g).cuda(),
                     t=torch.randint(0, m.num_timesteps, (rows,), generator=g).cuda(), static_condition=None)
    m.train()
    return m, batch


def step(m, batch, mode, seed, keep=False):
    """One step under `mode` from the same dropout stream -> (seconds, loss, gradients or None)."""
    m.train_set_deterministic(mode)
    m.seed(seed)
    torch.manual_seed(seed)  # the noise of forward_conditioning="data+noise" comes from torch's generator, as in the reference
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = m.p_losses(**batch)
    out["loss"].backward()
    loss = float(out["loss"].detach())
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    grads = {k: p.grad.detach().clone() for k, p in m.model.named_parameters()} if keep else None
    for p in m.model.parameters():
        p.grad = None
    return dt, loss, grads


def distance(a, b):
    """max over parameters of |a - b| / |a| (a parameter whose gradient is zero in both counts 0) and where it is reached."""
    worst, where = 0.0, None
    for k in a:
        n = float(a[k].double().norm())
        d = float((a[k].double() - b[k].double()).norm())
        r = d / n if n > 0 else (0.0 if d == 0 else float("inf"))
        if r > worst:
            worst, where = r, k
    return worst, where


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", choices=["ns", "oisst"], default="ns")
    ap.add_argument("--small", action="store_true", help="the 23x11 test pair instead of --config")
    ap.add_argument("--rows", type=int, default=None, help="batch rows of the step (ns 32, oisst 64, small 3)")
    ap.add_argument("--precision", type=int, choices=[32, 16, 48], default=32, help="operand precision of the training convs (48 = bf16x3)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=5, help="timed steps per mode")
    a = ap.parse_args()
    config = "small" if a.small else a.config
    rows = a.rows or {"ns": 32, "oisst": 64, "small": 3}[config]
    m, batch = make(config, rows, a.precision)
    res = dict(config=config, rows=rows, precision=a.precision, seed=a.seed, reps=a.reps)
    for mode in (False, True):  # warm both modes: first-use allocations, the workspace
        step(m, batch, mode, a.seed)
    times = {False: [], True: []}
    for _ in range(a.reps):
        for mode in (False, True):
            times[mode].append(step(m, batch, mode, a.seed)[0])
    for mode, key in ((False, "default"), (True, "deterministic")):
        ms = [1e3 * v for v in times[mode]]
        res[f"ms_per_step_{key}"] = round(statistics.median(ms), 2)
        res[f"ms_range_{key}"] = [round(min(ms), 2), round(max(ms), 2)]
    res["deterministic_over_default_time"] = round(res["ms_per_step_deterministic"] / res["ms_per_step_default"], 4)
    for mode, key in ((False, "default"), (True, "deterministic")):
        _, l1, g1 = step(m, batch, mode, a.seed, keep=True)
        _, l2, g2 = step(m, batch, mode, a.seed, keep=True)
        d, where = distance(g1, g2)
        res[f"grad_distance_{key}"], res[f"grad_distance_{key}_at"] = d, where
        whole = lambda g: torch.cat([g[k].double().reshape(-1) for k in g1])
        res[f"whole_grad_distance_{key}"] = float((whole(g1) - whole(g2)).norm() / whole(g1).norm())
        res[f"loss_equal_{key}"] = l1 == l2
        res[f"tensors_bitwise_equal_{key}"] = [sum(bool(torch.equal(g1[k], g2[k])) for k in g1), len(g1)]
    m.eval()
    m._engine.close()
    print(json.dumps(res))
    if res["grad_distance_deterministic"] != 0.0 or not res["loss_equal_deterministic"]:
        sys.exit("the deterministic mode's gradients differ between two identical steps")


if __name__ == "__main__":
    main()
