#!/usr/bin/env python
"""What does 16-bit storage cost a rollout?  Builds a 16-bit engine and an fp32 engine (`dtype="fp32"`, dyf_set_sample_precision(32))
from the same weights and seed, runs the same rollout on both -- same inputs, same dropout masks, same noise streams -- and prints
ONE JSON line: the per-horizon rel-RMS of the 16-bit fields against the fp32 fields and the time of both rollouts.

    python tools/precision_drift.py --config ns    --dtype bf16 [--rows 8]     # NS benchmark: 221x42, dim 64 @ 256^2, h = 16
    python tools/precision_drift.py --config oisst --dtype fp16 [--rows 8]     # OISST: 60x60, unet.Unet, T = 32, data+noise
    python tools/precision_drift.py --config synth512 --dtype fp16 --rows 4    # 512x512x4, unet.Unet, h = 32: 16 384 bottleneck tokens
    python tools/precision_drift.py --small                                    # the 23x11 test pair (dim 64 @ 64^2, h = 4)
    python tools/precision_drift.py --config oisst --dtype fp16 --attention-dropout exact   # the 16-bit engine in its exact
                                                # attention-dropout mode: the fp32 engine's keep bits at EVERY site, rounding alone is left
    python tools/precision_drift.py --config ns --dtype bf16x3 [--rows 8]      # the bf16x3 sampling mode (dyf_set_sample_precision(48))
                                                # against fp32: the same keep bits at every site, the conv operands alone differ
    python tools/precision_drift.py --config ns --dtype bf16x3 --halo-ab 3     # and the forms of its 3 x 3 halo convs against each other
                                                # (DYF_SAMPLE_HALO_FUSED = 1 fused, 0 the two-launch PASS form): one engine and one captured
                                                # graph per form, replayed in turn, 3 rounds -> "halo_ab" {form: [seconds, ...]}

Needs an MI355X.  Imports neither the oracle nor the reference: the fp32 engine is the yardstick.
"""
import argparse
import json
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import dyffusion_amd as D  # noqa: E402


def random_state(net, seed, conv_gain=1.0):
    """Random weights with O(1) activations (no checkpoints offline), the initialiser of the benchmark."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in net.state_dict().items():
        shp = tuple(v.shape)
        if k.endswith("num_batches_tracked"):
            sd[k] = torch.zeros((), dtype=torch.int64)
        elif k.endswith("running_var"):
            sd[k] = 0.5 + torch.rand(shp, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = 0.1 * torch.randn(shp, generator=g)
        elif k.endswith(".norm.g"):
            sd[k] = torch.ones(shp)
        elif len(shp) == 1:
            sd[k] = (1.0 if k.endswith("weight") else 0.0) + 0.05 * torch.randn(shp, generator=g)
        else:
            fan_in = shp[0] * 4 if k.startswith("readout") else math.prod(shp[1:])
            sd[k] = torch.randn(shp, generator=g) * ((0.7 if "time_mlp" in k else 1.4) / math.sqrt(fan_in))
            if len(shp) == 4:
                sd[k] = sd[k] * conv_gain
    return sd


def make(config, dtype, rows, attn_dropout=True, attn_mode="fast"):
    """(DYffusion, initial condition, static condition or None) of `config` on an engine of `dtype`; same weights for every dtype.
    attn_mode: DYffusion(attention_dropout=...) -- how the 16-bit engine draws the dropout of unet.Unet's Attention probabilities."""
    g = torch.Generator().manual_seed(3)
    if config in ("ns", "small"):
        hw, up, h = ((221, 42), [256, 256], 16) if config == "ns" else ((23, 11), [64, 64], 4)
        kw = dict(dim=64, with_time_emb=True, outer_sample_mode="bilinear", upsample_dims=up, dropout=0.15)
        F = D.UNet(num_input_channels=3, num_output_channels=3, num_conditional_channels=2, spatial_shape=hw, **kw)
        I = D.UNet(num_input_channels=6, num_output_channels=3, num_conditional_channels=2, spatial_shape=hw, **kw)
        F.load_state_dict(random_state(F, 0))
        I.load_state_dict(random_state(I, 1))
        m = D.DYffusion(F, D.InterpolatorHandle(I, h), timesteps=h, forward_conditioning="none", interpolate_before_t1=True,
                        schedule="before_t1_only", sampling_type="cold", refine_intermediate_predictions=True,
                        enable_interpolator_dropout=True, max_batch=rows, dtype=dtype)
        x0, c = torch.randn(rows, 3, *hw, generator=g), torch.rand(rows, 2, *hw, generator=g)
    elif config == "synth512":  # the shapes of bench.py's config4_synth512 (fp32: the streaming Attention core, 16 384 tokens)
        kw = dict(dim=64, dim_mults=(1, 2, 4), with_time_emb=True)
        I = D.Unet(num_input_channels=8, num_output_channels=4, block_dropout=0.1, attn_dropout=0.1 if attn_dropout else 0.0, **kw)
        F = D.Unet(num_input_channels=4, num_output_channels=4, **kw)
        # conv gains halved: the h = 32 recursion of a random-init pair must stay inside fp16's range
        F.load_state_dict(random_state(F, 0, 0.5))
        I.load_state_dict(random_state(I, 1, 0.5))
        m = D.DYffusion(F, D.InterpolatorHandle(I, 32), timesteps=32, forward_conditioning="none", interpolate_before_t1=True,
                        refine_intermediate_predictions=False, enable_interpolator_dropout=True, max_batch=rows, dtype=dtype,
                        allow_bf16_long_rollout=True, attention_dropout=attn_mode)
        x0, c = torch.randn(rows, 4, 512, 512, generator=g), None
    else:
        kw = dict(dim=64, dim_mults=(1, 2, 4), with_time_emb=True)
        # attn_dropout also covers the one site whose keep bits differ between the precisions in the 16-bit engine's default mode (the
        # attention probabilities: the quad form's own stream and k/256 granularity, nn.Dropout's p in fp32); --no-attention-dropout, or
        # --attention-dropout exact with the site left on, leaves rounding as the only difference
        F = D.Unet(num_input_channels=1, num_output_channels=1, num_conditional_channels=1, block_dropout=0.3,
                   attn_dropout=0.1 if attn_dropout else 0.0, **kw)
        I = D.Unet(num_input_channels=2, num_output_channels=1, num_conditional_channels=0, block_dropout=0.6, block_dropout1=0.2,
                   attn_dropout=0.6 if attn_dropout else 0.0, **kw)
        F.load_state_dict(random_state(F, 0, 0.5))
        I.load_state_dict(random_state(I, 1, 0.5))
        m = D.DYffusion(F, D.InterpolatorHandle(I, 7), timesteps=7, forward_conditioning="data+noise", interpolate_before_t1=True,
                        additional_interpolation_steps=25, refine_intermediate_predictions=False, max_batch=rows, dtype=dtype,
                        allow_bf16_long_rollout=True, attention_dropout=attn_mode)
        x0, c = torch.randn(rows, 1, 60, 60, generator=g), None
    return m, x0.cuda(), None if c is None else c.cuda()


def rollout(m, x0, c, seed, reps):
    """Fields of the first rollout after seeding (the one both engines are compared on) and the best time of `reps` later ones."""
    kw = {} if c is None else dict(static_condition=c)
    m.seed(seed)
    out = {k: v.clone() for k, v in m.sample(x0, **kw).items()}
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(reps):
        t0 = time.perf_counter()
        m.sample(x0, **kw)
        torch.cuda.synchronize()
        best = min(best, time.perf_counter() - t0)
    return out, best


def halo_ab(config, a, forms):
    """Seconds per rollout of a bf16x3 engine under each value of DYF_SAMPLE_HALO_FUSED: the switch is read when a conv is launched, so
    every form gets an engine of its own that captures its rollout under it; the captured graphs are then replayed in turn."""
    from dyffusion_amd import _lib
    engines = {}
    for form in forms:
        _lib.set_form("DYF_SAMPLE_HALO_FUSED", form)
        m, x0, c = make(config, "bf16x3", a.rows, not a.no_attention_dropout, a.attention_dropout)
        rollout(m, x0, c, a.seed, 1)  # capture + one replay
        engines[form] = (m, x0, c)
    _lib.set_form("DYF_SAMPLE_HALO_FUSED", None)
    times = {form: [] for form in forms}
    for _ in range(a.halo_ab):
        for form in forms:
            m, x0, c = engines[form]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            m.sample(x0, **({} if c is None else dict(static_condition=c)))
            torch.cuda.synchronize()
            times[form].append(time.perf_counter() - t0)
    for m, _, _ in engines.values():
        m._engine.close()
    return times


def rel_rms(a, b):
    return float(((a - b).double().pow(2).mean() / b.double().pow(2).mean()).sqrt())


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--config", choices=["ns", "oisst", "synth512"], default="ns")
    ap.add_argument("--small", action="store_true", help="the 23x11 test pair instead of --config")
    ap.add_argument("--dtype", choices=["bf16", "fp16", "bf16x3"], default="bf16",
                    help="the engine compared with fp32: 16-bit storage, or bf16x3 (fp32 forward, hi / lo bf16 conv operands)")
    ap.add_argument("--halo-ab", type=int, default=0, metavar="ROUNDS",
                    help="--dtype bf16x3: time the halo-conv forms against each other, ROUNDS rollouts each, alternating")
    ap.add_argument("--halo-forms", default="1,0", help="values of DYF_SAMPLE_HALO_FUSED --halo-ab compares (1 fused, 0 PASS)")
    ap.add_argument("--rows", type=int, default=8, help="batch rows (ensemble members x batch) of the rollout")
    ap.add_argument("--no-attention-dropout", action="store_true", help="oisst / synth512: attn_dropout = 0 in both networks")
    ap.add_argument("--attention-dropout", choices=["fast", "exact"], default="fast",
                    help="oisst / synth512: attention-dropout mode of the 16-bit engine (exact: the fp32 engine's keep bits)")
    ap.add_argument("--seed", type=int, default=7)
    ap.add_argument("--reps", type=int, default=2, help="timed rollouts per engine (the best counts)")
    a = ap.parse_args()
    config = "small" if a.small else a.config
    res = dict(config=config, dtype=a.dtype, rows=a.rows, seed=a.seed, attention_dropout=not a.no_attention_dropout,
               attention_dropout_mode=a.attention_dropout)
    fields, times = {}, {}
    for dtype in ("fp32", a.dtype):  # one engine at a time: the fp32 arena of a full-size pair is several GB
        m, x0, c = make(config, dtype, a.rows, not a.no_attention_dropout, a.attention_dropout)
        fields[dtype], times[dtype] = rollout(m, x0, c, a.seed, a.reps)
        fields[dtype] = {k: v.cpu() for k, v in fields[dtype].items()}
        nf, ni = m._engine.forward_counts()
        m._engine.close()
        del m
    keys = sorted(fields["fp32"], key=lambda k: int(k[1:].split("_")[0]))
    res["forwards"] = [nf, ni]
    res["rel_rms"] = {k: rel_rms(fields[a.dtype][k], fields["fp32"][k]) for k in keys}
    res["worst_rel_rms"] = max(res["rel_rms"].values())
    res["seconds_16bit"], res["seconds_fp32"] = times[a.dtype], times["fp32"]
    res["fp32_over_16bit_time"] = times["fp32"] / times[a.dtype]
    if a.halo_ab > 0 and a.dtype == "bf16x3":
        res["halo_ab"] = halo_ab(config, a, [f.strip() for f in a.halo_forms.split(",")])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
