"""Golden vectors of the engine-resident optimizer step (csrc/train_optim.hip): five steps of torch.optim.AdamW +
torch.nn.utils.clip_grad_norm_ (the installed torch) + the REFERENCE's LitEma (imported through oracle/ref_import.py), on the
forecaster weights of plosses_train_a.npz (unet_simple) and plosses_train_resnet_a.npz (unet.Unet), with seeded gradients.

    python tests/golden/make_optim_golden.py          # writes into tests/golden/ (or $DYF_GOLDEN_OUT)

Two files, each below the 1 MiB limit for a committed file (the four tensor families of 112 k parameters are 1.8 MB together):
    optim_adamw_ema.npz           final weights, EMA buffers (LitEma's names), per-step gradient norms, seeds, hyper-parameters,
                                  and the per-tensor deviation of this fp32 run from a float64 run of the same five steps
    optim_adamw_ema_moments.npz   final exp_avg / exp_avg_sq
Data only.  tests/test_optim_golden_regen.py regenerates both and compares bit for bit.

The gradients of step s are scale_s * randn(shape) drawn tensor by tensor, in `names` order, from torch.Generator(seed_s);
scale_s = target_norm_s / sqrt(number of parameters).  The target norms put BOTH branches of the clip into the run: steps 1-3 have a
global norm above max_norm = 1 (the gradients are scaled down), steps 4-5 below it (coefficient clamped to 1).  The learning rate
changes at step 3 (a scheduler's doing): the step size is an argument of every step, not a constant of the optimizer.
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), "..", ".."))
sys.path.insert(0, ROOT)
OUT = os.environ.get("DYF_GOLDEN_OUT") or os.path.dirname(os.path.abspath(__file__))

HP = dict(betas=[0.9, 0.999], eps=1e-8, weight_decay=1e-4, max_norm=1.0, ema_decay=0.9999,
          lrs=[1e-3, 1e-3, 5e-4, 5e-4, 5e-4],                 # changes at step 3
          target_norms=[4.0, 2.5, 1.5, 0.6, 0.3],             # > max_norm in steps 1-3, < max_norm in steps 4-5
          seeds=[9101, 9102, 9103, 9104, 9105])
NETS = {"simple": "plosses_train_a.npz", "resnet": "plosses_train_resnet_a.npz"}
BUFFER_TAILS = ("running_mean", "running_var", "num_batches_tracked")


def forecaster_parameters(fixture):
    """{name: fp32 tensor} of the forecaster's PARAMETERS (buffers left out), in the fixture's state_dict order."""
    with np.load(os.path.join(ROOT, "tests", "golden", fixture), allow_pickle=False) as z:
        return {k[3:]: torch.from_numpy(z[k].copy()) for k in z.files if k.startswith("F::") and not k.endswith(BUFFER_TAILS)}


def seeded_gradients(shapes, step):
    """The gradients of step `step` (0-based) for {name: shape}: also what the GPU tests import into the engine."""
    g = torch.Generator().manual_seed(HP["seeds"][step])
    n = sum(int(np.prod(s)) for s in shapes.values())
    scale = HP["target_norms"][step] / float(np.sqrt(n))
    return {k: scale * torch.randn(tuple(s), generator=g, dtype=torch.float32) for k, s in shapes.items()}


class _Named(torch.nn.Module):
    """A parameter container whose named_parameters() yields the state_dict names (dots included), which is all LitEma asks of a model."""

    def __init__(self, params, dtype):
        super().__init__()
        self.names = list(params)
        self.ps = torch.nn.ParameterList([torch.nn.Parameter(v.detach().clone().to(dtype)) for v in params.values()])

    def named_parameters(self, *a, **k):
        return iter(zip(self.names, self.ps))


def run(params, dtype, ema_factory):
    """Five steps.  Returns (weights, exp_avg, exp_avg_sq, ema shadow by parameter name, per-step norms)."""
    model = _Named(params, dtype)
    opt = torch.optim.AdamW(list(model.ps), lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"],
                            foreach=False)
    ema = ema_factory(model)
    shapes = {k: tuple(v.shape) for k, v in params.items()}
    norms = []
    for s in range(5):
        for p, g in zip(model.ps, seeded_gradients(shapes, s).values()):
            p.grad = g.to(dtype)
        for grp in opt.param_groups:
            grp["lr"] = HP["lrs"][s]
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(model.ps), HP["max_norm"], foreach=False)))
        opt.step()
        ema(model)
    w = {k: p.detach().clone() for k, p in zip(model.names, model.ps)}
    m = {k: opt.state[p]["exp_avg"].clone() for k, p in zip(model.names, model.ps)}
    v = {k: opt.state[p]["exp_avg_sq"].clone() for k, p in zip(model.names, model.ps)}
    return w, m, v, ema.shadow(model.names), norms


class _RefEma:
    """The reference's LitEma."""

    def __init__(self, model):
        from oracle import ref_import
        ref_import.activate()
        from src.models.modules.ema import LitEma
        self.ema = LitEma(model, decay=HP["ema_decay"])

    def __call__(self, model):
        self.ema(model)

    def shadow(self, names):
        bufs = dict(self.ema.named_buffers())
        return {k: bufs[k.replace(".", "")].detach().clone() for k in names}


class _Ema64:
    """The same rule in float64, for the deviation measurement only: shadow -= (1 - d)(shadow - p) after every step, d the fp32 value
    min(decay, (1 + n) / (10 + n)) of the n-th update."""

    def __init__(self, model):
        self.sh = {k: p.detach().clone() for k, p in model.named_parameters()}
        self.n = 0

    def __call__(self, model):
        self.n += 1
        d = float(min(np.float32(HP["ema_decay"]), np.float32(1 + self.n) / np.float32(10 + self.n)))
        for k, p in model.named_parameters():
            self.sh[k].sub_((1.0 - d) * (self.sh[k] - p.detach()))

    def shadow(self, names):
        return {k: self.sh[k] for k in names}


def main():
    torch.set_num_threads(1)
    main_out, moments = {"hp": np.array(json.dumps(HP))}, {}
    for tag, fixture in NETS.items():
        params = forecaster_parameters(fixture)
        names = list(params)
        w, m, v, sh, norms = run(params, torch.float32, _RefEma)
        w64, m64, v64, sh64, norms64 = run(params, torch.float64, _Ema64)
        main_out[f"{tag}::names"] = np.array(json.dumps(names))
        main_out[f"{tag}::norms"] = np.array(norms, dtype=np.float64)
        for fam, a, b in (("w", w, w64), ("exp_avg", m, m64), ("exp_avg_sq", v, v64), ("ema", sh, sh64)):
            # per tensor: max |fp32 torch run - float64 run|, the yardstick of the GPU parity tests
            main_out[f"{tag}::dev_{fam}"] = np.array([float((a[k].double() - b[k]).abs().max()) for k in names], dtype=np.float64)
        for k in names:
            main_out[f"{tag}::w::{k}"] = w[k].numpy()
            main_out[f"{tag}::ema::{k.replace('.', '')}"] = sh[k].numpy()
            moments[f"{tag}::exp_avg::{k}"] = m[k].numpy()
            moments[f"{tag}::exp_avg_sq::{k}"] = v[k].numpy()
        print(f"{tag}: {len(names)} tensors, {sum(p.numel() for p in params.values())} parameters, norms {[round(x, 4) for x in norms]}")
    os.makedirs(OUT, exist_ok=True)
    np.savez_compressed(os.path.join(OUT, "optim_adamw_ema.npz"), **main_out)
    np.savez_compressed(os.path.join(OUT, "optim_adamw_ema_moments.npz"), **moments)
    for f in ("optim_adamw_ema.npz", "optim_adamw_ema_moments.npz"):
        print(f, os.path.getsize(os.path.join(OUT, f)), "bytes")


if __name__ == "__main__":
    main()
