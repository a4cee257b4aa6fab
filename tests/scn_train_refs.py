"""Reference for the SimpleConvNet training step: a torch restatement of the reference's ConvBlock / SimpleConvNet in TRAIN mode
(src/models/simple_conv_net.py:38-55, 112-131) written out op by op -- Conv2d(k, 'same') -> BatchNorm2d on batch statistics (biased
variance; running statistics updated with momentum 0.1 and the unbiased variance) or on the running statistics -> FiLM
x (scale + 1) + shift from Linear(SiLU(time embedding)) -> exact (erf) GELU -> Dropout with the keep masks PASSED IN -> + block input
where cin == cout -> 1 x 1 head.  It computes in the dtype of the parameters it is given: the GPU tests hand it float64 copies and
differentiate it with torch.autograd.  tests/test_scn_train_refs.py pins it to the imported reference's losses, gradients and
running statistics (tests/golden/scn_*.npz).

Dropout sources (anything with `apply(x, p)`, the interface of oracle.nets.DropoutSeeded, which replays the fixtures' masks):
`MaskList` hands out given keep masks in call order, `EngineMasks` rebuilds the engine generator's masks on the host
(tests/rng_host.py): site i = block i, forward counter as the engine counts its forwards.
"""
import math
from typing import Dict, List, Optional

import torch
import torch.nn.functional as F
from torch import Tensor

from tests import rng_host as R

EPS, MOMENTUM = 1e-5, 0.1


class MaskList:
    """keep masks (NCHW, any dtype) in call order"""

    def __init__(self, masks: List[Tensor]):
        self.masks, self.pos = list(masks), 0

    def apply(self, x: Tensor, p: float) -> Tensor:
        if p <= 0.0:
            return x
        keep = self.masks[self.pos].to(x.dtype)
        self.pos += 1
        assert keep.shape == x.shape, (keep.shape, x.shape)
        return x * keep * (1.0 / (1.0 - p))


class EngineMasks:
    """The engine's own masks: call `begin_forward()` before every network forward that draws (the engine's forward counter)."""

    def __init__(self, seed: int, first_forward: int = 0, record: bool = False):
        self.seed, self.fwd, self.site = seed, first_forward - 1, 0
        self.record, self.masks = record, []

    def begin_forward(self):
        self.fwd += 1
        self.site = 0

    def apply(self, x: Tensor, p: float) -> Tensor:
        if p <= 0.0:
            return x
        b, c, h, w = x.shape
        keep = R.mask_nchw(b, (h, w, c), p, self.seed, self.fwd, self.site)
        self.site += 1
        if self.record:
            self.masks.append(keep)
        return x * keep.to(x.dtype) * (1.0 / (1.0 - p))


def gelu_erf(u: Tensor) -> Tensor:
    return 0.5 * u * (1.0 + torch.erf(u * (1.0 / math.sqrt(2.0))))


def gelu_tanh(u: Tensor) -> Tensor:
    return 0.5 * u * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (u + 0.044715 * u ** 3)))


def time_embedding(P: Dict[str, Tensor], t: Tensor, dim: int) -> Tensor:
    """SinusoidalPosEmb(dim) -> Linear -> GELU -> Linear (simple_conv_net.py:80-85)"""
    dt, dev = P["time_emb_mlp.1.weight"].dtype, P["time_emb_mlp.1.weight"].device
    half = dim // 2
    freqs = torch.exp(torch.arange(half, dtype=dt, device=dev) * (-math.log(10000.0) / (half - 1)))
    ang = t.to(device=dev, dtype=dt)[:, None] * freqs[None, :]
    e = torch.cat([ang.sin(), ang.cos()], dim=-1)
    e = gelu_erf(e @ P["time_emb_mlp.1.weight"].T + P["time_emb_mlp.1.bias"])
    return e @ P["time_emb_mlp.3.weight"].T + P["time_emb_mlp.3.bias"]


def batch_norm(P, pre, x, bn_training: bool, new_stats: Optional[dict]):
    g, b = P[f"{pre}.weight"][None, :, None, None], P[f"{pre}.bias"][None, :, None, None]
    if bn_training:
        mean = x.mean(dim=(0, 2, 3))
        var = ((x - mean[None, :, None, None]) ** 2).mean(dim=(0, 2, 3))
        if new_stats is not None:
            n = x.numel() // x.shape[1]
            with torch.no_grad():
                rm = new_stats.get(f"{pre}.running_mean", P[f"{pre}.running_mean"])
                rv = new_stats.get(f"{pre}.running_var", P[f"{pre}.running_var"])
                new_stats[f"{pre}.running_mean"] = (1 - MOMENTUM) * rm + MOMENTUM * mean.detach()
                new_stats[f"{pre}.running_var"] = (1 - MOMENTUM) * rv + MOMENTUM * var.detach() * (n / max(n - 1, 1))
    else:
        mean, var = P[f"{pre}.running_mean"], P[f"{pre}.running_var"]
    return (x - mean[None, :, None, None]) / torch.sqrt(var[None, :, None, None] + EPS) * g + b


def block(P, i: int, x: Tensor, temb: Optional[Tensor], k: int, p: float, dropout, bn_training: bool, new_stats=None,
          gelu=gelu_erf, residual: bool = True, drop_tap=None) -> Tensor:
    """ConvBlock.forward.  drop_tap = (ky, kx): that tap of the conv weight is zeroed (a deliberately wrong network, for the
    sensitivity checks of the tolerance)."""
    pre = f"convs.{i}"
    w = P[f"{pre}.conv.weight"]
    if drop_tap is not None:
        m = torch.ones_like(w)
        m[:, :, drop_tap[0], drop_tap[1]] = 0
        w = w * m
    res = x
    x = F.conv2d(x, w, P[f"{pre}.conv.bias"], padding=(k - 1) // 2)
    x = batch_norm(P, f"{pre}.norm", x, bn_training, new_stats)
    if temb is not None:
        ss = F.silu(temb) @ P[f"{pre}.time_mlp.1.weight"].T + P[f"{pre}.time_mlp.1.bias"]
        scale, shift = ss[:, :, None, None].chunk(2, dim=1)
        x = x * (scale + 1) + shift
    x = gelu(x)
    if dropout is not None:
        x = dropout.apply(x, p)
    if residual and w.shape[0] == w.shape[1]:
        x = x + res
    return x


def forward(P: Dict[str, Tensor], cfg: dict, inputs: Tensor, time: Optional[Tensor] = None, condition: Optional[Tensor] = None,
            dropout=None, bn_training: bool = False, new_stats: Optional[dict] = None, gelu=gelu_erf, residual: bool = True,
            drop_tap=None) -> Tensor:
    """SimpleConvNet.forward.  cfg: dim, kernel_sizes, with_time_emb, dropout.  `new_stats` (a dict) receives / carries the running
    statistics as the train-mode forwards update them (two forecaster passes of one step -> two updates).  drop_tap: (block, ky, kx)."""
    dt = P["head.weight"].dtype
    x = inputs.to(dt) if condition is None else torch.cat([inputs.to(dt), condition.to(dt)], dim=1)
    temb = time_embedding(P, time, cfg["dim"]) if cfg.get("with_time_emb", False) else None
    for i, k in enumerate(cfg["kernel_sizes"]):
        tap = drop_tap[1:] if drop_tap is not None and drop_tap[0] == i else None
        x = block(P, i, x, temb, k, cfg.get("dropout", 0.0), dropout, bn_training, new_stats, gelu, residual, tap)
    return F.conv2d(x, P["head.weight"], P["head.bias"])


def to_dtype(P: Dict[str, Tensor], dtype, requires_grad: bool = False, device=None) -> Dict[str, Tensor]:
    """A copy of the floating-point tensors in `dtype`; with requires_grad the parameters (not the running statistics) are leaves."""
    out = {}
    for k, v in P.items():
        if not v.is_floating_point():
            out[k] = v
            continue
        v = v.detach().to(dtype=dtype, device=device).clone()
        if requires_grad and not k.endswith(("running_mean", "running_var")):
            v.requires_grad_(True)
        out[k] = v
    return out


def grad_errors(got: Dict[str, Tensor], want: Dict[str, Tensor]):
    """Every tensor's ||got - want|| over the GLOBAL norm of `want` (tests/test_gpu_training.py's measure): under batch statistics
    d loss / d conv.bias is exactly zero and the reference leaves ~3e-9 of the gradient norm there, so a per-tensor relative
    measure would compare noise.  Returns (worst, its name, the global norm)."""
    assert sorted(got) == sorted(want), (sorted(set(got) ^ set(want)))
    gn = float(torch.cat([g.double().reshape(-1) for g in want.values()]).norm())
    errs = {k: float((got[k].detach().cpu().double() - want[k].detach().cpu().double()).norm()) / gn for k in want}
    worst = max(errs, key=errs.get)
    return errs[worst], worst, gn


# ---------------------------------------------------------------------------------------------- whole steps under torch.autograd
def _collect(Pg):
    return {k: v.grad for k, v in Pg.items() if torch.is_tensor(v) and v.requires_grad}


def plosses_step(PF, PI, hp, xt_last, cond, t, sc, drop, begin_forward=None, dtype=torch.float64, **variant):
    """DYffusion.p_losses in train mode + backward (oracle.losses.p_losses, pinned to the reference, over this file's network):
    forecaster on batch statistics, frozen interpolator on its running statistics, both with dropout from `drop`.
    `begin_forward()` runs before every network forward.  Returns (losses, forecaster gradients, running statistics after)."""
    from oracle import losses
    mk = hp["model"]
    PFg, PIc, stats = to_dtype(PF, dtype, True), to_dtype(PI, dtype), {}

    def f_fn(x, tt, c):
        if begin_forward:
            begin_forward()
        return forward(PFg, mk, x, tt, c, dropout=drop, bn_training=True, new_stats=stats, **variant)

    def i_fn(x, tt, c):
        if begin_forward:
            begin_forward()
        return forward(PIc, mk, x, tt, c, dropout=drop, bn_training=False)

    out = losses.p_losses(f_fn, i_fn, xt_last.to(dtype), cond.to(dtype), t, None if sc is None else sc.to(dtype), hp)
    out["loss"].backward()
    return {k: float(out[k].detach()) for k in ("loss", "loss_forward", "loss_forward2")}, _collect(PFg), stats


def interp_step(P, hp, dynamics, cond, t, drop, dtype=torch.float64, **variant):
    """InterpolationExperiment.get_loss in train mode + backward (oracle.losses.interpolation_loss)."""
    from oracle import losses
    Pg, stats = to_dtype(P, dtype, True), {}
    loss = losses.interpolation_loss(lambda x, tt, c: forward(Pg, hp["model"], x, tt, c, dropout=drop, bn_training=True, new_stats=stats, **variant),
                                     dynamics.to(dtype), t, cond.to(dtype), hp["window"], hp["loss_function"])
    loss.backward()
    return {"loss": float(loss.detach())}, _collect(Pg), stats


def get_loss_step(P, hp, x, c, y, drop, dtype=torch.float64, **variant):
    """BaseModel.get_loss in train mode + backward (_base_model.py:108-138)."""
    from oracle import losses
    Pg, stats = to_dtype(P, dtype, True), {}
    pred = forward(Pg, hp["model"], x, None, c, dropout=drop, bn_training=True, new_stats=stats, **variant)
    loss = losses.criterion_fn(hp["loss_function"])(pred, y.to(dtype))
    loss.backward()
    return {"loss": float(loss.detach())}, _collect(Pg), stats


def fixture_step(name, z, drop, begin_forward=None, dtype=torch.float64, **variant):
    """The step a tests/golden/scn_*.npz fixture records, by its name."""
    import json
    from tests.helpers import split_state
    hp = json.loads(str(z["hp"]))
    T = lambda k: torch.from_numpy(z[k])
    PF = split_state(z, "F")
    if name.startswith("scn_plosses"):
        return plosses_step(PF, split_state(z, "I"), hp, T("xt_last"), T("cond"), T("t"), T("sc"), drop, begin_forward, dtype, **variant)
    if begin_forward:
        begin_forward()
    if name.startswith("scn_interp"):
        return interp_step(PF, hp, T("dynamics"), T("cond"), T("t"), drop, dtype, **variant)
    return get_loss_step(PF, hp, T("x"), T("c"), T("y"), drop, dtype, **variant)
