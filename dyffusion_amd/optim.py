"""Engine-resident optimizer: AdamW + global gradient-norm clipping + weight EMA on the engine's own training copy.

What the reference's training loop does with `torch.optim.AdamW`, Lightning's `gradient_clip_val` (clip_grad_norm_) and `LitEma`
(src/models/modules/ema.py; _base_experiment.py:100-107, 263-270, 459-461, 715-735), without the gradients, the optimizer state or
the weights leaving the GPU: `loss.backward()` leaves the parameter gradients in the engine, `step()` is two kernel launches
(csrc/train_optim.hip), and the torch module is brought up to date only when something reads it (`pull()`).  A step waits for
nothing it launches; what it does wait for is the PREVIOUS step's outcome (skipped or not: the step count of the bias corrections
and of the EMA warm-up depends on it), which was copied to the host a whole forward and backward earlier -- in a loop that never
synchronises otherwise, the host runs at most one step ahead of the GPU.

    model.train()
    opt = EngineAdamW(model, lr=3e-4, weight_decay=1e-4, max_grad_norm=1.0, ema_decay=0.9999)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, ...)          # param_groups[0]["lr"] is read at every step
    for batch in loader:
        model.p_losses(...)["loss"].backward()                   # gradients accumulate in the engine
        opt.step(); sched.step()
    with opt.ema_scope():
        model.sample(...)                                        # through the EMA weights
"""
import math
from contextlib import contextmanager
from typing import Dict, Optional

import numpy as np
import torch

from . import _lib as L
from .engine import mark_weights_modified, state_version, sync_train_weights


def _torch_adamw_defaults(lr, betas, eps, weight_decay) -> dict:
    """The `defaults` of the installed torch.optim.AdamW for these values: param_groups then carry exactly torch's keys."""
    return dict(torch.optim.AdamW([torch.nn.Parameter(torch.zeros(1))], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                                  foreach=False).defaults)


def ema_decay_at(decay: float, num_updates: int) -> float:
    """The decay LitEma applies at its `num_updates`-th update (counted from 1): the configured decay, warmed up as
    (1 + n) / (10 + n), evaluated in fp32 as a tensor expression would be."""
    warm = np.float32(1 + num_updates) / np.float32(10 + num_updates)
    return float(min(np.float32(decay), warm))


class EngineAdamW(torch.optim.Optimizer):
    """AdamW whose state and arithmetic live in the HIP engine.  `owner`: a `DYffusion` in training mode (its forecaster -- any of the
    three backbones -- is trained, the interpolator stays frozen) or a `UNet` / `Unet` trained through its own `get_loss` (stage 1; a
    stand-alone `SimpleConvNet` is refused: its stage 1 trains through `param.grad` and torch.optim).

    While attached, `loss.backward()` leaves the gradients in the engine, where they accumulate until `step()`; `param.grad` stays
    None.  After a step the torch module is stale until `pull()`, which runs by itself before anything reads the module (sampling,
    prediction, eval-mode losses, `state_dict()`).  Editing the module's parameters while engine steps are pending is an error.
    One parameter group, no AMSGrad.  `detach()` returns the network to the classic `param.grad` path."""

    def __init__(self, owner, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2,
                 max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None):
        from .simple_conv_net import SimpleConvNet
        net = getattr(owner, "model", owner) if hasattr(owner, "p_losses") else owner
        if isinstance(owner, SimpleConvNet):  # (as a DYffusion's forecaster it is trained resident like the other backbones)
            raise NotImplementedError("EngineAdamW: a stand-alone SimpleConvNet (stage 1) trains through param.grad and torch.optim; "
                                      "the engine-resident optimizer serves it as the forecaster of a DYffusion")
        if not (isinstance(net, torch.nn.Module) and hasattr(net, "engine_net_config") and hasattr(net, "_train_backward")):
            raise TypeError(f"EngineAdamW: owner must be a DYffusion, a UNet or a Unet, got {type(owner).__name__}")
        if not lr >= 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if not eps >= 0.0:
            raise ValueError(f"Invalid epsilon value: {eps}")
        if len(betas) != 2 or not 0.0 <= betas[0] < 1.0 or not 0.0 <= betas[1] < 1.0:
            raise ValueError(f"Invalid beta parameters: {betas}")
        if not weight_decay >= 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if ema_decay is not None and not 0.0 <= ema_decay <= 1.0:
            raise ValueError("Decay must be between 0 and 1")
        if resident := net.__dict__.get("_engine_optim"):
            raise RuntimeError(f"the network already has an engine-resident optimizer ({resident!r}): detach() it first")
        self.owner, self._net = owner, net
        self._names = [k for k, _ in net.named_parameters()]
        self.max_grad_norm = None if max_grad_norm is None or max_grad_norm <= 0 else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self._ema_base = 0          # EMA updates minus applied optimizer steps (a skipped step updates neither)
        super().__init__(list(net.parameters()), _torch_adamw_defaults(lr, tuple(betas), eps, weight_decay))
        self._eng = None            # the engine the resident state lives in (bound at the first backward / step)
        self._slot = None
        self._stale = False         # the engine is ahead of the torch module
        self._stale_version = None  # state_version(net) when it fell behind: a different value later = edited by hand
        self._pending_bn = 0        # training forwards whose BatchNorm bookkeeping (num_batches_tracked) the module has not seen
        self._host = None           # state waiting for an engine: {"state": {name: {...}}, "step": int, "ema": {name: tensor} | None}
        self._in_ema_scope = False
        net.__dict__["_engine_optim"] = self

    # ------------------------------------------------------------------ engine binding
    def _shapes(self) -> Dict[str, tuple]:
        return {k: tuple(p.shape) for k, p in self._net.named_parameters()}

    def _device(self):
        p = next(self._net.parameters())
        return p.device if (p.is_cuda and self._eng is not None and p.device.index == self._eng.device) else None

    def _bind(self, eng, slot: int):
        if self._eng is eng:
            return
        if self._eng is not None:
            self.release_engine(self._eng)
        g = self.param_groups[0]
        eng.optim_create(slot, beta1=g["betas"][0], beta2=g["betas"][1], eps=g["eps"], weight_decay=g["weight_decay"],
                         max_grad_norm=self.max_grad_norm or 0.0, ema=self.ema_decay is not None)
        self._eng, self._slot = eng, slot
        eng._before_close.append(self.release_engine)
        if self._host is not None:
            host, self._host = self._host, None
            if host["state"]:
                eng.optim_import(slot, L.OPTIM_EXP_AVG, {k: v["exp_avg"] for k, v in host["state"].items()})
                eng.optim_import(slot, L.OPTIM_EXP_AVG_SQ, {k: v["exp_avg_sq"] for k, v in host["state"].items()})
            eng.optim_set_step(slot, host["step"])
            if host.get("ema") and self.ema_decay is not None:
                eng.optim_import(slot, L.OPTIM_EMA, host["ema"])
            if host.get("grad") and any(bool(g.any()) for g in host["grad"].values()):
                # gradients accumulated in the engine this state was released from and not yet stepped on: added to whatever a
                # backward has already left in this one
                here = eng.optim_export(slot, L.OPTIM_GRAD, self._shapes())
                eng.optim_import(slot, L.OPTIM_GRAD, {k: here[k] + g for k, g in host["grad"].items()})

    def release_engine(self, eng):
        """The engine goes away (closed, or replaced for a larger batch / another grid): module and state move to the host side."""
        if self._eng is not eng:
            return
        self.pull()
        self._host = self._export_host()
        self._host["grad"] = eng.optim_export(self._slot, L.OPTIM_GRAD, self._shapes())  # a backward without its step yet: carried over
        if self.release_engine in eng._before_close:
            eng._before_close.remove(self.release_engine)
        eng.optim_destroy(self._slot)
        self._eng = self._slot = None

    def _export_host(self):
        shapes, eng, slot = self._shapes(), self._eng, self._slot
        m, v = eng.optim_export(slot, L.OPTIM_EXP_AVG, shapes), eng.optim_export(slot, L.OPTIM_EXP_AVG_SQ, shapes)
        ema = eng.optim_export(slot, L.OPTIM_EMA, shapes) if self.ema_decay is not None else None
        return dict(state={k: dict(exp_avg=m[k], exp_avg_sq=v[k]) for k in shapes}, step=eng.optim_get_step(slot), ema=ema)

    def _require_engine(self):
        if self._eng is None:
            eng, slot = getattr(self._net, "_engine", None), getattr(self._net, "_engine_slot", None)
            if eng is None:
                raise RuntimeError("EngineAdamW: the network has no engine yet -- run a training forward (p_losses / get_loss) first")
            self._bind(eng, slot)
        if not self._stale:  # weights the module was given since (torch.optim steps, load_state_dict): the engine's copy follows
            sync_train_weights(self._net, self._eng, self._slot)
        return self._eng

    def detach(self):
        """Bring the module up to date, drop the resident state and return the network to the classic `param.grad` path."""
        if self._eng is not None:
            self.release_engine(self._eng)
        self._net.__dict__.pop("_engine_optim", None)

    # ------------------------------------------------------------------ hooks of engine.py (collect_train_results, sync_*)
    def after_backward(self, eng, slot: int, n_forwards: int):
        """dyf_train_backward has accumulated this step's gradients into the engine's arena: they stay there."""
        self._bind(eng, slot)
        self._pending_bn += int(n_forwards)
        self._mark_stale()

    def engine_is_ahead(self, eng) -> bool:
        """True while the engine's training copy holds state the module has not pulled; raises if the module was edited meanwhile."""
        if not self._stale or self._eng is not eng:
            return False
        self._check_untouched()
        return True

    def _mark_stale(self):
        if not self._stale:
            self._stale, self._stale_version = True, state_version(self._net)

    def _check_untouched(self):
        if state_version(self._net) != self._stale_version:
            raise RuntimeError("the module's parameters were modified while engine-resident optimizer steps are pending: the "
                               "engine holds the current weights.  Call optimizer.pull() before editing the module (or "
                               "optimizer.detach() to return to torch.optim)")

    # ------------------------------------------------------------------ torch.optim surface
    def add_param_group(self, param_group):
        if getattr(self, "_names", None) is not None and self.param_groups:
            raise NotImplementedError("EngineAdamW has one parameter group: all parameters of the network it was built over")
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none: bool = True):
        """Clears the engine's gradient arena (`step()` already leaves it cleared: this exists for loop compatibility)."""
        if self._eng is not None:
            self._eng.train_zero_grads(self._slot)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        eng = self._require_engine()
        if eng.comm_world > 1:
            raise NotImplementedError("EngineAdamW.step(): the all-reduce of engine-resident gradients over a communicator of "
                                      f"{eng.comm_world} ranks is not implemented; use torch.optim with distributed.all_reduce_gradients")
        if self._in_ema_scope:
            raise RuntimeError("EngineAdamW.step() inside ema_scope(): the engine holds the EMA weights")
        if self._stale:
            self._check_untouched()
        decay_now = 0.0
        if self.ema_decay is not None:
            # LitEma counts its updates; a step the engine skipped (non-finite gradients) updated nothing and is not counted.  Reading
            # the count waits for the PREVIOUS step's outcome only, which was copied out a whole forward and backward ago.
            decay_now = ema_decay_at(self.ema_decay, self._ema_base + eng.optim_get_step(self._slot) + 1)
        eng.optim_step(self._slot, float(self.param_groups[0]["lr"]), decay_now)
        self._mark_stale()
        return loss

    @property
    def last_grad_norm(self) -> float:
        """Global gradient norm (before clipping) of the most recent step; synchronises with that step when read."""
        return self._require_engine().optim_last(self._slot)[0]

    @property
    def last_step_skipped(self) -> bool:
        """The most recent step met a non-finite gradient norm and changed nothing; synchronises when read."""
        skipped = self._require_engine().optim_last(self._slot)[1]
        return skipped

    @property
    def ema_num_updates(self) -> int:
        """LitEma's `num_updates`: EMA updates applied so far."""
        return self._ema_base + self.step_count

    @property
    def step_count(self) -> int:
        return self._host["step"] if self._eng is None and self._host is not None else 0 if self._eng is None else self._eng.optim_get_step(self._slot)

    _KINDS = {"weight": L.OPTIM_WEIGHT, "grad": L.OPTIM_GRAD, "exp_avg": L.OPTIM_EXP_AVG, "exp_avg_sq": L.OPTIM_EXP_AVG_SQ, "ema": L.OPTIM_EMA,
              "weight_fwd": L.OPTIM_WEIGHT_FWD}

    def export(self, kind: str, device=None) -> Dict[str, torch.Tensor]:
        """The engine's tensors of `kind` ("weight" | "grad" | "exp_avg" | "exp_avg_sq" | "ema") by parameter name, PyTorch layouts,
        on the CPU or on `device` (the engine's GPU).  "weight_fwd": the 4-d (conv) weights read from the engine's second,
        forward-layout copy; "stats": the BatchNorm running statistics."""
        eng = self._require_engine()
        if kind == "stats":
            bufs = {k: tuple(b.shape) for k, b in self._net.named_buffers() if k.endswith(("running_mean", "running_var"))}
            return eng.optim_export(self._slot, L.OPTIM_WEIGHT, bufs, device=device)
        shapes = self._shapes()
        if kind == "weight_fwd":
            shapes = {k: s for k, s in shapes.items() if len(s) == 4 and not k.endswith(".norm.g")}
        return eng.optim_export(self._slot, self._KINDS[kind], shapes, device=device)

    def import_gradients(self, grads: Dict[str, torch.Tensor]):
        """Replace the engine's gradients of the named parameters (an external gradient exchange; tests)."""
        shapes = self._shapes()
        for k, g in grads.items():
            if tuple(g.shape) != shapes[k]:
                raise ValueError(f"gradient of {k}: shape {tuple(g.shape)}, expected {shapes[k]}")
        self._require_engine().optim_import(self._slot, L.OPTIM_GRAD, grads)

    # ------------------------------------------------------------------ module <- engine
    @torch.no_grad()
    def pull(self):
        """Weights, BatchNorm running statistics and num_batches_tracked from the engine into the torch module (device-to-device
        when the module lives on the engine's GPU).  The module's training-copy mark is set, so no re-upload of what just came
        from there follows; its sampling-copy mark is left behind, so the next sampling call refreshes the packed weights."""
        if not self._stale or self._eng is None:
            return
        self._check_untouched()
        self._stale = False  # (first: the module's state_dict() hook calls pull())
        eng, slot, net, dev = self._eng, self._slot, self._net, self._device()
        params = dict(net.named_parameters())
        bufs = {k: b for k, b in net.named_buffers() if k.endswith(("running_mean", "running_var"))}
        shapes = {k: tuple(t.shape) for k, t in list(params.items()) + list(bufs.items())}
        for k, v in eng.optim_export(slot, L.OPTIM_WEIGHT, shapes, device=dev).items():
            (params.get(k) if k in params else bufs[k]).copy_(v)
        if self._pending_bn:
            for k, b in net.named_buffers():
                if k.endswith("num_batches_tracked"):
                    b += self._pending_bn
            self._pending_bn = 0
        net.__dict__.pop("_version_tensors", None)
        net._train_version = (id(eng), state_version(net))

    # ------------------------------------------------------------------ EMA
    @contextmanager
    def ema_scope(self):
        """Everything inside runs on the EMA weights (the reference validates through them): the engine swaps weights and shadow in
        place, sampling sees the shadow; on exit they are swapped back bitwise."""
        if self.ema_decay is None:
            raise RuntimeError("ema_scope(): the optimizer was built without ema_decay")
        eng = self._require_engine()
        self._swap(eng)
        self._in_ema_scope = True
        try:
            yield self
        finally:
            self._in_ema_scope = False
            self._swap(eng)

    def _swap(self, eng):
        if self._stale:
            self._check_untouched()
        eng.optim_swap_ema(self._slot)
        self._stale = False   # whatever the module held, the engine's training copy now differs from it:
        self._mark_stale()    # the next reader pulls, and the version marks then refresh the sampling copy
        mark_weights_modified(self._net)
        self._stale_version = state_version(self._net)

    def ema_state_dict(self) -> Dict[str, torch.Tensor]:
        """The shadow under LitEma's buffer names (parameter name without the dots), plus `decay` and `num_updates`."""
        if self.ema_decay is None:
            raise RuntimeError("ema_state_dict(): the optimizer was built without ema_decay")
        if self._in_ema_scope:
            raise RuntimeError("ema_state_dict() inside ema_scope(): weights and shadow are swapped")
        if self._eng is not None:
            shadow = self._eng.optim_export(self._slot, L.OPTIM_EMA, self._shapes(), device=self._device())
        elif self._host is not None and self._host.get("ema"):
            shadow = self._host["ema"]
        else:
            shadow = {k: p.detach().clone() for k, p in self._net.named_parameters()}
        out = {"decay": torch.tensor(self.ema_decay, dtype=torch.float32), "num_updates": torch.tensor(self.ema_num_updates, dtype=torch.int)}
        out.update({k.replace(".", ""): v for k, v in shadow.items()})
        return out

    def load_ema_state_dict(self, sd: Dict[str, torch.Tensor]):
        shadow = {k: sd[k.replace(".", "")].detach().to(torch.float32) for k in self._names}
        for k, shape in self._shapes().items():
            if tuple(shadow[k].shape) != shape:
                raise ValueError(f"EMA tensor {k}: shape {tuple(shadow[k].shape)}, expected {shape}")
        if "num_updates" in sd:
            self._ema_base = max(0, int(sd["num_updates"])) - self.step_count
        if self._eng is not None:
            self._eng.optim_import(self._slot, L.OPTIM_EMA, shadow)
        else:
            self._host = self._host or dict(state={}, step=0, ema=None)
            self._host["ema"] = shadow

    # ------------------------------------------------------------------ state in torch.optim.AdamW's format
    def state_dict(self) -> dict:
        """`torch.optim.AdamW.state_dict()`'s layout: state[i] = {step, exp_avg, exp_avg_sq} in named_parameters() order (empty
        before the first step, as torch's) and param_groups with parameter indices."""
        groups = [{**{k: v for k, v in g.items() if k != "params"}, "params": list(range(len(self._names)))} for g in self.param_groups]
        if self._eng is not None:
            host = self._export_host()
            dev = self._device()
            if dev is not None:
                host["state"] = {k: {kk: t.to(dev) for kk, t in v.items()} for k, v in host["state"].items()}
        else:
            host = self._host or dict(state={}, step=0)
        state = {}
        if host["step"] > 0 or self._host is not None:
            for i, k in enumerate(self._names):
                if k in host["state"]:
                    state[i] = dict(step=torch.tensor(float(host["step"])), exp_avg=host["state"][k]["exp_avg"], exp_avg_sq=host["state"][k]["exp_avg_sq"])
        return {"state": state, "param_groups": groups}

    def load_state_dict(self, state_dict: dict):
        """A `torch.optim.AdamW` state_dict (or a Lightning checkpoint's `optimizer_states[0]`): hyper-parameters of the one group,
        exp_avg / exp_avg_sq per parameter and the (common) step count."""
        ema_updates = self.ema_num_updates  # unchanged by a new step count
        groups = state_dict["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != len(self._names):
            raise ValueError(f"EngineAdamW: one parameter group of {len(self._names)} parameters expected, got "
                             f"{[len(g['params']) for g in groups]}")
        if groups[0].get("amsgrad"):
            raise NotImplementedError("EngineAdamW: amsgrad is not implemented")
        idx = {pid: self._names[j] for j, pid in enumerate(groups[0]["params"])}
        shapes = self._shapes()
        state, steps = {}, set()
        for pid, st in state_dict["state"].items():
            k = idx[pid]
            for kk in ("exp_avg", "exp_avg_sq"):
                if tuple(st[kk].shape) != shapes[k]:
                    raise ValueError(f"{kk} of {k}: shape {tuple(st[kk].shape)}, expected {shapes[k]}")
            state[k] = dict(exp_avg=st["exp_avg"].detach().to(torch.float32), exp_avg_sq=st["exp_avg_sq"].detach().to(torch.float32))
            steps.add(int(float(st["step"])))
        if len(steps) > 1:
            raise ValueError(f"EngineAdamW keeps one step count for all parameters, the state has {sorted(steps)}")
        if state and len(state) != len(self._names):
            raise ValueError("EngineAdamW: state for every parameter or for none")
        old = self.param_groups[0]
        hyper_changed = any(k in groups[0] and groups[0][k] != old[k] for k in ("betas", "eps", "weight_decay"))
        for k, v in groups[0].items():
            if k != "params":
                old[k] = v
        step = steps.pop() if steps else 0
        self._ema_base = ema_updates - step
        if not state:
            state = {k: dict(exp_avg=torch.zeros(shapes[k]), exp_avg_sq=torch.zeros(shapes[k])) for k in self._names}
        if self._eng is not None and not hyper_changed:
            self._eng.optim_import(self._slot, L.OPTIM_EXP_AVG, {k: v["exp_avg"] for k, v in state.items()})
            self._eng.optim_import(self._slot, L.OPTIM_EXP_AVG_SQ, {k: v["exp_avg_sq"] for k, v in state.items()})
            self._eng.optim_set_step(self._slot, step)
            return
        ema = None
        eng, slot = self._eng, self._slot
        if eng is not None:  # betas / eps / weight_decay are fixed when the engine's optimizer is created: build it again
            ema = eng.optim_export(slot, L.OPTIM_EMA, shapes) if self.ema_decay is not None else None
            self.pull()
            eng._before_close.remove(self.release_engine)
            self._eng = self._slot = None
        elif self._host is not None:
            ema = self._host.get("ema")
        self._host = dict(state=state, step=step, ema=ema)
        if eng is not None:
            self._bind(eng, slot)

    def __repr__(self):
        g = self.param_groups[0]
        return (f"EngineAdamW(lr={g['lr']}, betas={g['betas']}, eps={g['eps']}, weight_decay={g['weight_decay']}, "
                f"max_grad_norm={self.max_grad_norm}, ema_decay={self.ema_decay})")
