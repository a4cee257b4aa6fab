"""Golden fixtures of the SimpleConvNet TRAINING step (spring-mesh experiments, model/cnn_simple.yaml) from the IMPORTED reference.

Run once where the reference checkout is present:  python tests/golden/make_scn_train_golden.py
Every file stores the inputs, the weights before the step (`F::` forecaster / the network itself, `I::` interpolator), the
gradients after loss.backward() (`G::`), the BatchNorm running statistics after the step (`B::`), the losses and the dropout seed:
all nn.Dropout layers draw from oracle.nets.DropoutSeeded(seed) in call order.

  scn_plosses_train_a   DYffusion.p_losses in train mode: dim 8, kernel_sizes [9, 7, 5, 3], dropout 0.1, h = 4, L1, lambda2 = 0.5,
                        forward_conditioning "data", B = 6 (forecaster 4 + 5 channels, interpolator 8 + 1)
  scn_plosses_train_b   kernel_sizes [5, 3], MSE, additional_interpolation_steps 2, time_encoding "normalized", lambda 0.7 / 1.0
  scn_interp_train_a    InterpolationExperiment.get_loss at h = 4 with a patched torch.randint (stage 1)
  scn_get_loss_a        SimpleConvNet built directly (6 + 2 channels = dim 8: the residual is live in block 0), with_time_emb=False,
                        kernel_sizes [3, 5], dropout 0.2, a 10 x 6 grid, B = 3: BaseModel.get_loss + backward
"""
import json
import os
import sys

import numpy as np
import torch

_DIR = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.abspath(os.path.join(_DIR, "..", "..")))
sys.path.insert(0, _DIR)
HERE = os.environ.get("DYF_GOLDEN_OUT") or _DIR

from make_golden import load_seeded, patched_dropout  # noqa: E402  (activates the reference import)
from oracle import ref_import  # noqa: E402
from oracle.nets import DropoutSeeded  # noqa: E402

torch.set_num_threads(1)  # one summation order whatever the machine: the fixtures regenerate bit for bit


def _stats(net):
    return {f"B::{k}": v.detach().numpy().copy() for k, v in net.state_dict().items()
            if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}


def gen_plosses_train():
    variants = [
        ("scn_plosses_train_a", dict(dim=8, kernel_sizes=[9, 7, 5, 3], dropout=0.1, with_time_emb=True), dict(h=4, seed=171),
         dict(forward_conditioning="data", lambda_reconstruction=1.0, lambda_reconstruction2=0.5, loss_function="l1")),
        ("scn_plosses_train_b", dict(dim=8, kernel_sizes=[5, 3], dropout=0.1, with_time_emb=True), dict(h=4, seed=172),
         dict(forward_conditioning="data", additional_interpolation_steps=2, lambda_reconstruction=0.7, lambda_reconstruction2=1.0,
              loss_function="mse", time_encoding="normalized")),
    ]
    for name, mk, meta, dk in variants:
        h = meta["h"]
        dkw = dict(enable_interpolator_dropout=True)
        dkw.update(dk)
        exp, ipol = ref_import.build_reference_dyffusion(system="spring-mesh", model="cnn_simple", model_kwargs=mk, horizon=h,
                                                         diffusion_kwargs=dkw)
        load_seeded(exp.model.model, seed=131)
        load_seeded(ipol.model, seed=132)
        dyn = exp.model
        dyn.train()
        dyn.interpolator.eval()  # frozen (dyffusion.py:468): eval-mode BatchNorm, its Dropout stays active (:154-160)
        for p in dyn.model.parameters():
            p.requires_grad_(True)
        assert not ipol.model.training and all(not p.requires_grad for p in ipol.model.parameters())
        T = dyn.num_timesteps
        g = torch.Generator().manual_seed(119)
        B = 6
        xt_last = torch.randn(B, 4, 10, 10, generator=g)
        cond = torch.randn(B, 4, 10, 10, generator=g)
        sc = torch.rand(B, 1, 10, 10, generator=g)
        t = torch.tensor([0, 1, T - 1, 2 % T, T - 2, 0])
        sd0 = {k: v.detach().clone() for k, v in dyn.model.state_dict().items()}
        with patched_dropout(DropoutSeeded(seed=meta["seed"])):
            out = dyn.p_losses(xt_last, cond, t, static_condition=sc)
            out["loss"].backward()
        assert all(p.grad is None for p in ipol.model.parameters())
        hp = dict(timesteps=h, num_timesteps=T, model=mk, B=B, dropout_seed=meta["seed"],
                  **{k: dkw.get(k, d) for k, d in dict(
                      schedule="before_t1_only", additional_interpolation_steps=0, additional_interpolation_steps_factor=0,
                      interpolate_before_t1=True, time_encoding="dynamics", forward_conditioning="none",
                      lambda_reconstruction=1.0, lambda_reconstruction2=0.0, loss_function="l1",
                      enable_interpolator_dropout=True).items()})
        arrs = {f"F::{k}": v.numpy() for k, v in sd0.items()}
        arrs.update({f"I::{k}": v.numpy() for k, v in ipol.model.state_dict().items()})
        arrs.update({f"G::{k}": p.grad.numpy() for k, p in dyn.model.named_parameters()})
        arrs.update(_stats(dyn.model))
        vals = {k.split("/")[-1]: float(v) for k, v in out.items()}
        np.savez_compressed(os.path.join(HERE, name + ".npz"), xt_last=xt_last.numpy(), cond=cond.numpy(), sc=sc.numpy(),
                            t=t.numpy(), hp=json.dumps(hp), losses=json.dumps(vals), **arrs)
        n_par = sum(p.numel() for p in dyn.model.parameters())
        gn = float(torch.cat([p.grad.reshape(-1) for p in dyn.model.parameters()]).norm())
        print(name, vals, "parameters", n_par, sum(p.numel() for p in ipol.model.parameters()), "grad norm", gn)


def gen_interp_train():
    mk = dict(dim=8, kernel_sizes=[9, 7, 5, 3], dropout=0.1, with_time_emb=True)
    name, h, loss_fn, seed, idx = "scn_interp_train_a", 4, "mse", 181, [0, 2, 1, 2, 0]
    _, ipol = ref_import.build_reference_dyffusion(system="spring-mesh", model="cnn_simple", model_kwargs=mk, horizon=h)
    load_seeded(ipol.model, seed=141)
    from src.utilities.utils import get_loss
    ipol.model.criterion = get_loss(loss_fn)
    ipol.train()
    for p_ in ipol.model.parameters():
        p_.requires_grad_(True)
    g = torch.Generator().manual_seed(123)
    B = len(idx)
    dynamics = torch.randn(B, 1 + h, 4, 10, 10, generator=g)
    cond = torch.rand(B, 1, 10, 10, generator=g)
    sd0 = {k: v.detach().clone() for k, v in ipol.model.state_dict().items()}
    orig_randint = torch.randint
    torch.randint = lambda *a, **k: torch.tensor(idx, dtype=torch.long)
    try:
        with patched_dropout(DropoutSeeded(seed=seed)):
            loss = ipol.get_loss(dict(dynamics=dynamics, condition=cond))
            loss.backward()
    finally:
        torch.randint = orig_randint
    times = torch.tensor(list(ipol.horizon_range))[torch.tensor(idx)]
    arrs = {f"F::{k}": v.numpy() for k, v in sd0.items()}
    arrs.update({f"G::{k}": p_.grad.numpy() for k, p_ in ipol.model.named_parameters()})
    arrs.update(_stats(ipol.model))
    hp = dict(horizon=h, window=1, model=mk, loss_function=loss_fn, dropout_seed=seed, randint=idx,
              horizon_range=[int(v) for v in ipol.horizon_range])
    np.savez_compressed(os.path.join(HERE, name + ".npz"), dynamics=dynamics.numpy(), cond=cond.numpy(), t=times.numpy(),
                        losses=json.dumps(dict(loss=float(loss))), hp=json.dumps(hp), **arrs)
    print(name, "times", times.tolist(), "loss", float(loss), "grad norm",
          float(torch.cat([p_.grad.reshape(-1) for p_ in ipol.model.parameters()]).norm()))


def gen_get_loss():
    from src.models.simple_conv_net import SimpleConvNet
    mk = dict(dim=8, kernel_sizes=[3, 5], dropout=0.2, with_time_emb=False)
    name, seed, loss_fn = "scn_get_loss_a", 191, "l1"
    net = SimpleConvNet(num_input_channels=6, num_output_channels=3, num_conditional_channels=2, spatial_shape=(10, 6),
                        loss_function=loss_fn, verbose=False, **mk)
    load_seeded(net, seed=151)
    net.train()
    g = torch.Generator().manual_seed(127)
    B = 3
    x = torch.randn(B, 6, 10, 6, generator=g)
    c = torch.rand(B, 2, 10, 6, generator=g)
    y = torch.randn(B, 3, 10, 6, generator=g)
    sd0 = {k: v.detach().clone() for k, v in net.state_dict().items()}
    with patched_dropout(DropoutSeeded(seed=seed)):
        loss = net.get_loss(x, y, condition=c)
        loss.backward()
    arrs = {f"F::{k}": v.numpy() for k, v in sd0.items()}
    arrs.update({f"G::{k}": p_.grad.numpy() for k, p_ in net.named_parameters()})
    arrs.update(_stats(net))
    hp = dict(model=mk, loss_function=loss_fn, dropout_seed=seed, n_in=6, n_cond=2, n_out=3)
    np.savez_compressed(os.path.join(HERE, name + ".npz"), x=x.numpy(), c=c.numpy(), y=y.numpy(),
                        losses=json.dumps(dict(loss=float(loss))), hp=json.dumps(hp), **arrs)
    print(name, "loss", float(loss), "grad norm", float(torch.cat([p_.grad.reshape(-1) for p_ in net.parameters()]).norm()))


if __name__ == "__main__":
    gen_plosses_train()
    gen_interp_train()
    gen_get_loss()
