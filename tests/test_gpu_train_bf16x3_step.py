"""-m gpu: whole training steps under `train_precision="bf16x3"` (dyf_train_set_precision(48)): the convs the 16-bit dispatch takes
run three bf16 MFMA terms per product on (hi, lo) operand pairs, everything else is the fp32 step (csrc/train_gemm.hip,
csrc/train_halo16.hip) -- against torch.autograd over the oracle, at the project's fp32 tolerances where the objective allows.

ResNet-UNet, dim 64, mults (1, 2), 16 x 16, B = 3, no dropout (the setup of test_dim64_resnet_training_step_on_the_matrix_core_convs):
loss within 1e-4 relative, every parameter gradient within 1e-3 of the global gradient norm -- the fp32 step's own bounds.  On the CPU
the three-term model (tests/split3_refs.py) sits at 3.9e-6 there, the bf16-mixed model at 1.29e-2.

unet_simple, dim 64, 23 x 11 fields on a 128 x 128 grid, B = 3, dropout 0.15 with the engine's masks (the setup of
test_training_step_at_dim64_on_the_matrix_cores_matches_autograd_of_the_oracle; the halo forms take its 3 x 3 layers): losses within
1e-4 relative.  The gradient is NOT held to 1e-3: this objective is chaotic (the docstring of
test_training_step_with_16bit_conv_operands_matches_the_operand_rounding_model), and the three-term CPU model itself sits 6.3e-3 from
the fp32 oracle.  Instead three gradients are computed on the same inputs and masks -- the fp32 oracle's, the three-term model's and the
bf16-mixed model's (oracle.losses.training_operand_rounding) -- and the engine's whole-gradient distance from the fp32 oracle must be
at most 4 x the three-term model's (members of one cloud spread 0.54 .. 1.59 x per parameter in that test; a factor of about 2.5 on
top) and at most 0.25 x the bf16-mixed model's (the result is not plain bf16).

Deterministic mode: two identical dim-64 ResNet-UNet steps are bitwise equal, on `:det` forms.  SimpleConvNet keeps recording with
fp32 operands under 48: its step is bitwise the step under 32 (both in the deterministic mode -- the default mode's atomics differ
from run to run under either setting).
"""
import json

import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd.engine import parse_train_precision
from oracle import losses, nets
from tests import split3_refs as S3
from tests.gpu_common import DEV, build_dyffusion, seeded_pair
from tests.helpers import load_npz, split_state

pytestmark = pytest.mark.gpu


def _logged_step(m, eng, step):
    eng.form_log(True)
    try:
        out = step()
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    return out, forms


# ------------------------------------------------------------------------------------------------ ResNet-UNet
def _resnet_model(**kw):
    from tests.test_gpu_training_resnet import _mirror
    from tests.test_gpu_unet_resnet import seeded_unet
    mk = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0)
    PF, PI = seeded_unet(64, (1, 2), 2, 1, seed=91), seeded_unet(64, (1, 2), 2, 1, seed=92)
    hp = dict(timesteps=4, forward_conditioning="data", schedule="before_t1_only", additional_interpolation_steps=0,
              interpolate_before_t1=True, time_encoding="dynamics", lambda_reconstruction=1.0, lambda_reconstruction2=0.5,
              loss_function="l1", enable_interpolator_dropout=True, B=3)
    m = D.DYffusion(_mirror(PF, mk, 1, 1, 1), D.InterpolatorHandle(_mirror(PI, mk, 2, 0, 1), 4), timesteps=4, max_batch=3,
                    **{k: hp[k] for k in ("forward_conditioning", "schedule", "interpolate_before_t1", "time_encoding",
                                          "lambda_reconstruction", "lambda_reconstruction2", "loss_function")}, **kw)
    g = torch.Generator().manual_seed(17)
    batch = torch.randn(3, 1, 16, 16, generator=g), torch.randn(3, 1, 16, 16, generator=g), torch.tensor([0, 2, 3])
    return m, PF, PI, mk, hp, batch


def _resnet_step(**kw):
    m, PF, PI, mk, hp, (xt_last, cond, t) = _resnet_model(**kw)
    m.seed(7)
    m.train()
    eng = m._ensure_engine((16, 16), 3, sync=False)
    assert eng.train_precision == 48

    def step():
        out = m.p_losses(xt_last.to(DEV), cond.to(DEV), t.to(DEV), static_condition=None)
        out["loss"].backward()
        return out

    out, forms = _logged_step(m, eng, step)
    got = {k: p.grad.detach().cpu().clone() for k, p in m.model.named_parameters()}
    m.eval()
    return float(out["loss"].detach()), got, forms, (PF, PI, mk, hp, xt_last, cond, t)


def test_dim64_resnet_step_holds_the_fp32_tolerances():
    from tests.test_gpu_training_resnet import _oracle_step
    loss, got, forms, (PF, PI, mk, hp, xt_last, cond, t) = _resnet_step(train_precision="bf16x3")
    drop = nets.DropoutOff()
    drop.begin_forward = lambda: None
    want, grads = _oracle_step(PF, PI, mk, hp, xt_last, cond, t, drop, None)
    gn = float(torch.cat([v.reshape(-1) for v in grads.values()]).norm())
    errs = {k: float((got[k] - grads[k]).norm()) / gn for k in grads}
    worst = max(errs, key=errs.get)
    whole = float(torch.cat([(got[k] - grads[k]).reshape(-1) for k in grads]).norm()) / gn
    print(f"bf16x3 dim-64 ResNet-UNet: loss {loss:.6f} (oracle {float(want['loss'].detach()):.6f}), grad norm {gn:.4f}, whole gradient {whole:.2e}, "
          f"worst gradient error / grad norm {errs[worst]:.2e} ({worst}); forms {sorted(k for k in forms if '16x3' in k)}")
    assert loss == pytest.approx(float(want["loss"]), rel=1e-4)
    assert errs[worst] <= 1e-3, errs[worst]
    assert any("16x3" in k and "forward" in k for k in forms) and any("16x3" in k and "dgrad" in k for k in forms) \
        and any("16x3" in k and "wgrad" in k for k in forms), sorted(forms)
    assert not any(k.startswith("t_gemm_mfma16<") or k.startswith("t_gemm_mfma16:") for k in forms), sorted(forms)  # no one-term form ran


def test_deterministic_bf16x3_steps_are_bitwise_equal():
    la, ga, forms, _ = _resnet_step(train_precision="bf16x3", train_deterministic=True)
    lb, gb, _, _ = _resnet_step(train_precision="bf16x3", train_deterministic=True)
    names = sorted(forms)
    print(f"bf16x3 deterministic dim-64 ResNet-UNet step: forms {names}")
    assert any("16x3" in k and k.endswith(":det") for k in names) and not any(k.endswith(":atomic") for k in names), names
    assert la == lb and all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert any(bool(g.any()) for g in ga.values())


# ------------------------------------------------------------------------------------------------ unet_simple
def test_dim64_unet_simple_step_sits_with_the_three_term_model_not_with_bf16():
    from tests.test_gpu_training import _oracle_step
    mk = dict(dim=64, outer_sample_mode="bilinear", upsample_dims=[128, 128], with_time_emb=True, input_dropout=0.0, dropout=0.15)
    hp = dict(timesteps=4, schedule="before_t1_only", additional_interpolation_steps=0, additional_interpolation_steps_factor=0,
              interpolate_before_t1=True, time_encoding="dynamics", forward_conditioning="none", lambda_reconstruction=1.0,
              lambda_reconstruction2=0.5, loss_function="l1", enable_interpolator_dropout=True, model=mk)
    C, Cs, B = 3, 2, 3
    PF, PI = seeded_pair(64, C, Cs)
    g = torch.Generator().manual_seed(3)
    xt_last, cond = torch.randn(B, C, 23, 11, generator=g), torch.randn(B, C, 23, 11, generator=g)
    sc, t = torch.rand(B, Cs, 23, 11, generator=g), torch.tensor([0, 2, 3])
    seed = 4242
    m = build_dyffusion(PF, PI, mk, C, Cs, hp, max_batch=B, train_precision="bf16x3")
    m.seed(seed)
    m.train()
    m._ensure_engine((23, 11), B)
    eng = m._engine
    assert eng.train_precision == 48

    def step():
        out = m.p_losses(xt_last.to(DEV), cond.to(DEV), t.to(DEV), static_condition=sc.to(DEV))
        out["loss"].backward()
        return out

    out, forms = _logged_step(m, eng, step)
    got = {k: p.grad.detach().cpu().clone() for k, p in m.model.named_parameters()}
    m.eval()
    want32, g32, _ = _oracle_step(PF, PI, mk, hp, xt_last, cond, t, sc, seed)
    with S3.split3_operands():
        want3, g3, _ = _oracle_step(PF, PI, mk, hp, xt_last, cond, t, sc, seed)
    with losses.training_operand_rounding():
        want16, g16, _ = _oracle_step(PF, PI, mk, hp, xt_last, cond, t, sc, seed)
    cat = lambda d: torch.cat([d[k].reshape(-1) for k in sorted(g32)])
    gn = float(cat(g32).norm())
    e_eng, e3, e16 = (float((cat(d) - cat(g32)).norm()) / gn for d in (got, g3, g16))
    per = {k: float((got[k] - g32[k]).norm()) / gn for k in g32}
    worst = max(per, key=per.get)
    print(f"bf16x3 dim-64 unet_simple: loss {float(out['loss']):.6f} (fp32 oracle {float(want32['loss']):.6f}, three-term model "
          f"{float(want3['loss']):.6f}, bf16-mixed model {float(want16['loss']):.6f}); whole-gradient distance from the fp32 oracle / grad norm: "
          f"engine {e_eng:.3e}, three-term model {e3:.3e}, bf16-mixed model {e16:.3e}; engine's worst parameter {per[worst]:.2e} ({worst})")
    print(f"forms: {sorted(k for k in forms if '16' in k)}")
    for k_got, k_want in (("loss", "loss"), ("train/loss_forward", "loss_forward"), ("train/loss_forward2", "loss_forward2")):
        assert float(out[k_got]) == pytest.approx(float(want32[k_want]), rel=1e-4), k_got
    for name in ("t_halo3x3_16x3:forward", "t_halo3x3_16x3:dgrad", "t_wgrad3x3_16x3"):
        assert name in forms, sorted(forms)
    assert e_eng <= 4.0 * e3, (e_eng, e3)
    assert e_eng <= 0.25 * e16, (e_eng, e16)
    eng.close()


# ------------------------------------------------------------------------------------------------ SimpleConvNet
def test_simple_conv_net_keeps_fp32_operands_under_bf16x3():
    from tests.test_gpu_training_scn import _mirror
    z = load_npz("scn_get_loss_a.npz")
    hp = json.loads(str(z["hp"]))
    P = split_state(z, "F")
    x, c, y = (torch.from_numpy(z[k]) for k in ("x", "c", "y"))

    def step(precision):
        net = _mirror(P, hp["model"], hp["n_in"], hp["n_cond"], hp["n_out"], hp["loss_function"])
        net.train_precision = precision
        net.train_deterministic = True
        net.train()
        eng = net._own_engine(x.shape[0], x.shape[-2:])
        assert eng.train_precision == parse_train_precision(precision)
        eng.seed(99)
        loss = net.get_loss(x.to(DEV), y.to(DEV), condition=c.to(DEV))
        loss.backward()
        grads = {k: p.grad.detach().cpu().clone() for k, p in net.named_parameters()}
        net.eval()
        return float(loss.detach()), grads

    l48, g48 = step("bf16x3")
    l32, g32 = step(32)
    print(f"SimpleConvNet get_loss step: loss {l48:.6f} under bf16x3, {l32:.6f} under 32")
    assert l48 == l32
    assert sorted(g48) == sorted(g32) and all(torch.equal(g48[k], g32[k]) for k in g32), [k for k in g32 if not torch.equal(g48[k], g32[k])]
    assert any(bool(v.any()) for v in g48.values())
