"""-m gpu: the engine-resident optimizer (csrc/train_optim.hip, dyffusion_amd/optim.py): AdamW + clip_grad_norm_ + LitEma on the
engine's own weights, gradients and state, against tests/golden/optim_adamw_ema*.npz (torch.optim.AdamW + clip_grad_norm_ + the
reference's LitEma on the CPU, five steps with seeded gradients; tests/golden/make_optim_golden.py) and against torch.optim on the
gradients the engine itself computed.

Networks: the forecasters of plosses_train_a.npz (unet_simple, dim 4: BatchNorm statistics, a ConvTranspose2d readout, 32x32x4x4
convs = 16 384 elements = four chunks of OPT_CHUNK = 4096, short vectors) and of plosses_train_resnet_a.npz
(unet.Unet, dim 8: weight-standardised convs, LayerNorm gains, tensors whose size is no multiple of 4, length-1 and length-3 vectors).

Bound (stated by the issue): per tensor, 4 x the max-abs deviation of torch's own fp32 CPU run from a float64 run of the same five
steps (stored by the generator as <net>::dev_<family>) -- one factor of 2 for a different but legitimate operation order, one for the
reduction order of the norm that feeds the clip coefficient.  Each test prints the ratio it measured (deviation / that yardstick).

Measured on an MI355X: see the docstring of test_injected_gradients_match_torch_adamw_clip_and_litema.
"""
import copy
import importlib.util
import json
import os

import numpy as np
import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from tests.gpu_common import DEV, build_dyffusion
from tests.helpers import GOLDEN, load_npz, split_state

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location("make_optim_golden", os.path.join(GOLDEN, "make_optim_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)  # HP, seeded_gradients: the recipe of the fixture's gradients (the reference is not imported by this)
HP = G.HP
_FIX = {}


def _fixture():
    if not _FIX:
        _FIX["main"] = load_npz("optim_adamw_ema.npz")
        _FIX["moments"] = load_npz("optim_adamw_ema_moments.npz")
        assert json.loads(str(_FIX["main"]["hp"])) == HP
    return _FIX["main"], _FIX["moments"]


def _build(tag, dropout=False, **hp_over):
    """(model, inputs of one p_losses call) for the fixture network `tag`, freshly built."""
    if tag == "simple":
        z = load_npz("plosses_train_a.npz")
        hp = dict(json.loads(str(z["hp"])), **hp_over)
        mk = dict(hp["model"]) if dropout else dict(hp["model"], dropout=0.0)
        m = build_dyffusion(split_state(z, "F"), split_state(z, "I"), mk, 4, 1, hp, max_batch=hp["B"])
        batch = dict(xt_last=torch.from_numpy(z["xt_last"]).to(DEV), condition=torch.from_numpy(z["cond"]).to(DEV),
                     t=torch.from_numpy(z["t"]).to(DEV), static_condition=torch.from_numpy(z["sc"]).to(DEV))
        return m, batch
    from tests.test_gpu_training_resnet import _build as build_resnet
    z = load_npz("plosses_train_resnet_a.npz")
    hp = dict(json.loads(str(z["hp"])), **hp_over)
    mk = dict(hp["model"]) if dropout else dict(hp["model"], block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0)
    m, _, _ = build_resnet(z, hp, mk)
    batch = dict(xt_last=torch.from_numpy(z["xt_last"]).to(DEV), condition=torch.from_numpy(z["cond"]).to(DEV),
                 t=torch.from_numpy(z["t"]).to(DEV), static_condition=None)
    return m, batch


def _attach(m, batch, **kw):
    """An EngineAdamW on `m` with the fixture's hyper-parameters, bound to m's engine."""
    args = dict(lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"], max_grad_norm=HP["max_norm"],
                ema_decay=HP["ema_decay"])
    args.update(kw)
    m.train()
    m._ensure_engine(batch["condition"].shape[-2:], batch["condition"].shape[0], sync=False)
    return D.EngineAdamW(m, **args)


def _shapes(m, tag="simple"):
    """{name: shape} in the FIXTURE's tensor order (the reference's state_dict order, which the seeded gradients are drawn in; the mirror
    registers its parameters in another order)."""
    names = json.loads(str(_fixture()[0][f"{tag}::names"]))
    have = {k: tuple(p.shape) for k, p in m.model.named_parameters()}
    assert sorted(have) == sorted(names)
    return {k: have[k] for k in names}


def _ratios(got, want, dev, names):
    """max over tensors of max|got - want| / dev[tensor], and the tensor it is reached at."""
    worst, where = 0.0, None
    for k, d in zip(names, dev):
        r = float((got[k].detach().double().cpu() - want[k].detach().double()).abs().max()) / float(d)
        if r > worst:
            worst, where = r, k
    return worst, where


def _five_steps(tag, check_layouts=False):
    m, batch = _build(tag)
    opt = _attach(m, batch)
    shapes = _shapes(m, tag)
    stats0 = opt.export("stats")
    norms = []
    for s in range(5):
        opt.param_groups[0]["lr"] = HP["lrs"][s]
        opt.import_gradients(G.seeded_gradients(shapes, s))
        opt.step()
        norms.append(opt.last_grad_norm)
        assert not opt.last_step_skipped
        if check_layouts:  # w and wt never disagree; the gradients are cleared; BatchNorm statistics do not move
            w, wf = opt.export("weight"), opt.export("weight_fwd")
            assert wf and all(torch.equal(w[k], wf[k]) for k in wf), s
            assert all(not g.any() for g in opt.export("grad").values()), s
            stats = opt.export("stats")
            assert all(torch.equal(stats[k], stats0[k]) for k in stats0), s
    out = {fam: opt.export(fam) for fam in ("weight", "exp_avg", "exp_avg_sq", "ema")}
    return m, opt, out, norms


@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_injected_gradients_match_torch_adamw_clip_and_litema(tag):
    """Five engine steps on the fixture's seeded gradients against the fixture.

    Measured (MI355X, worst tensor, deviation / torch's own fp32-vs-float64 deviation; the bound is 4):
    simple: weight 0.08, exp_avg 0 and exp_avg_sq 0 (80/80 tensors bitwise equal), ema 0.08; resnet: weight 0.55, exp_avg 1.91, exp_avg_sq 1.63, ema 0.57."""
    z, mo = _fixture()
    names = json.loads(str(z[f"{tag}::names"]))
    m, opt, out, norms = _five_steps(tag, check_layouts=True)
    assert opt.step_count == 5
    for s, (a, b) in enumerate(zip(norms, z[f"{tag}::norms"])):
        print(f"{tag} step {s + 1}: grad norm {a:.9g} (torch fp32 {b:.9g})")
        assert a == pytest.approx(b, rel=2e-6)  # torch reduces in fp32, tensor by tensor; the engine in double
    want = {"weight": {k: torch.from_numpy(z[f"{tag}::w::{k}"]) for k in names},
            "ema": {k: torch.from_numpy(z[f"{tag}::ema::{k.replace('.', '')}"]) for k in names},
            "exp_avg": {k: torch.from_numpy(mo[f"{tag}::exp_avg::{k}"]) for k in names},
            "exp_avg_sq": {k: torch.from_numpy(mo[f"{tag}::exp_avg_sq::{k}"]) for k in names}}
    fails = []
    for fam, key in (("weight", "w"), ("exp_avg", "exp_avg"), ("exp_avg_sq", "exp_avg_sq"), ("ema", "ema")):
        worst, where = _ratios(out[fam], want[fam], z[f"{tag}::dev_{key}"], names)
        exact = sum(torch.equal(out[fam][k], want[fam][k]) for k in names)
        print(f"{tag} {fam}: worst deviation / torch's fp32-vs-float64 deviation = {worst:.3f} at {where}; {exact}/{len(names)} tensors bitwise equal")
        if worst > 4.0:
            fails.append((fam, worst, where))
    # the EMA buffers under LitEma's names
    ema_sd = opt.ema_state_dict()
    assert int(ema_sd["num_updates"]) == 5 and set(ema_sd) == {k.replace(".", "") for k in names} | {"decay", "num_updates"}
    assert not fails, fails


@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_two_runs_are_bitwise_equal(tag):
    _, _, a, na = _five_steps(tag)
    _, _, b, nb = _five_steps(tag)
    assert na == nb
    for fam in a:
        assert all(torch.equal(a[fam][k], b[fam][k]) for k in a[fam]), fam


@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_non_finite_gradient_skips_the_step(tag):
    z, _ = _fixture()
    names = json.loads(str(z[f"{tag}::names"]))
    m, batch = _build(tag)
    opt = _attach(m, batch)
    shapes = _shapes(m, tag)
    before = {fam: opt.export(fam) for fam in ("weight", "weight_fwd", "exp_avg", "exp_avg_sq", "ema")}
    bad = G.seeded_gradients(shapes, 0)
    bad[names[-1]].reshape(-1)[-1] = float("inf")
    opt.import_gradients(bad)
    opt.step()
    assert opt.last_step_skipped and not np.isfinite(opt.last_grad_norm)
    assert opt.step_count == 0
    after = {fam: opt.export(fam) for fam in before}
    for fam in before:
        assert all(torch.equal(before[fam][k], after[fam][k]) for k in before[fam]), fam
    assert all(not g.any() for g in opt.export("grad").values())  # the gradients are cleared all the same
    # the next finite step is step 1 of the fixture's run: its recorded norm, a fresh engine's first step bit for bit, and torch's first step
    good = G.seeded_gradients(shapes, 0)
    opt.import_gradients(good)
    opt.step()
    assert not opt.last_step_skipped and opt.step_count == 1
    assert opt.last_grad_norm == pytest.approx(float(z[f"{tag}::norms"][0]), rel=2e-6)
    m2, batch2 = _build(tag)
    opt2 = _attach(m2, batch2)
    opt2.import_gradients(good)
    opt2.step()
    for fam in ("weight", "exp_avg", "exp_avg_sq", "ema"):
        a, b = opt.export(fam), opt2.export(fam)
        assert all(torch.equal(a[k], b[k]) for k in a), fam
    p0 = dict(_build(tag)[0].model.named_parameters())
    ps = [torch.nn.Parameter(p0[k].detach().cpu().clone()) for k in names]
    ref = torch.optim.AdamW(ps, lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"], foreach=False)
    for p, g in zip(ps, good.values()):
        p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_(ps, HP["max_norm"], foreach=False)
    ref.step()
    worst, where = _ratios(opt.export("weight"), dict(zip(names, ps)), z[f"{tag}::dev_w"], names)
    print(f"{tag}: first finite step after the skipped one vs torch: worst ratio {worst:.3f} at {where}")
    assert worst <= 4.0


def _shadow_step(names, ps, ref, grads, max_norm):
    """One step of the CPU torch.optim shadow `ref` over `ps` (named `names`, in that order) on the gradients {name: tensor}."""
    for k, p in zip(names, ps):
        p.grad = grads[k].detach().cpu().clone()
    if max_norm:
        torch.nn.utils.clip_grad_norm_(ps, max_norm, foreach=False)
    ref.step()


@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_resident_loop_follows_torch_on_its_own_gradients(tag):
    """p_losses -> backward -> step, three times; the engine's own gradients, exported before each step, drive a CPU torch.optim.AdamW +
    clip_grad_norm_ shadow (which sidesteps the run-to-run last-bit differences of the weight-gradient atomics)."""
    z, _ = _fixture()
    names = json.loads(str(z[f"{tag}::names"]))
    m, batch = _build(tag)
    opt = _attach(m, batch, ema_decay=None)
    p0 = dict(m.model.named_parameters())
    ps = [torch.nn.Parameter(p0[k].detach().cpu().clone()) for k in names]
    ref = torch.optim.AdamW(ps, lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"], foreach=False)
    losses = []
    for it in range(3):
        out = m.p_losses(**batch)
        out["loss"].backward()
        losses.append(float(out["loss"]))
        assert all(p.grad is None for p in m.model.parameters())
        grads = opt.export("grad")
        assert any(g.any() for g in grads.values())
        opt.step()
        _shadow_step(names, ps, ref, grads, HP["max_norm"])
        worst, where = _ratios(opt.export("weight"), dict(zip(names, ps)), z[f"{tag}::dev_w"], names)
        print(f"{tag} iteration {it + 1}: loss {losses[-1]:.6f}, grad norm {opt.last_grad_norm:.4f}, worst ratio {worst:.3f} at {where}")
        assert worst <= 4.0, (it, worst, where)
    losses.append(float(m.p_losses(**batch)["loss"]))
    print(f"{tag}: loss of the same batch over three resident steps: {[round(v, 5) for v in losses]}")
    assert losses[-1] < losses[0]
    m.eval()


def test_gradients_accumulate_in_the_engine_across_backward_calls():
    m, batch = _build("simple")
    opt = _attach(m, batch, ema_decay=None)

    def backward():
        m.p_losses(**batch)["loss"].backward()

    backward()
    g1 = opt.export("grad")
    opt.zero_grad()
    assert all(not g.any() for g in opt.export("grad").values())
    backward()
    g2 = opt.export("grad")
    opt.zero_grad()
    backward()
    backward()
    g12 = opt.export("grad")
    gn = float(torch.cat([(g1[k] + g2[k]).reshape(-1) for k in g1]).norm())
    worst = max(float((g12[k] - (g1[k] + g2[k])).norm()) for k in g1) / gn
    print(f"two backwards, one step: worst per-tensor |accumulated - (g1 + g2)| / grad norm = {worst:.2e}")
    assert worst <= 1e-3
    opt.step()
    assert opt.step_count == 1 and opt.last_grad_norm == pytest.approx(gn, rel=1e-3)
    m.eval()


def _fresh_sample(tag, state, batch):
    """The sample of a freshly built model of `tag` with the forecaster's state_dict `state`."""
    f, fbatch = _build(tag, enable_interpolator_dropout=False)
    f.model.load_state_dict({k: v.detach().cpu() for k, v in state.items()})
    f.eval()
    return f.sample(batch["condition"], static_condition=batch["static_condition"])


def test_sampling_sees_the_resident_update_and_the_ema_scope():
    tag = "simple"
    m, batch = _build(tag, enable_interpolator_dropout=False)
    opt = _attach(m, batch)
    for _ in range(2):
        m.p_losses(**batch)["loss"].backward()
        opt.step()
    m.eval()
    got = m.sample(batch["condition"], static_condition=batch["static_condition"])
    state = {k: v.clone() for k, v in m.model.state_dict().items()}  # pull()'s state_dict
    assert int(state["input_ops.0.ops.1.num_batches_tracked"]) == 4  # two forecaster passes per iteration
    want = _fresh_sample(tag, state, batch)
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
    w_before = opt.export("weight")
    shadow = opt.export("ema")
    assert any(not torch.equal(shadow[k], w_before[k]) for k in shadow)
    with opt.ema_scope():
        got_ema = m.sample(batch["condition"], static_condition=batch["static_condition"])
    want_ema = _fresh_sample(tag, dict(state, **shadow), batch)
    assert all(torch.equal(got_ema[k], want_ema[k]) for k in want_ema)
    assert any(not torch.equal(got_ema[k], got[k]) for k in got)
    w_after, wf_after = opt.export("weight"), opt.export("weight_fwd")
    assert all(torch.equal(w_after[k], w_before[k]) for k in w_before)
    assert all(torch.equal(wf_after[k], w_before[k]) for k in wf_after)
    again = m.sample(batch["condition"], static_condition=batch["static_condition"])  # and sampling is back on the trained weights
    assert all(torch.equal(again[k], got[k]) for k in got)
    # editing the module while steps are pending is refused
    m.train()
    m.p_losses(**batch)["loss"].backward()
    opt.step()
    with torch.no_grad():
        next(m.model.parameters()).add_(1.0)
    with pytest.raises(RuntimeError, match="pending"):
        m.p_losses(**batch)
    m.eval()


def test_optimizer_hand_over_between_torch_and_the_engine():
    tag = "simple"
    z, _ = _fixture()
    names = json.loads(str(z[f"{tag}::names"]))
    m, batch = _build(tag)
    m.train()
    topt = torch.optim.AdamW(m.model.parameters(), lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"],
                             foreach=False)
    for _ in range(2):  # two classic iterations: gradients into param.grad, torch.optim on the module
        topt.zero_grad()
        m.p_losses(**batch)["loss"].backward()
        topt.step()
    handed = copy.deepcopy(topt.state_dict())  # (load_state_dict keeps the `step` tensors it is given: every reader gets its own copy)
    shapes = _shapes(m, tag)
    g3 = G.seeded_gradients(shapes, 4)
    # torch's third step, on a CPU copy of the module and of the optimizer
    mnames = [k for k, _ in m.model.named_parameters()]  # torch's state is indexed in the module's own parameter order
    ps = [torch.nn.Parameter(p.detach().cpu().clone()) for p in m.model.parameters()]
    ref = torch.optim.AdamW(ps, lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"], foreach=False)
    ref.load_state_dict(copy.deepcopy(handed))
    _shadow_step(mnames, ps, ref, g3, None)
    # the engine's third step
    opt = D.EngineAdamW(m, lr=1.0, max_grad_norm=None, ema_decay=None)
    opt.load_state_dict(handed)
    assert opt.param_groups[0]["lr"] == HP["lrs"][0] and opt.step_count == 2
    opt.import_gradients(g3)
    opt.step()
    worst, where = _ratios(opt.export("weight"), dict(zip(mnames, ps)), z[f"{tag}::dev_w"], names)
    print(f"hand-over torch -> engine: worst ratio {worst:.3f} at {where}")
    assert worst <= 4.0
    # and back: the engine's state loads into torch.optim.AdamW
    back = torch.optim.AdamW(m.model.parameters(), lr=1.0)
    back.load_state_dict(opt.state_dict())
    assert len(back.state) == len(names) and all(float(s["step"]) == 3.0 for s in back.state.values())
    assert opt.step_count == 3
    m.eval()


def test_stage1_interpolator_trains_resident_in_its_own_slot():
    """UNet.get_loss (stage 1) on the interpolator of a pair: the optimizer lives in slot NET_INTERPOLATOR."""
    z, _ = _fixture()
    m, batch = _build("simple")
    m._ensure_engine(batch["condition"].shape[-2:], batch["condition"].shape[0], sync=False)
    net = m._ipol_net
    assert net._engine_slot == L.NET_INTERPOLATOR
    net.train()
    opt = D.EngineAdamW(net, lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"],
                        max_grad_norm=HP["max_norm"], ema_decay=None)
    names = [k for k, _ in net.named_parameters()]
    ps = [torch.nn.Parameter(p.detach().cpu().clone()) for p in net.parameters()]
    ref = torch.optim.AdamW(ps, lr=HP["lrs"][0], betas=tuple(HP["betas"]), eps=HP["eps"], weight_decay=HP["weight_decay"], foreach=False)
    inputs = torch.cat([batch["condition"], batch["xt_last"]], 1)
    time = torch.full((inputs.shape[0],), 2.0, device=DEV)
    # the yardstick: the forecaster's tensors of the same names have the same shapes except the stem, whose entry serves as well
    fnames = json.loads(str(z["simple::names"]))
    dev = dict(zip(fnames, z["simple::dev_w"]))
    for it in range(2):
        loss = net.get_loss(inputs, batch["xt_last"], condition=batch["static_condition"], time=time)
        loss.backward()
        assert all(p.grad is None for p in net.parameters())
        grads = opt.export("grad")
        assert opt._slot == L.NET_INTERPOLATOR and any(g.any() for g in grads.values())
        opt.step()
        _shadow_step(names, ps, ref, grads, HP["max_norm"])
        worst, where = _ratios(opt.export("weight"), dict(zip(names, ps)), [dev[k] for k in names], names)
        print(f"interpolator iteration {it + 1}: loss {float(loss):.6f}, worst ratio {worst:.3f} at {where}")
        assert worst <= 4.0
    net.eval()


def test_state_and_pending_gradients_survive_a_replaced_engine():
    """A larger batch makes DYffusion build a new engine: the optimizer's moments, EMA, step count AND the gradients of a backward that
    has not been stepped on yet move with it (export and import are exact)."""
    m, batch = _build("simple")
    opt = _attach(m, batch)
    m.p_losses(**batch)["loss"].backward()
    opt.step()
    m.p_losses(**batch)["loss"].backward()  # accumulated, not yet applied
    before = {fam: opt.export(fam) for fam in ("weight", "grad", "exp_avg", "exp_avg_sq", "ema")}
    assert any(g.any() for g in before["grad"].values())
    old = m._engine
    hw, nb = batch["condition"].shape[-2:], batch["condition"].shape[0]
    new = m._ensure_engine(hw, 2 * nb, sync=False)
    assert new is not old and opt._eng is None
    m.p_losses(**batch)  # a training forward on the new engine; its loss is never back-propagated
    after = {fam: opt.export(fam) for fam in before}  # binds to the new engine
    assert opt._eng is new and opt.step_count == 1
    for fam in before:
        assert all(torch.equal(before[fam][k], after[fam][k]) for k in before[fam]), fam
    opt.step()
    assert opt.step_count == 2 and not opt.last_step_skipped
    m.eval()
