"""-m gpu: the training step of the SimpleConvNet backbone (spring-mesh experiments, model/cnn_simple.yaml) on the engine: the third
walk over the recorded ops (csrc/train_resnet.inc sc_walk) -- `DYffusion.p_losses` / `InterpolationExperiment.get_loss` /
`SimpleConvNet.get_loss` in train mode + `loss.backward()`, the deterministic mode and the engine-resident AdamW.

Reference: torch.autograd in float64 over tests/scn_train_refs.py, which tests/test_scn_train_refs.py pins to the imported reference's
own losses, gradients and running statistics (tests/golden/scn_*.npz, masks from DropoutSeeded).  The engine draws its dropout masks
from its own generator -- a recorded forward takes no injected masks, and the C ABI gets no new entry point for it -- so the reference
replays exactly those masks, rebuilt on the host (tests/rng_host.py): forward counter 0 = first interpolator call, 1 = first
forecaster pass, 2 / 3 = the second pair; site i = block i (the streams sampling draws, csrc/simple_conv_net.hip).  The fixtures' own
gradients (other masks) serve as an anchor of scale, as in tests/test_gpu_training.py.

Tolerances (tests/test_gpu_training.py:8-9, 93): losses within 1e-4 relative, every parameter's gradient within 1e-3 of the GLOBAL
gradient norm (under batch statistics d loss / d conv.bias is exactly zero and the reference leaves 3e-9 of the gradient norm there:
a per-tensor relative bound would compare noise), running statistics rtol 1e-4 / atol 1e-6."""
import json

import numpy as np
import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from dyffusion_amd.optim import ema_decay_at
from oracle import init as oinit
from tests import scn_train_refs as S
from tests.gpu_common import DEV
from tests.helpers import load_npz, rel_rms, split_state

pytestmark = pytest.mark.gpu
LOSS_RTOL, GRAD_TOL = 1e-4, 1e-3


def _mirror(P, mk, n_in, n_cond, n_out, loss_function="mse"):
    net = D.SimpleConvNet(dim=mk["dim"], with_time_emb=mk.get("with_time_emb", True), kernel_sizes=mk["kernel_sizes"],
                          dropout=mk.get("dropout", 0.0), num_input_channels=n_in, num_output_channels=n_out,
                          num_conditional_channels=n_cond, loss_function=loss_function)
    net.load_state_dict(P, strict=True)
    return net


def _pair(PF, PI, hp, C=4, Cs=1, **engine_kw):
    mk = hp["model"]
    f_cond = Cs + (0 if hp.get("forward_conditioning", "none") == "none" else C)
    F, I = _mirror(PF, mk, C, f_cond, C), _mirror(PI, mk, 2 * C, Cs, C)
    keys = ["forward_conditioning", "schedule", "additional_interpolation_steps", "additional_interpolation_steps_factor",
            "interpolate_before_t1", "time_encoding", "enable_interpolator_dropout", "lambda_reconstruction", "lambda_reconstruction2",
            "loss_function"]
    return D.DYffusion(F, D.InterpolatorHandle(I, hp["timesteps"], 1), timesteps=hp["timesteps"], **{k: hp[k] for k in keys if k in hp},
                       **engine_kw)


def _check_step(tag, losses, want_losses, got, want, stats_got, stats_want):
    for k, v in want_losses.items():
        assert losses[k] == pytest.approx(v, rel=LOSS_RTOL), k
    worst, which, gn = S.grad_errors(got, want)
    print(f"{tag}: loss {losses['loss']:.6f}, grad norm {gn:.4f}, worst per-tensor gradient error / grad norm = {worst:.2e} ({which})")
    assert worst <= GRAD_TOL
    assert stats_want
    for k, v in stats_want.items():
        assert torch.allclose(stats_got[k].cpu(), v.float(), rtol=1e-4, atol=1e-6), k
    return gn


def _plosses(m, batch, seed):
    m.seed(seed)
    m.train()
    out = m.p_losses(batch["xt_last"].to(DEV), batch["cond"].to(DEV), batch["t"].to(DEV), static_condition=batch["sc"].to(DEV))
    assert set(out) == {"loss", "train/loss_forward", "train/loss_forward2"}
    out["loss"].backward()
    losses = {"loss": float(out["loss"].detach()), "loss_forward": float(out["train/loss_forward"]), "loss_forward2": float(out["train/loss_forward2"])}
    return losses, {k: p.grad.detach().cpu() for k, p in m.model.named_parameters()}


def _ref_plosses(PF, PI, hp, batch, seed):
    drop = S.EngineMasks(seed)
    return S.plosses_step(PF, PI, hp, batch["xt_last"], batch["cond"], batch["t"], batch["sc"], drop, drop.begin_forward)


# ------------------------------------------------------------------------------------------------ 1. forecaster step
@pytest.mark.parametrize("name", ["scn_plosses_train_a", "scn_plosses_train_b"])
def test_forecaster_step_matches_autograd_of_the_reference_restatement(name):
    z = load_npz(name + ".npz")
    hp = json.loads(str(z["hp"]))
    PF, PI = split_state(z, "F"), split_state(z, "I")
    batch = {k: torch.from_numpy(z[k]) for k in ("xt_last", "cond", "sc", "t")}
    m = _pair(PF, PI, hp, max_batch=hp["B"])
    seed = 20240928
    losses, got = _plosses(m, batch, seed)
    want_losses, want, stats = _ref_plosses(PF, PI, hp, batch, seed)
    gn = _check_step(name, losses, want_losses, got, want, m.model.state_dict(), stats)
    assert all(p.grad is None for p in m._ipol_net.parameters())  # frozen: the second term is differentiated THROUGH it only
    G = split_state(z, "G")  # the reference's own gradients (DropoutSeeded masks): the same scale
    assert 0.5 <= gn / float(torch.cat([g.reshape(-1) for g in G.values()]).norm()) <= 2.0
    sd = m.model.state_dict()
    assert int(sd["convs.0.norm.num_batches_tracked"]) == int(z["B::convs.0.norm.num_batches_tracked"]) == 2
    isd = m._ipol_net.state_dict()
    assert all(torch.equal(isd[k].cpu(), PI[k]) for k in PI)  # running statistics of the interpolator untouched
    m.eval()


# ------------------------------------------------------------------------------------------------ 2. stage 1 and direct get_loss
def test_interpolator_stage1_matches_autograd_of_the_reference_restatement(monkeypatch):
    z = load_npz("scn_interp_train_a.npz")
    hp = json.loads(str(z["hp"]))
    P = split_state(z, "F")
    dyn, cond, t = torch.from_numpy(z["dynamics"]), torch.from_numpy(z["cond"]), torch.from_numpy(z["t"])
    B, C = dyn.shape[0], dyn.shape[2]
    net = _mirror(P, hp["model"], (hp["window"] + 1) * C, cond.shape[1], C, hp["loss_function"])
    exp = D.InterpolationExperiment(net, horizon=hp["horizon"], window=hp["window"])
    exp.train()
    seed = 777
    net._own_engine(B, dyn.shape[-2:]).seed(seed)
    idx = torch.tensor(hp["randint"])
    monkeypatch.setattr(torch, "randint", lambda *a, **k: idx.to(k.get("device", "cpu")))
    loss = exp.get_loss(dict(dynamics=dyn.to(DEV), condition=cond.to(DEV)))
    monkeypatch.undo()
    loss.backward()
    drop = S.EngineMasks(seed)
    drop.begin_forward()
    want_losses, want, stats = S.interp_step(P, hp, dyn, cond, t, drop)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    gn = _check_step("scn_interp_train_a", {"loss": float(loss.detach())}, want_losses, got, want, net.state_dict(), stats)
    G = split_state(z, "G")
    assert 0.5 <= gn / float(torch.cat([g.reshape(-1) for g in G.values()]).norm()) <= 2.0
    assert int(net.state_dict()["convs.0.norm.num_batches_tracked"]) == 1
    # eval mode: plain forward + criterion, no tape
    exp.eval()
    le = net.get_loss(exp.get_inputs_from_dynamics(dyn.to(DEV)), dyn[torch.arange(B), hp["window"] + t - 1].to(DEV), time=t.to(DEV), condition=cond.to(DEV))
    assert le.requires_grad is False and float(le) > 0


def test_get_loss_without_time_embedding_and_a_live_residual_in_block_0():
    """with_time_emb=False (no FiLM operand), 6 + 2 = 8 = dim input channels (block 0 adds the network INPUT back), a 10 x 6 grid."""
    z = load_npz("scn_get_loss_a.npz")
    hp = json.loads(str(z["hp"]))
    P = split_state(z, "F")
    x, c, y = (torch.from_numpy(z[k]) for k in ("x", "c", "y"))
    net = _mirror(P, hp["model"], hp["n_in"], hp["n_cond"], hp["n_out"], hp["loss_function"])
    net.train()
    seed = 99
    net._own_engine(x.shape[0], x.shape[-2:]).seed(seed)
    loss = net.get_loss(x.to(DEV), y.to(DEV), condition=c.to(DEV))
    loss.backward()
    drop = S.EngineMasks(seed)
    drop.begin_forward()
    want_losses, want, stats = S.get_loss_step(P, hp, x, c, y, drop)
    got = {k: p.grad.detach().cpu() for k, p in net.named_parameters()}
    gn = _check_step("scn_get_loss_a", {"loss": float(loss.detach())}, want_losses, got, want, net.state_dict(), stats)
    G = split_state(z, "G")
    assert 0.5 <= gn / float(torch.cat([g.reshape(-1) for g in G.values()]).norm()) <= 2.0
    net.eval()


# ------------------------------------------------------------------------------------------------ 3. the shipped width
SPRING = dict(timesteps=4, schedule="before_t1_only", additional_interpolation_steps=0, additional_interpolation_steps_factor=0,
              interpolate_before_t1=True, time_encoding="dynamics", forward_conditioning="data", lambda_reconstruction=1.0,
              lambda_reconstruction2=0.5, loss_function="l1", enable_interpolator_dropout=True,
              model=dict(dim=64, kernel_sizes=[9, 7, 5, 3], with_time_emb=True, dropout=0.1))


def _spring_pair(B, seeds=(7, 8), **engine_kw):
    C, Cs = 4, 1
    ks = SPRING["model"]["kernel_sizes"]
    PF = oinit.seeded_state(oinit.simple_conv_net_param_shapes(64, C + C + Cs, C, ks), seed=seeds[0], gain=0.8)
    PI = oinit.seeded_state(oinit.simple_conv_net_param_shapes(64, 2 * C + Cs, C, ks), seed=seeds[1], gain=0.8)
    g = torch.Generator().manual_seed(3 + B)
    batch = dict(xt_last=torch.randn(B, C, 10, 10, generator=g), cond=torch.randn(B, C, 10, 10, generator=g),
                 sc=torch.rand(B, Cs, 10, 10, generator=g), t=torch.arange(B) % 4)
    return PF, PI, batch, _pair(PF, PI, SPRING, max_batch=B, **engine_kw)


@pytest.mark.parametrize("B", [4, 64])
def test_step_at_dim64_on_the_spring_mesh_grid(B):
    """model/cnn_simple.yaml's width and kernel sizes on the 10 x 10 grid, both loss terms.  The 64 -> 64 convs and the head's weight
    gradient run on the fp32 matrix-core kernel (train_gemm.hip notes its weight-gradient launches in the form log: 3 + 1 per
    forecaster backward); the first layer (cin = 9, 729 sums per output channel) takes the plain tiled weight-gradient kernel."""
    PF, PI, batch, m = _spring_pair(B)
    m._ensure_engine((10, 10), B)
    eng = m._engine
    eng.form_log(True)
    seed = 4242
    losses, got = _plosses(m, batch, seed)
    forms = eng.form_log_read()
    eng.form_log(False)
    want_losses, want, stats = _ref_plosses(PF, PI, SPRING, batch, seed)
    _check_step(f"dim 64, B = {B}", losses, want_losses, got, want, m.model.state_dict(), stats)
    print(sorted((k, v) for k, v in forms.items() if "wgrad" in k))
    assert sum(forms.get("t_gemm_mfma<wgrad>:atomic", {}).values()) == 8
    assert sum(forms.get("t_conv_wgrad:atomic", {}).values()) == 2
    m.eval()
    eng.close()


# ------------------------------------------------------------------------------------------------ 4. recorded forward == fp32 sampling forward
def test_recorded_running_statistics_forward_equals_the_fp32_sampling_forward():
    """Two independent kernels for one function: the recorded forward on running statistics (conv + fused norm kernels of train.hip)
    and the fp32 sampling forward (`dtype="fp32"`, sc_f32_forward: one kernel per block with folded BatchNorm), on the SAME dropout
    masks -- both draw site i of forward 0 from the engine's generator after the same seed.  rel-RMS <= 1e-5."""
    z = load_npz("scn_plosses_train_a.npz")
    hp = json.loads(str(z["hp"]))
    PI = split_state(z, "I")
    net = _mirror(PI, hp["model"], 8, 1, 4)
    g = torch.Generator().manual_seed(17)
    x, c, t = torch.randn(5, 8, 10, 10, generator=g).to(DEV), torch.rand(5, 1, 10, 10, generator=g).to(DEV), torch.tensor([1., 2., 3., 1., 2.]).to(DEV)
    eng = D.HipEngine(net.engine_net_config(), net.engine_net_config(), 10, 10, max_batch=5, use_graph=False, dtype="fp32")
    eng.load_weights(L.NET_FORECASTER, net.state_dict())
    for drop in (False, True):
        eng.seed(5)
        rec = eng.train_forward(L.NET_FORECASTER, 0, x, t, c, batch_stats=False, dropout=drop)
        eng.seed(5)
        smp = eng.net_forward(L.NET_FORECASTER, x, t, c, dropout_mode=1 if drop else 0)
        err = rel_rms(rec.cpu(), smp.cpu())
        print(f"recorded vs fp32 sampling forward, dropout {drop}: rel-RMS {err:.2e}")
        assert err <= 1e-5
        if drop:  # and the masks are the host-rebuilt ones
            src = S.EngineMasks(5)
            src.begin_forward()
            ref = S.forward(S.to_dtype(PI, torch.float64), hp["model"], x.cpu(), t.cpu(), c.cpu(), dropout=src)
            assert rel_rms(rec.cpu(), ref) <= 1e-5
    eng.close()


# ------------------------------------------------------------------------------------------------ 5. deterministic mode
def test_deterministic_mode_repeats_bitwise_without_atomics():
    runs = []
    for _ in range(2):
        PF, PI, batch, m = _spring_pair(8, train_deterministic=True)
        m._ensure_engine((10, 10), 8)
        eng = m._engine
        eng.form_log(True)
        _, grads = _plosses(m, batch, 31)
        forms = eng.form_log_read()
        eng.form_log(False)
        assert forms and not [k for k in forms if k.endswith(":atomic")], sorted(forms)
        assert any(k.endswith(":det") for k in forms)
        sd = {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items() if k.endswith(("running_mean", "running_var"))}
        runs.append((grads, sd))
        m.eval()
        eng.close()
    (ga, sa), (gb, sb) = runs
    assert all(torch.equal(ga[k], gb[k]) for k in ga) and any(g.any() for g in ga.values())
    assert all(torch.equal(sa[k], sb[k]) for k in sa)


# ------------------------------------------------------------------------------------------------ 6. engine-resident AdamW
def test_engine_adamw_over_a_simple_conv_net():
    """Three steps p_losses -> backward -> step with clipping, weight decay and EMA; the engine's own gradients, exported before each
    step, drive torch.optim.AdamW + clip_grad_norm_ + the EMA rule (warm-up included) on the CPU; weights AND the EMA shadow are compared
    after every step.  Bound as tests/test_gpu_engine_adamw.py: per tensor 4 x the deviation of torch's own fp32 run from a float64 run of the same steps (here computed next to it; floored at half an ulp
    of the tensor's largest weight)."""
    z = load_npz("scn_plosses_train_a.npz")
    hp = json.loads(str(z["hp"]))
    hp["model"] = dict(hp["model"], dropout=0.0)
    PF, PI = split_state(z, "F"), split_state(z, "I")
    batch = {k: torch.from_numpy(z[k]).to(DEV) for k in ("xt_last", "cond", "sc", "t")}
    m = _pair(PF, PI, hp, max_batch=hp["B"])
    m.train()
    m._ensure_engine((10, 10), hp["B"], sync=False)
    kw = dict(lr=2e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.05)
    opt = D.EngineAdamW(m, max_grad_norm=1.0, ema_decay=0.9, **kw)
    names = [k for k, _ in m.model.named_parameters()]
    p0 = dict(m.model.named_parameters())
    shadows = {}
    for dt in (torch.float32, torch.float64):
        ps = [torch.nn.Parameter(p0[k].detach().cpu().to(dt).clone()) for k in names]
        shadows[dt] = (ps, torch.optim.AdamW(ps, foreach=False, **kw))
    # the EMA rule (LitEma, src/models/modules/ema.py): after every step shadow -= (1 - d)(shadow - p), d = optim.ema_decay_at(decay, n)
    ema = {dt: [p.detach().clone() for p in shadows[dt][0]] for dt in shadows}
    run = lambda: m.p_losses(batch["xt_last"], batch["cond"], batch["t"], static_condition=batch["sc"])
    hist = []
    for it in range(3):
        out = run()
        out["loss"].backward()
        hist.append(float(out["loss"].detach()))
        assert all(p.grad is None for p in m.model.parameters())
        grads = opt.export("grad")
        assert any(g.any() for g in grads.values())
        opt.step()
        assert not opt.last_step_skipped and opt.last_grad_norm > 1.0  # the clip is live
        for dt, (ps, ref) in shadows.items():
            for k, p in zip(names, ps):
                p.grad = grads[k].detach().cpu().to(dt).clone()
            torch.nn.utils.clip_grad_norm_(ps, 1.0, foreach=False)
            ref.step()
            d = ema_decay_at(0.9, it + 1)
            one_minus = float(np.float32(1.0) - np.float32(d)) if dt == torch.float32 else 1.0 - d
            with torch.no_grad():
                for sh, p in zip(ema[dt], ps):
                    sh.sub_(one_minus * (sh - p))
        for fam, got, ref32, ref64 in (("weight", opt.export("weight"), shadows[torch.float32][0], shadows[torch.float64][0]),
                                       ("ema", opt.export("ema"), ema[torch.float32], ema[torch.float64])):
            worst, where = 0.0, None
            for k, p32, p64 in zip(names, ref32, ref64):
                dev = max(float((p32.detach().double() - p64.detach()).abs().max()), 2.0 ** -24 * float(p64.detach().abs().max()))
                r = float((got[k].double().cpu() - p32.detach().double()).abs().max()) / dev
                if r > worst:
                    worst, where = r, k
            print(f"iteration {it + 1} {fam}: loss {hist[-1]:.6f}, grad norm {opt.last_grad_norm:.4f}, worst deviation / torch's fp32-vs-float64 "
                  f"deviation {worst:.3f} at {where}")
            assert worst <= 4.0, (it, fam, worst, where)
    hist.append(float(run()["loss"]))
    assert hist[-1] < hist[0]
    # state_dict() / pull(): the module holds the engine's weights and statistics; the EMA shadow differs and ema_scope() samples through it
    m.eval()
    sd = {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items()}
    w, shadow = opt.export("weight"), opt.export("ema")
    assert all(torch.equal(sd[k], w[k].cpu()) for k in names)
    assert any(not torch.equal(shadow[k], w[k]) for k in names)
    x0, sc = batch["cond"], batch["sc"]
    got = m.sample(x0, static_condition=sc)
    with opt.ema_scope():
        got_ema = m.sample(x0, static_condition=sc)
    again = m.sample(x0, static_condition=sc)
    assert all(torch.equal(again[k], got[k]) for k in got) and any(not torch.equal(got_ema[k], got[k]) for k in got)
    f = _pair(dict(sd, **{k: v.cpu() for k, v in shadow.items()}), PI, hp, max_batch=hp["B"])
    want_ema = f.sample(x0, static_condition=sc)
    assert all(torch.equal(got_ema[k], want_ema[k]) for k in want_ema)
    # the state survives a replaced engine (a larger batch builds a new one)
    m.train()
    run()["loss"].backward()
    before = {fam: opt.export(fam) for fam in ("weight", "grad", "exp_avg", "exp_avg_sq", "ema")}
    old = m._engine
    new = m._ensure_engine((10, 10), 2 * hp["B"], sync=False)
    assert new is not old
    run()
    after = {fam: opt.export(fam) for fam in before}
    for fam in before:
        assert all(torch.equal(before[fam][k], after[fam][k]) for k in before[fam]), fam
    opt.step()
    assert opt.step_count == 4 and not opt.last_step_skipped
    m.eval()


# ------------------------------------------------------------------------------------------------ 7. SGD
def test_sgd_steps_reduce_the_loss_and_sampling_uses_the_updated_weights():
    z = load_npz("scn_plosses_train_a.npz")
    hp = json.loads(str(z["hp"]))
    hp["model"] = dict(hp["model"], dropout=0.0)
    PF, PI = split_state(z, "F"), split_state(z, "I")
    batch = {k: torch.from_numpy(z[k]).to(DEV) for k in ("xt_last", "cond", "sc", "t")}
    m = _pair(PF, PI, hp, max_batch=hp["B"])
    before = m.sample(batch["cond"], static_condition=batch["sc"])
    m.train()
    opt = torch.optim.SGD(m.model.parameters(), lr=0.02)
    hist = []
    for _ in range(4):
        opt.zero_grad()
        out = m.p_losses(batch["xt_last"], batch["cond"], batch["t"], static_condition=batch["sc"])
        out["loss"].backward()
        opt.step()
        hist.append(float(out["loss"]))
    print("loss over 4 SGD steps:", [round(v, 5) for v in hist])
    assert hist[-1] < hist[0]
    m.eval()
    after = m.sample(batch["cond"], static_condition=batch["sc"])
    fresh = _pair({k: v.detach().cpu() for k, v in m.model.state_dict().items()}, PI, hp, max_batch=hp["B"])
    want = fresh.sample(batch["cond"], static_condition=batch["sc"])
    assert all(torch.equal(after[k], want[k]) for k in want)
    assert any(not torch.equal(after[k], before[k]) for k in before)


# ------------------------------------------------------------------------------------------------ 8. 16-bit operands
def test_16bit_training_operands_are_refused_and_the_engine_stays_usable():
    z = load_npz("scn_get_loss_a.npz")
    hp = json.loads(str(z["hp"]))
    P = split_state(z, "F")
    x, c, y = (torch.from_numpy(z[k]).to(DEV) for k in ("x", "c", "y"))
    net = _mirror(P, hp["model"], hp["n_in"], hp["n_cond"], hp["n_out"], hp["loss_function"])
    net.train_precision = 16
    net.train()
    with pytest.raises(NotImplementedError, match="SimpleConvNet"):
        net.get_loss(x, y, condition=c)
    eng = net._engine
    assert eng.train_precision == 16
    eng.train_set_precision(32)
    loss = net.get_loss(x, y, condition=c)
    loss.backward()
    assert float(loss) > 0 and all(p.grad is not None for p in net.parameters())
    net.eval()
    assert torch.isfinite(net(x, condition=c)).all()
