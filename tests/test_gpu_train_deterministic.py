"""-m gpu: the deterministic training mode (dyf_train_set_deterministic; `train_deterministic=True`, the reference's
`trainer.deterministic`).  With it no floating-point sum of a recorded forward, of its backward or of the criterion is merged with
atomics: every cross-workgroup sum goes through slabs of the split-K workspace and a fixed-order second launch, the adjoint of the outer
resample is a gather (csrc/train.hip, train_gemm.hip, train_halo16.hip, kernels.hip).

What is held:
  * every recorded op, one at a time on the cases of tests/test_gpu_train_ops.py: three runs on identical inputs are bitwise equal, and
    the first holds that file's own bound (rel-RMS <= 1e-5 against float64, its zero rule) -- `check` is imported, not restated;
  * the shapes at which each merged sum has many contributors (SPLIT_* below), under fp32 and bf16-mixed operands, with the form log
    showing a `:det` launch and no `:atomic` one -- equal bits alone cannot show that no order-dependent launch ran;
  * whole steps of both fixture networks with dropout on, both precisions: two freshly built models give equal losses, gradients, running
    statistics, and three resident AdamW iterations give bitwise equal weights / moments / EMA; the step's form log has no `:atomic` name,
    and the same step with the mode off has one (the note is live);
  * the gradients of the two modes agree within the end-to-end bound of tests/test_gpu_training*.py (1e-3 of the gradient norm per
    tensor): both are sums of the same terms;
  * `train_deterministic=None` follows torch.use_deterministic_algorithms, and the host glue of a step runs under that flag;
  * the switch round-trips, and fp32 sampling is bit-equal with the mode on and off.

The 16-bit halo weight gradient (t_wgrad3x3_16) admits a layer from 64 tiles of 8 x 16 pixels: 3 x 3 / 64 -> 64 on 32 x 32 with 4 rows
has 32, so under bf16-mixed operands that shape runs t_gemm_mfma16<wgrad>; the smallest shape the halo form accepts at 4 rows, 64 x 32
(64 tiles), is in the list next to it.
"""
import pytest
import torch

import dyffusion_amd as D
from tests import train_op_refs as T
from tests.gpu_common import DEV, build_dyffusion, seeded_pair
from tests.test_gpu_engine_adamw import _attach, _build
from tests.test_gpu_train_ops import ACCUMULATE, check

pytestmark = pytest.mark.gpu
OPS = ("conv", "convt", "linear", "small", "gn_act", "norm_act", "layernorm", "resize", "up2_bilinear", "linattn", "attention")
GRAD_BOUND = 1e-3  # tests/test_gpu_training.py, test_gpu_training_resnet.py: per-tensor |difference| / norm of the whole gradient


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False, train_deterministic=True)
    e.train_set_precision(32)
    e.set_row_offset(T.ROW_OFFSET)
    yield e
    e.close()


class Recorded:
    """The engine with every op_train call and its result kept, so that `check` (tests/test_gpu_train_ops.py) runs unchanged and the
    same call can be repeated."""

    def __init__(self, eng):
        self._eng, self.calls = eng, []

    def __getattr__(self, name):
        return getattr(self._eng, name)

    def op_train(self, *a, **kw):
        r = self._eng.op_train(*a, **kw)
        self.calls.append((a, kw, r))
        return r


def flat(r):
    """Every tensor an op_train call returned, in a fixed order."""
    return [r["y"]] + [t for t in (r["dinputs"] or []) if t is not None] + list(r["dparams"] or [])


def assert_same(a, b, what):
    fa, fb = flat(a), flat(b)
    assert len(fa) == len(fb)
    for i, (x, y) in enumerate(zip(fa, fb)):
        assert torch.equal(x.cpu(), y.cpu()), f"{what}: returned tensor {i} differs between identical runs"


def three_runs(eng, op, args, cid, accumulate=False, bound=True):
    """`check` once (bound=False: the call alone, no reference), then the same call twice more; all results bitwise equal."""
    rec = Recorded(eng)
    if bound:
        check(rec, op, args, cid, accumulate)
    else:
        case = T.build(op, args)
        eng.seed(T.SEED)
        rec.op_train(case.op, [t.to(DEV) for t in case.ins], case.params, case.dout.to(DEV), None, **case.kw)
    (a, kw, first), = rec.calls
    for run in (2, 3):
        eng.seed(T.SEED)  # a case that draws dropout draws forward 0 again
        assert_same(first, eng.op_train(*a, **kw), f"{op} {cid} run {run}")
    return first


def logged(eng, fn):
    eng.form_log(True)
    try:
        out = fn()
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    return out, forms


def det_only(forms, what):
    names = sorted(forms)
    print(f"{what}: forms {names}")
    assert any(k.endswith(":det") for k in names), (what, names)
    assert not any(k.endswith(":atomic") for k in names), (what, names)


# ---------------------------------------------------------------------------------------------- 1. every op, one at a time
ALL_CASES = [pytest.param(op, args, False, id=f"{op}-{cid}") for op in OPS for cid, args in T.specs(op)] + \
            [pytest.param(op, args, True, id=f"accumulate-{op}-{'-'.join(str(a) for a in args)}") for op, args in ACCUMULATE]


@pytest.mark.parametrize("op,args,accumulate", ALL_CASES)
def test_every_op_is_repeatable_and_holds_the_fp32_bound(eng, op, args, accumulate, request):
    assert eng.train_deterministic is True
    three_runs(eng, op, args, request.node.callspec.id, accumulate)


# ---------------------------------------------------------------------------------------------- 2. many contributors per sum
# (k, stride, pad, cin, cout, ws, bias, h, w, nb, var0) of tests/train_op_refs.py
SPLIT_CONVS = [
    ("3x3-64to64-32x32-nb4", (3, 1, 1, 64, 64, 0, 1, 32, 32, 4, 0)),     # t_gemm_mfma<wgrad> at 16 pixel splits (bf16-mixed: t_gemm_mfma16)
    ("3x3-64to64-64x32-nb4", (3, 1, 1, 64, 64, 0, 1, 64, 32, 4, 0)),     # 64 tiles: bf16-mixed takes t_wgrad3x3_16
    ("3x3-3to64-64x64-nb1", (3, 1, 1, 3, 64, 0, 1, 64, 64, 1, 0)),       # the small-channel matrix-core forward and wgrad
    ("4x4s2-3to64-128x128-nb1", (4, 2, 1, 3, 64, 0, 1, 128, 128, 1, 0)),
    ("3x3-24to40-bias-33x33-nb2", (3, 1, 1, 24, 40, 0, 1, 33, 33, 2, 0)),  # the tiled VALU wgrad and the any-channel-count bias sum
    ("1x1-64to3-64x64-nb1", (1, 1, 0, 64, 3, 0, 1, 64, 64, 1, 0)),
]
SPLIT_OTHER = [
    ("layernorm-C64-hw545-nb3", "layernorm", (64, 545, 3, 0.0)),
    ("bn_batch-C64-65x65-nb2", "norm_act", ("bn_batch", 64, 65, 65, 2, 0, 0.0, "relu", "mask")),
]


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("cid,args", SPLIT_CONVS, ids=[c for c, _ in SPLIT_CONVS])
def test_split_conv_shapes_run_deterministic_forms_only(eng, cid, args, precision):
    eng.train_set_precision(precision)
    try:
        # the float64 bound is fp32's: bf16-mixed operands are held to repeatability alone
        _, forms = logged(eng, lambda: three_runs(eng, "conv", args, f"{cid}-{precision}", bound=precision == 32))
    finally:
        eng.train_set_precision(32)
    det_only(forms, f"conv {cid} operands {precision}")
    if precision == 16 and cid == "3x3-64to64-64x32-nb4":
        assert "t_wgrad3x3_16:det" in forms, sorted(forms)


@pytest.mark.parametrize("cid,op,args", SPLIT_OTHER, ids=[c for c, _, _ in SPLIT_OTHER])
def test_split_norm_shapes_run_deterministic_forms_only(eng, cid, op, args):
    _, forms = logged(eng, lambda: three_runs(eng, op, args, cid))
    det_only(forms, cid)


@pytest.mark.parametrize("kind", ["l1", "mse", "smoothl1"])
def test_criterion_returns_the_identical_double(eng, kind):
    g = torch.Generator().manual_seed(5)
    a, b = (torch.randn(2, 3, 33, 33, generator=g) * 1.5).to(DEV), torch.randn(2, 3, 33, 33, generator=g).to(DEV)
    assert a.numel() % 4 != 0
    vals, forms = logged(eng, lambda: [eng.criterion(a, b, kind) for _ in range(3)])
    det_only(forms, f"criterion {kind}")
    assert vals[0] == vals[1] == vals[2], vals
    d = (a.double() - b.double()).cpu()
    want = float(d.abs().mean() if kind == "l1" else d.pow(2).mean() if kind == "mse" else
                 torch.where(d.abs() < 1, 0.5 * d * d, d.abs() - 0.5).mean())
    assert vals[0] == pytest.approx(want, rel=1e-6)  # fp32 terms, float64 sums


# ---------------------------------------------------------------------------------------------- 3. whole steps
def fresh(tag, mode, precision, seed=4242):
    m, batch = _build(tag, dropout=True)
    m._engine_opts["train_precision"] = precision
    m.train_set_deterministic(mode)
    m.seed(seed)
    m.train()
    return m, batch


def one_step(tag, mode, precision):
    """p_losses + backward of a freshly built model -> (losses, gradients, running statistics, form log of the step)."""
    m, batch = fresh(tag, mode, precision)
    eng = m._ensure_engine(batch["condition"].shape[-2:], batch["condition"].shape[0], sync=False)
    assert eng.train_deterministic is bool(mode) and eng.train_precision == precision

    def step():
        out = m.p_losses(**batch)
        out["loss"].backward()
        return out

    out, forms = logged(eng, step)
    losses = {k: float(v) for k, v in out.items() if isinstance(v, (int, float)) or (torch.is_tensor(v) and v.numel() == 1)}
    grads = {k: p.grad.detach().cpu().clone() for k, p in m.model.named_parameters()}
    stats = {k: v.detach().cpu().clone() for k, v in m.model.state_dict().items() if "running_" in k}
    m.eval()
    return losses, grads, stats, forms


_STEPS = {}


def step_once(tag, mode, precision):
    key = (tag, mode, precision)
    if key not in _STEPS:
        _STEPS[key] = one_step(tag, mode, precision)
    return _STEPS[key]


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_two_fresh_models_take_the_same_step(tag, precision):
    la, ga, sa, forms = step_once(tag, True, precision)
    lb, gb, sb, _ = one_step(tag, True, precision)
    assert la == lb and len(la) >= 1, (la, lb)
    assert sorted(ga) == sorted(gb) and all(torch.equal(ga[k], gb[k]) for k in ga), [k for k in ga if not torch.equal(ga[k], gb[k])]
    assert any(g.any() for g in ga.values())
    if tag == "simple":
        assert sa and all(torch.equal(sa[k], sb[k]) for k in sa)
    det_only(forms, f"{tag} step, operands {precision}, mode on")
    _, _, _, off = step_once(tag, False, precision)
    print(f"{tag} step, operands {precision}, mode off: forms {sorted(off)}")
    assert any(k.endswith(":atomic") for k in off) and not any(k.endswith(":det") for k in off), sorted(off)


@pytest.mark.parametrize("precision", [32, 16])
@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_three_resident_iterations_are_bitwise_equal(tag, precision):
    def run():
        m, batch = fresh(tag, True, precision)
        opt = _attach(m, batch)
        norms = []
        for _ in range(3):
            m.p_losses(**batch)["loss"].backward()
            opt.step()
            norms.append(opt.last_grad_norm)
        out = {fam: opt.export(fam) for fam in ("weight", "exp_avg", "exp_avg_sq", "ema")}
        m.eval()
        return out, norms

    a, na = run()
    b, nb = run()
    assert na == nb, (na, nb)
    for fam in a:
        assert all(torch.equal(a[fam][k], b[fam][k]) for k in a[fam]), (fam, [k for k in a[fam] if not torch.equal(a[fam][k], b[fam][k])])


def _dim64_resnet_step():
    from tests.test_gpu_training_resnet import _mirror
    from tests.test_gpu_unet_resnet import seeded_unet
    mk = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0)
    PF, PI = seeded_unet(64, (1, 2), 2, 1, seed=91), seeded_unet(64, (1, 2), 2, 1, seed=92)
    m = D.DYffusion(_mirror(PF, mk, 1, 1, 1), D.InterpolatorHandle(_mirror(PI, mk, 2, 0, 1), 4), timesteps=4, max_batch=3,
                    forward_conditioning="data", schedule="before_t1_only", interpolate_before_t1=True, time_encoding="dynamics",
                    lambda_reconstruction=1.0, lambda_reconstruction2=0.5, loss_function="l1", train_deterministic=True)
    g = torch.Generator().manual_seed(17)
    xt_last, cond, t = torch.randn(3, 1, 16, 16, generator=g), torch.randn(3, 1, 16, 16, generator=g), torch.tensor([0, 2, 3])
    m.seed(7)
    m.train()
    eng = m._ensure_engine((16, 16), 3, sync=False)

    def step():
        out = m.p_losses(xt_last.to(DEV), cond.to(DEV), t.to(DEV), static_condition=None)
        out["loss"].backward()
        return float(out["loss"])

    loss, forms = logged(eng, step)
    grads = {k: p.grad.detach().cpu().clone() for k, p in m.model.named_parameters()}
    m.eval()
    return loss, grads, forms


def test_dim64_resnet_step_pair_on_the_matrix_core_forms():
    la, ga, forms = _dim64_resnet_step()
    lb, gb, _ = _dim64_resnet_step()
    det_only(forms, "dim-64 ResNet-UNet step")
    assert "t_gemm_mfma<wgrad>:det" in forms, sorted(forms)
    assert la == lb and all(torch.equal(ga[k], gb[k]) for k in ga)


# ---------------------------------------------------------------------------------------------- 4. parity with the default mode
@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_gradients_of_both_modes_agree_within_the_end_to_end_bound(tag):
    _, on, _, _ = step_once(tag, True, 32)
    _, off, _, _ = step_once(tag, False, 32)
    gn = float(torch.cat([v.reshape(-1) for v in off.values()]).norm())
    errs = {k: float((on[k] - off[k]).norm()) / gn for k in off}
    worst = max(errs, key=errs.get)
    print(f"{tag}: mode on vs off, worst per-tensor |difference| / gradient norm {errs[worst]:.2e} ({worst})")
    assert gn > 0 and errs[worst] <= GRAD_BOUND, errs[worst]


# ---------------------------------------------------------------------------------------------- 5. following torch
@pytest.mark.parametrize("tag", ["simple", "resnet"])
def test_none_follows_torch_and_the_host_glue_runs_under_the_flag(tag):
    _, want, _, _ = step_once(tag, True, 32)
    before = torch.are_deterministic_algorithms_enabled()
    torch.use_deterministic_algorithms(True)
    try:
        m, batch = fresh(tag, None, 32)
        out = m.p_losses(**batch)
        out["loss"].backward()
        assert m._engine.train_deterministic is True
        got = {k: p.grad.detach().cpu().clone() for k, p in m.model.named_parameters()}
        m.eval()
    finally:
        torch.use_deterministic_algorithms(before)
    assert all(torch.equal(got[k], want[k]) for k in want), [k for k in want if not torch.equal(got[k], want[k])]
    assert m._engine.train_deterministic is before  # and back with the flag


# ---------------------------------------------------------------------------------------------- 6. the switch
def test_switch_round_trip_and_the_default_forms_come_back(eng):
    args = SPLIT_CONVS[0][1]
    case = T.build("conv", args)

    def run():
        return eng.op_train(case.op, [t.to(DEV) for t in case.ins], case.params, case.dout.to(DEV), None, **case.kw)

    try:
        eng.train_set_deterministic(False)
        assert eng.train_deterministic is False
        _, off = logged(eng, run)
        eng.train_set_deterministic(True)
        assert eng.train_deterministic is True
        _, on = logged(eng, run)
    finally:
        eng.train_set_deterministic(True)
    print(f"mode off: {sorted(off)}; mode on: {sorted(on)}")
    assert "t_gemm_mfma<wgrad>:atomic" in off and not any(k.endswith(":det") for k in off)
    det_only(on, "mode on again")
    with pytest.raises(ValueError):
        eng.train_set_deterministic(1)


def test_fp32_sampling_does_not_read_the_mode():
    hp = dict(timesteps=4, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only", sampling_type="cold",
              refine_intermediate_predictions=True, enable_interpolator_dropout=False, num_input_channels=3)
    mk = dict(dim=64, upsample_dims=[64, 64], outer_sample_mode="bilinear", with_time_emb=True, dropout=0.15)
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(0)
    x0, c = torch.randn(3, 3, 23, 11, generator=g).to(DEV), torch.rand(3, 2, 23, 11, generator=g).to(DEV)
    m = build_dyffusion(PF, PI, mk, 3, 2, hp, max_batch=3, use_graph=False, dtype="fp32", train_deterministic=False)
    off = m.sample(x0, static_condition=c)
    m.train_set_deterministic(True)
    assert m._engine.train_deterministic is True
    on = m.sample(x0, static_condition=c)
    assert sorted(on) == sorted(off) and all(torch.equal(on[k], off[k]) for k in off)
