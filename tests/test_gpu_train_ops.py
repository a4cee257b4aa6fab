"""-m gpu: every op the training step records for either backbone (csrc/train_resnet.inc RCtx: forward kernels and the recorded
adjoints), ONE op at a time through the training step's own launch code (dyf_op_train_f32), against float64 torch on the CPU.

The end-to-end training tests hold a gradient to 1e-3 of the GLOBAL gradient norm at toy sizes; here every output and every gradient
is held on its own, at the shapes where the launch geometry changes: LinearAttention across the 32-pixel chunks (a last chunk of one
pixel: 33, 225, 257, 545) and the 256-pixel splits (257, 545); Attention at OISST's 225 tokens; GroupNorm / LayerNorm at channel
counts that do not divide 256 (24: straddling channel quads, the LayerNorm-gain fallback kernel) and that reach or pass it (256, 512);
the convs of every layer kind on an odd and an even grid.  Cases and references: tests/train_op_refs.py; that the bound tells a
dropped pixel or term from the reference: tests/test_train_op_refs.py.

Bound: rel-RMS <= 1e-5 per compared tensor (the project's bound for fp32 kernels), outputs finite.  fp32 torch.autograd on the same
inputs sits at 6e-8 .. 5e-7 against float64: every test prints its worst tensor next to that baseline.  Dropout masks come from the
engine's generator and are rebuilt on the host (tests/rng_host.py).

A tensor whose float64 value is zero is compared absolutely against 1e-5 x the RMS of the op's other gradients.  Zero means zero to
the reference's own precision: an RMS below 1e-12 of that of the other gradients (float64 rounding leaves 1e-17 where the exact
value is 0; seven orders below what the absolute bound resolves).  The listed cases that have one, all of them degenerate single-
pixel shapes: dq and dk of LinearAttention at hw = 1 (the k-softmax over one pixel is 1, so the context is v for every d and the
output does not depend on q), dq and dk of Attention at N = 1 (a softmax over one key is constant), dz and dgamma of GroupNorm at
C = 8, hw = 1 (groups of ONE element: xhat = 0).  The last one found the normalisation backward keeping an fma's rounding residue
times rstd = 316 (2e-5 of dy instead of 0): t_norm_bwd_apply now rounds gamma * dbn as the group sums round it.

unet_simple's ops (norm_act, up2_bilinear, resize, convt) run at the shapes where their launches change: BatchNorm on batch and on running
statistics and GroupNorm(8) at 8 / 24 / 64 channels on 1 x 1, 3 x 5 and 15 x 15 planes (BatchNorm over ONE value, nb = 1 at 1 x 1, has
xhat = 0: dz and dgamma are zero as above) and on one 65 x 65 plane, where a workgroup of the sum kernels takes 17 pixels; the updated
running statistics are compared like a gradient.  An injected keep mask is the sampling path's dropout: those cases run the forward alone;
dropout from the generator, with its gradients, has a case per kind.  The x2 upsample runs with one source and with the two that stand
for a concatenation, also onto a gradient the second source already has; the readout also at 4096 pixels, where the step's small-channel
matrix-core forms take its two weight-side products.
"""
import pytest
import torch

import dyffusion_amd as D
from tests import train_op_refs as T
from tests.gpu_common import DEV
from tests.helpers import rel_rms

pytestmark = pytest.mark.gpu
ZERO = 1e-12  # a float64 gradient this far below the op's other gradients is rounding noise around an exact 0


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False)
    e.train_set_precision(32)  # fp32 conv operands (the 16-bit operand model has its own tests)
    e.set_row_offset(T.ROW_OFFSET)
    yield e
    e.close()


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def check(eng, op, args, cid, accumulate=False):
    case = T.build(op, args)
    keep = T.engine_keep(case)
    g = torch.Generator().manual_seed(11)
    gin = [torch.randn(p.shape, generator=g) for p in case.params] if accumulate else None
    want = case.run(keep=keep, grads_in=gin)
    base = case.run(torch.float32, keep=keep, grads_in=gin)
    if case.p > 0.0:
        eng.seed(T.SEED)  # the forward counter restarts: the op draws the masks of forward 0, site 0
    extra = {}
    if case.mask is not None:
        extra["mask"] = case.mask.to(DEV)
    if case.skip_grad is not None:
        extra["skip_grad"] = case.skip_grad.to(DEV)
    r = eng.op_train(case.op, [t.to(DEV) for t in case.ins], case.params, case.dout.to(DEV), gin, **case.kw, **extra)
    got = {"y": r["y"].cpu()}
    if case.mask is None:  # (an injected mask: the forward alone ran)
        got.update({"d" + n: t.cpu() for n, t in zip(case.in_names, r["dinputs"]) if t is not None})
        got.update({"d" + n: t for n, t in zip(case.p_names, r["dparams"])})
    if case.stats is not None:  # the running statistics as the forward left them
        got.update(zip(("running_mean", "running_var"), r["dparams"][len(case.p_names):]))
    if case.split_qkv:
        d = got.pop("dx")
        got.update(dq=d[..., :128], dk=d[..., 128:256], dv=d[..., 256:])
    assert sorted(got) == sorted(want)
    errs, fp32 = {}, {}
    for k, w in want.items():
        assert bool(torch.isfinite(got[k]).all()), k
        others = [v.reshape(-1) for n, v in want.items() if n != k and n.startswith("d")]
        if others and rms(w) <= ZERO * rms(torch.cat(others)):  # zero in float64: absolute, against the op's other gradients
            errs[k] = float(got[k].abs().max()) / rms(torch.cat(others))
            fp32[k] = float(base[k].abs().max()) / rms(torch.cat(others))
            print(f"train-op {case.op} {cid}: {k} is zero in float64")
        else:
            errs[k], fp32[k] = rel_rms(got[k].reshape(w.shape), w), rel_rms(base[k], w)
    worst = max(errs, key=errs.get)
    print(f"train-op {case.op} {cid}: max err {errs[worst]:.3e} ({worst}); fp32 torch {max(fp32.values()):.3e}")
    assert errs[worst] <= T.TOL, errs
    return errs


def cases(op):
    return [pytest.param(args, id=cid) for cid, args in T.specs(op)]


@pytest.mark.parametrize("args", cases("linattn"))
def test_linattn(eng, args, request):
    check(eng, "linattn", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("attention"))
def test_attention(eng, args, request):
    check(eng, "attention", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("gn_act"))
def test_gn_act(eng, args, request):
    check(eng, "gn_act", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("layernorm"))
def test_layernorm(eng, args, request):
    check(eng, "layernorm", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("conv"))
def test_conv(eng, args, request):
    k, s, pd, ci, co, ws, bias, h, w, nb, _ = args
    took = [eng.train_conv_check(kind, nb, h, w, ci, co, k, s, pd)[2] for kind in (0, 1, 2)]
    print(f"conv {request.node.callspec.id}: matrix-core form took forward / dgrad / wgrad: {took}")
    assert took[0] == request.node.callspec.id.endswith("-mfma")
    check(eng, "conv", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("linear"))
def test_linear(eng, args, request):
    check(eng, "linear", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("small"))
def test_small_ops(eng, args, request):
    check(eng, "small", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("norm_act"))
def test_norm_act(eng, args, request):
    check(eng, "norm_act", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("up2_bilinear"))
def test_up2_bilinear(eng, args, request):
    errs = check(eng, "up2_bilinear", args, request.node.callspec.id)
    assert ("dx2" in errs) == (args[3] > 0)  # both source gradients were compared


@pytest.mark.parametrize("args", cases("resize"))
def test_resize(eng, args, request):
    check(eng, "resize", args, request.node.callspec.id)


@pytest.mark.parametrize("args", cases("convt"))
def test_conv_transpose4s2(eng, args, request):
    check(eng, "convt", args, request.node.callspec.id)


ACCUMULATE = [("conv", (3, 1, 1, 24, 40, 1, 1, 11, 13, 3, 0)), ("conv", (1, 1, 0, 128, 64, 0, 1, 11, 13, 3, 0)), ("conv", (7, 1, 3, 3, 8, 0, 1, 11, 13, 1, 0)),
              ("gn_act", (24, 35, 3, 1, 0.2)), ("layernorm", (24, 33, 3, 0.1)), ("layernorm", (64, 33, 3, 0.0)), ("linear", (5, 17, 6, 1)),
              ("small", ("learned_sinu", 5)), ("norm_act", ("bn_batch", 24, 3, 5, 3, 1, 0.1, "relu", "gen")),
              ("norm_act", ("bn_running", 24, 15, 15, 3, 1, 0.0, "leaky", "mask")), ("norm_act", ("gn8", 64, 3, 5, 3, 0, 0.0, "relu", "mask")),
              ("convt", (64, 3, 11, 13, 3)), ("convt", (8, 1, 4, 4, 1))]


@pytest.mark.parametrize("op,args", ACCUMULATE, ids=[f"{op}-{'-'.join(str(a) for a in args)}" for op, args in ACCUMULATE])
def test_parameter_gradients_accumulate(eng, op, args, request):
    """The gradient buffers hold random values when the op runs: the result is incoming + gradient (the two forecaster passes of a step
    meet this way); a kernel that assigned would lose the incoming part."""
    check(eng, op, args, request.node.callspec.id, accumulate=True)


def test_what_the_seam_cannot_express_is_refused(eng):
    x = torch.zeros(1, 2, 2, 8, device=DEV)
    with pytest.raises(ValueError):
        eng.op_train("gn_act", [x], [torch.ones(8), torch.zeros(8)], x, groups=3)       # groups must divide C
    with pytest.raises(ValueError):
        eng.op_train("gelu", [x], [], x, p=0.5)                                         # no dropout in a GELU
    with pytest.raises(ValueError):
        eng.op_train("dropout", [torch.zeros(9, 2, 2, 8, device=DEV)], [], torch.zeros(9, 2, 2, 8, device=DEV), p=0.5)  # 9 rows > 2 max_batch
    with pytest.raises(NotImplementedError):
        q = torch.zeros(1, 1, 4097, 384, device=DEV)
        eng.op_train("attention", [q], [], torch.zeros(1, 1, 4097, 128, device=DEV))   # keeps its probabilities: <= 4096 tokens
