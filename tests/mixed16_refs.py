"""The float64 reference of ONE training convolution under `train_precision="bf16-mixed"` (dyf_train_set_precision(16);
csrc/train_halo16.hip, the t_gemm_mfma16 forms of csrc/train_gemm.hip), and the cases tests/test_gpu_train_bf16_mixed_ops.py runs it
at -- test infrastructure, no GPU.

The mode rounds the two operands of a product to bf16 (round-to-nearest-even) while it stages them and accumulates in fp32.  The
product of two bf16 values is exact in fp32 (8 + 8 significand bits), so against a model that rounds the SAME operands and then
computes in float64 the engine differs by its fp32 summation order alone, and the project's bound for fp32 kernels
(train_op_refs.TOL, 1e-5 rel-RMS per tensor) applies unchanged -- the mode itself sits 2.3e-3 from unrounded float64.

`reference(case)` is that model for a conv `Case` of tests/train_op_refs.py: tests/split3_refs.py with `terms=1, acc=torch.float64`
for a pass that rounds, plain float64 torch for one that does not.  The forward (x, w), the data gradient (dz, w) and the weight
gradient (dz, x) round each on their own, exactly when `oracle.losses.conv_operand_rules(cin, cout)` gives the pass to the 16-bit
forms; the bias gradient is a plain sum of dz.  A weight-standardised layer standardises in float64, casts to float32 -- the engine
rounds the fp32 standardised weight -- and then rounds; its weight gradient goes back through the standardisation in float64.

`mutant=` turns the reference into a deliberately wrong one, each a mistake a staging path or a dispatch rule could make;
tests/test_train_bf16_mixed_refs.py shows that the bound tells every one of them from the reference on the GPU test's own inputs.
"""
import torch

from oracle import losses
from tests import split3_refs
from tests import train_op_refs as T

MUTANTS = ("truncate", "w_unrounded", "wgrad_x_unrounded", "dgrad_uses_fwd_rule", "no_rounding")

# ------------------------------------------------------------------------------------------------------------------- the cases
# (k, stride, pad, cin, cout, ws, bias, h, w, nb, var0)
MFMA = [(cid, a) for cid, a in T.specs("conv") if cid.endswith("-mfma")]
# the shapes where the launch changes: those of tests/test_gpu_train_bf16x3_ops.py (the thresholds of csrc/train_halo16.hip
# thalo_conv3x3 / thalo_wgrad3x3 and csrc/train_gemm.hip do not depend on the mode); the marks name the forms the shape must reach
SHAPES = [
    ("1x1-128to64-11x13-nb3", (1, 1, 0, 128, 64, 0, 1, 11, 13, 3, 0), None),
    ("4x4s2-64to64-12x16-nb4", (4, 2, 1, 64, 64, 0, 1, 12, 16, 4, 0), None),       # even plane, too few tiles for the parity-class data gradient
    ("4x4s2-64to64-11x13-nb4", (4, 2, 1, 64, 64, 0, 1, 11, 13, 4, 0), None),       # odd plane: no parity classes at any size
    ("4x4s2-64to64-128x128-nb2", (4, 2, 1, 64, 64, 0, 1, 128, 128, 2, 0), ("p",)),  # 64 tiles per class: the parity-class data gradient from here
    ("3x3-64to64-32x32-nb4", (3, 1, 1, 64, 64, 0, 1, 32, 32, 4, 0), None),         # split-K forward / dgrad, pixel splits of the wgrad
    ("3x3-64to64-64x96-nb4", (3, 1, 1, 64, 64, 0, 1, 64, 96, 4, 0), ("fd", "w")),  # 192 tiles: the halo forward and dgrad from here
    ("3x3-64to64-61x93-nb4", (3, 1, 1, 64, 64, 0, 1, 61, 93, 4, 0), ("fd", "w")),  # the same tile count, ragged edges
    ("3x3-64to64-64x32-nb4", (3, 1, 1, 64, 64, 0, 1, 64, 32, 4, 0), ("w",)),       # 64 tiles: the halo weight gradient from here
    ("3x3-64to128-64x48-nb4", (3, 1, 1, 64, 128, 0, 1, 64, 48, 4, 0), ("f", "w")),  # two column blocks of the halo forward
]
SPLITK, HALO_FWD, HALO_WGRAD = SHAPES[4], SHAPES[5], SHAPES[7]
# layers where only some of the three passes take the 16-bit form: (k, pad, cin, cout) -> conv_operand_rules
MIXED_LAYERS = [(1, 0, 32, 64), (3, 1, 96, 64), (3, 1, 64, 96), (3, 1, 64, 40), (1, 0, 64, 1)]
MIXED_RULES = {(32, 64): (True, False, False), (96, 64): (True, False, False), (64, 96): (False, True, True),
               (64, 40): (False, False, True), (64, 1): (False, False, False)}
MIXED = [(f"{k}x{k}-{ci}to{co}-{h}x{w}-nb3", (k, 1, pd, ci, co, 0, 1, h, w, 3, 0)) for k, pd, ci, co in MIXED_LAYERS for h, w in T.CONV_GRIDS]
ACCUMULATE = [(3, 1, 1, 24, 40, 1, 1, 11, 13, 3, 0), (1, 1, 0, 128, 64, 0, 1, 11, 13, 3, 0), (7, 1, 3, 3, 8, 0, 1, 11, 13, 1, 0)]  # test_gpu_train_ops
FP16_BUILD = [SHAPES[0], HALO_FWD]  # one GEMM-form and one halo-form case for the fp16 build of the library


def all_cases():
    """(id, args) of every conv case of the GPU test, each once."""
    seen, out = set(), []
    for cid, a in MFMA + [(c, a) for c, a, _ in SHAPES] + MIXED + [("-".join(str(v) for v in a), a) for a in ACCUMULATE]:
        if a not in seen:
            seen.add(a)
            out.append((cid, a))
    return out


# --------------------------------------------------------------------------------------------------------------- the reference
def bf16_rne(t):
    return t.to(torch.float32).to(torch.bfloat16).to(torch.float32)


def bf16_truncate(t):
    """The low 16 bits dropped: what a staging path does that shifts instead of rounding."""
    return (t.to(torch.float32).contiguous().view(torch.int32) & -65536).view(torch.float32)


def _nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def _contract(kind, a, b, ra, rb, rnd, shape, stride, pad):
    """One of the three bilinear maps of a conv in float64: "fwd" (a = x, b = w), "dgrad" (a = dz, b = w; shape = x's) or "wgrad" (a = dz,
    b = x; shape = w's), with a rounded by `rnd` if `ra` and b if `rb`.  Where both are, the operands hold bf16 values and the pass is
    split3_refs' one-term product (its own rounding is then the identity, also on truncated values)."""
    a = rnd(a) if ra else a
    b = rnd(b) if rb else b
    if ra and rb:
        if kind == "fwd":
            return split3_refs.conv_forward(a, b, None, stride, pad, terms=1, acc=torch.float64)
        if kind == "dgrad":
            return split3_refs.conv_input_grad(shape, b, a, stride, pad, terms=1, acc=torch.float64)
        return split3_refs.conv_weight_grad(b, shape, a, stride, pad, terms=1, acc=torch.float64)
    a, b = a.double(), b.double()
    if kind == "fwd":
        return torch.nn.functional.conv2d(a, b, None, stride=stride, padding=pad)
    if kind == "dgrad":
        return torch.nn.grad.conv2d_input(shape, b, a, stride=stride, padding=pad)
    return torch.nn.grad.conv2d_weight(b, shape, a, stride=stride, padding=pad)


def standardise(w, fp32_as=None):
    """w (float64, (cout, cin, k, k)) -> the standardised weight as float64 values, biased variance, eps 1e-5.  `fp32_as` = None: in
    float64 (the reference).  The other two are the noise-floor variants of the CPU test: "engine" = the arithmetic of the engine's own
    kernel (csrc/train_resnet.inc t_ws_fwd: sums in fp64, var = E[w^2] - mean^2, mean and rstd cast to fp32, (w - mean) * rstd in fp32),
    "torch" = every step in float32, the statistics too."""
    if fp32_as == "torch":
        w = w.float()
    mean = w.mean((1, 2, 3), keepdim=True)
    if fp32_as == "engine":
        rstd = ((w * w).mean((1, 2, 3), keepdim=True) - mean * mean).clamp_min(0).add(1e-5).rsqrt()
        return ((w.float() - mean.float()) * rstd.float()).double()
    return ((w - mean) * (w.var((1, 2, 3), unbiased=False, keepdim=True) + 1e-5).rsqrt()).double()


def reference(case, grads_in=None, mutant=None, ws_fp32_as=None):
    """-> {"y", "dx", "dweight", "dbias"} in float64, NHWC / PyTorch weight layout like Case.run; parameter gradients start from
    `grads_in`.  `ws_fp32_as`: see `standardise` (the noise-floor variants of the CPU test)."""
    assert case.op == "conv" and (mutant is None or mutant in MUTANTS), (case.op, mutant)
    stride, pad, ws = case.kw["stride"], case.kw["pad"], case.kw["ws"]
    x, dz = _nchw(case.ins[0]), _nchw(case.dout)
    w = case.params[0]
    bias = case.params[1] if len(case.params) > 1 else None
    cout, cin = w.shape[0], w.shape[1]
    f16, d16, w16 = losses.conv_operand_rules(cin, cout)
    if mutant == "dgrad_uses_fwd_rule":
        d16 = f16
    if mutant == "no_rounding":
        f16 = d16 = w16 = False
    rnd = bf16_truncate if mutant == "truncate" else bf16_rne

    w_leaf = w.double().requires_grad_(True)
    w_std = standardise(w_leaf, ws_fp32_as) if ws else w_leaf
    w_exact = w_std.detach()       # what a pass with fp32 operands multiplies by
    w_f32 = w_exact.float()        # what a 16-bit pass rounds: the engine's fp32 (standardised) weight

    y = _contract("fwd", x, w_f32 if f16 else w_exact, f16, f16 and mutant != "w_unrounded", rnd, None, stride, pad)
    if bias is not None:
        y = y + bias.double()[None, :, None, None]
    dx = _contract("dgrad", dz, w_f32 if d16 else w_exact, d16, d16, rnd, x.shape, stride, pad)
    dw_std = _contract("wgrad", dz, x, w16, w16 and mutant != "wgrad_x_unrounded", rnd, w.shape, stride, pad)
    dw = torch.autograd.grad(w_std, w_leaf, dw_std)[0] if ws else dw_std
    out = {"y": _nhwc(y), "dx": _nhwc(dx), "dweight": dw + (0 if grads_in is None else grads_in[0].double())}
    if bias is not None:
        out["dbias"] = dz.double().sum((0, 2, 3)) + (0 if grads_in is None else grads_in[1].double())
    return out


def oracle_model(case):
    """The same case through `oracle.losses`'s autograd model of the mode (what `training_operand_rounding` patches into the restated
    backbones), in float32: -> the same keys."""
    from oracle import nets
    assert not case.kw["ws"]
    x = _nchw(case.ins[0]).requires_grad_(True)
    ps = [p.clone().requires_grad_(True) for p in case.params]
    with losses.training_operand_rounding():
        y = nets.conv2d(x, ps[0], ps[1] if len(ps) > 1 else None, stride=case.kw["stride"], padding=case.kw["pad"])
    grads = torch.autograd.grad(y, [x] + ps, _nchw(case.dout))
    out = {"y": _nhwc(y.detach()), "dx": _nhwc(grads[0]), "dweight": grads[1]}
    if len(ps) > 1:
        out["dbias"] = grads[2]
    return out
