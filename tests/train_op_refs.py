"""Plain references of the ops the training step records for either backbone (dyffusion_amd/csrc/train_resnet.inc RCtx), and the cases
tests/test_gpu_train_ops.py runs them at -- test infrastructure, no GPU.

Every op is a pure torch function of a few lines, NHWC in and out like the engine's op seam (HipEngine.op_train); it computes in the
dtype of its arguments (float64 for the reference, float32 for the "what does fp32 arithmetic cost" baseline) and its gradients come
from torch.autograd.  A dropout keep mask is an argument (the tests rebuild the engine's masks with tests/rng_host.py).

`mutant=` turns a reference into a deliberately wrong one -- each is a mistake a kernel of this step could make -- so that
tests/test_train_op_refs.py can show that the bound of the GPU test tells right from wrong on the GPU test's own inputs.
"""
import math

import numpy as np
import torch

from tests import rng_host

TOL = 1e-5  # rel-RMS per compared tensor: the project's bound for fp32 kernels (tests/test_gpu_fp32_attention_stream.py TOL_CORE)
HEADS, DH, HID = 4, 32, 128
SEED, ROW_OFFSET = 20261018, 5  # the engine generator's seed and the global index of batch row 0 in the dropout cases


# ----------------------------------------------------------------------------------------------------------------- the ops
def conv(x, w, b=None, stride=1, pad=0, ws=False, mutant=None):
    """nn.Conv2d / WeightStandardizedConv2d as a sum over taps: x (nb,h,w,ci), w (co,ci,k,k) -> (nb,ho,wo,co)."""
    if ws:
        mean, var = w.mean((1, 2, 3), keepdim=True), w.var((1, 2, 3), unbiased=mutant == "unbiased", keepdim=True)
        w = (w - mean) * (var + 1e-5).rsqrt()
    nb, h, wd, ci = x.shape
    k = w.shape[2]
    ho, wo = (h + 2 * pad - k) // stride + 1, (wd + 2 * pad - k) // stride + 1
    xp = torch.zeros(nb, h + 2 * pad, wd + 2 * pad, ci, dtype=x.dtype)
    xp[:, pad:pad + h, pad:pad + wd] = x
    y = 0
    for ky in range(k):
        for kx in range(k):
            y = y + xp[:, ky:ky + stride * (ho - 1) + 1:stride, kx:kx + stride * (wo - 1) + 1:stride] @ w[:, :, ky, kx].T
    return y if b is None else y + b


def gn_act(z, gamma, beta, groups, ss=None, keep=None, p=0.0, mutant=None):
    """GroupNorm (biased variance, eps 1e-5) + FiLM (ss (nb,2C) = scale | shift) + SiLU + Dropout: z (nb,h,w,C)."""
    nb, h, w, C = z.shape
    cpg = C // groups
    zg = z.reshape(nb, h * w, groups, cpg)
    mean, var = zg.mean((1, 3)), zg.var((1, 3), unbiased=mutant == "unbiased")
    c = torch.arange(C)
    idx = (c // 4 * 4 if mutant == "quad_group" else c) // cpg  # the group of a channel (mutant: of the first channel of its quad)
    v = (z - mean[:, None, None, idx]) * (var + 1e-5).rsqrt()[:, None, None, idx] * gamma + beta
    if ss is not None:
        v = v * (1 + ss[:, None, None, :C]) + ss[:, None, None, C:]
    y = v * torch.sigmoid(v)
    return y if keep is None else y * keep * (1.0 / (1.0 - p))


def layernorm(x, g, keep=None, p=0.0, mutant=None):
    """unet.LayerNorm over the channels of a pixel (biased variance, gain only, eps 1e-5) + Dropout: x (nb,h,w,C), g (1,C,1,1)."""
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=mutant == "unbiased", keepdim=True)
    y = (x - mean) * (var + 1e-5).rsqrt() * g.reshape(-1)
    return y if keep is None else y * keep * (1.0 / (1.0 - p))


def _heads(qkv):
    nb, h, w, _ = qkv.shape
    return (qkv[..., i * HID:(i + 1) * HID].reshape(nb, h * w, HEADS, DH) for i in range(3))


def linattn(qkv, mutant=None):
    """LinearAttention core: softmax_d(q) / sqrt(32) . (softmax_pixels(k)^T (v / hw)): qkv (nb,h,w,384) -> (nb,h,w,128)."""
    nb, h, w, _ = qkv.shape
    hw = h * w
    q, k, v = _heads(qkv)
    if mutant == "kstat_last_pixel" and hw > 1:  # the statistics of the k-softmax miss the last pixel
        m = k[:, :-1].amax(1, keepdim=True)
        sk = (k - m).exp() / (k[:, :-1] - m).exp().sum(1, keepdim=True)
    else:
        sk = k.softmax(1)
    if mutant != "v_not_over_hw":
        v = v / hw
    if mutant == "second_split":  # pixels 256..511 never reach the context
        sk = torch.cat([sk[:, :256], 0 * sk[:, 256:512], sk[:, 512:]], 1)
    ctx = torch.einsum("bphd,bphe->bhde", sk, v)
    return torch.einsum("bhde,bphd->bphe", ctx, q.softmax(-1) * DH ** -0.5).reshape(nb, h, w, HID)


def attention(qkv, keep=None, p=0.0):
    """Attention core: softmax_j(q_i . k_j / sqrt(32)), Dropout on the probabilities (keep (nb,4,N,N)), times v."""
    nb, h, w, _ = qkv.shape
    q, k, v = _heads(qkv)
    pr = (torch.einsum("bihd,bjhd->bhij", q, k) * DH ** -0.5).softmax(-1)
    if keep is not None:
        pr = pr * keep * (1.0 / (1.0 - p))
    return torch.einsum("bhij,bjhd->bihd", pr, v).reshape(nb, h, w, HID)


def linear(x, w, b, pre=False):
    return (x * torch.sigmoid(x) if pre else x) @ w.T + b


def learned_sinu(t, w):
    fr = t[:, None] * w[None, :] * (2 * math.pi)
    return torch.cat([t[:, None], fr.sin(), fr.cos()], -1)


def dropout(x, keep=None, p=0.0):
    return x if keep is None else x * keep * (1.0 / (1.0 - p))


def gelu(x):
    return 0.5 * x * (1 + torch.erf(x * 2 ** -0.5))


def up2_nearest(x):
    return x.repeat_interleave(2, 1).repeat_interleave(2, 2)


# ---- unet_simple's ops (unet_simple.py:13-82, 164-197)
def _act(v, act):
    return v * torch.sigmoid(v) if act == "silu" else torch.where(v > 0, v, 0.2 * v) if act == "leaky" else v.clamp_min(0)


def norm_act(z, gamma, beta, rmean=None, rvar=None, groups=0, running=False, act="leaky", ss=None, keep=None, p=0.0, mutant=None):
    """UNetBlock after its conv: BatchNorm2d (batch statistics, or `running`) or GroupNorm(groups), biased variance, eps 1e-5 -> FiLM ->
    activation -> Dropout: z (nb,h,w,C)."""
    nb, h, w, C = z.shape
    if groups:
        zg = z.reshape(nb, h * w, groups, C // groups)
        idx = torch.arange(C) // (C // groups)
        mean, var = zg.mean((1, 3))[:, None, None, idx], zg.var((1, 3), unbiased=False)[:, None, None, idx]
    elif running:
        mean, var = rmean, rvar
    elif mutant == "per_sample_count":  # the batch's 1 / (nb hw) taken per sample: every sample normalised by its own statistics
        mean, var = z.mean((1, 2), keepdim=True), z.var((1, 2), unbiased=False, keepdim=True)
    else:
        mean, var = z.mean((0, 1, 2)), z.var((0, 1, 2), unbiased=False)
    v = (z - mean) * (var + 1e-5).rsqrt() * gamma + beta
    if ss is not None:
        v = v * (1 + ss[:, None, None, :C]) + ss[:, None, None, C:]
    y = _act(v, act)
    return y if keep is None else y * keep * (1.0 / (1.0 - p))


def bn_running_update(z, rmean, rvar, mutant=None):
    """What a training-mode BatchNorm2d(momentum=0.1) forward leaves in its buffers: the batch mean and the UNBIASED batch variance (one
    value per channel has none: the biased one, 0)."""
    cnt = z.shape[0] * z.shape[1] * z.shape[2]
    var = z.var((0, 1, 2), unbiased=False)
    if cnt > 1 and mutant != "biased_running_var":
        var = var * cnt / (cnt - 1)
    return 0.9 * rmean + 0.1 * z.mean((0, 1, 2)), 0.9 * rvar + 0.1 * var


def _resample_matrix(n_in, n_out, nearest, dtype, mutant=None):
    """(n_out, n_in) weights of F.interpolate along one axis: bilinear with align_corners=False, or nearest."""
    M = torch.zeros(n_out, n_in, dtype=dtype)
    dst = torch.arange(n_out)
    if nearest:
        M[dst, (dst.to(dtype) * (n_in / n_out)).floor().long().clamp_max(n_in - 1)] = 1
        return M
    src = dst.to(dtype) * (n_in / n_out) if mutant == "no_half_pixel" else ((dst.to(dtype) + 0.5) * (n_in / n_out) - 0.5).clamp_min(0)
    i0 = src.floor().long().clamp_max(n_in - 1)
    lam = src - i0
    M[dst, i0] += 1 - lam
    M[dst, (i0 + 1).clamp_max(n_in - 1)] += lam
    return M


def resize(x, oh, ow, nearest=False, mutant=None):
    """F.interpolate(size=(oh, ow)) on NHWC as two matrix products."""
    _, h, w, _ = x.shape
    rows = torch.einsum("oh,bhwc->bowc", _resample_matrix(h, oh, nearest, x.dtype, mutant), x)
    return torch.einsum("pw,bowc->bopc", _resample_matrix(w, ow, nearest, x.dtype, mutant), rows)


def up2_bilinear(x, x2=None, mutant=None):
    """Upsample(scale_factor=2, bilinear) of x, or of cat([x, x2]) on the channels."""
    if x2 is not None:
        if mutant == "skip_half_dropped":  # the gradient of the second source never written
            x2 = x2.detach() + 0 * x2
        x = torch.cat([x, x2], -1)
    return resize(x, 2 * x.shape[1], 2 * x.shape[2])


def conv_transpose4s2(x, w, b, mutant=None):
    """ConvTranspose2d(cin, C, 4, stride 2, padding 1) as a scatter over taps: x (nb,h,w,cin), w (cin,C,4,4) -> (nb,2h,2w,C)."""
    nb, h, wd, _ = x.shape
    y = torch.zeros(nb, 2 * h + 2, 2 * wd + 2, w.shape[1], dtype=x.dtype)
    for ky in range(4):
        for kx in range(4):
            tap = w[:, :, kx, ky] if mutant == "taps_transposed" else w[:, :, ky, kx]
            y[:, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] = y[:, ky:ky + 2 * h:2, kx:kx + 2 * wd:2] + x @ tap
    return y[:, 1:2 * h + 1, 1:2 * wd + 1] + b


# ----------------------------------------------------------------------------------------------------------------- the cases
class Case:
    """One op at one shape: fp32 CPU inputs / parameters / output gradient, the arguments of HipEngine.op_train, and the reference."""

    def __init__(self, cid, op, ins, params, fn, kw=None, p=0.0, keep_shape=None, in_names=("x",), p_names=(), split_qkv=False):
        self.id, self.op, self.ins, self.params, self.fn, self.kw, self.p = cid, op, ins, params, fn, dict(kw or {}), p
        self.keep_shape = keep_shape          # per batch row, in the engine's element order; None: no dropout site
        self.in_names, self.p_names, self.split_qkv = in_names, p_names, split_qkv
        self.dout = None
        self.grad_inputs = [True] * len(ins)  # a time input has no gradient
        self.stats = None       # norm_act on batch statistics: (ins, params, mutant) -> {"running_mean", "running_var"} after the forward
        self.mask = None        # an injected uint8 keep mask: the forward alone runs
        self.skip_grad = None   # up2_bilinear: the gradient its second source already has

    def run(self, dtype=torch.float64, keep=None, mutant=None, grads_in=None):
        """-> {"y", "d<input>", ..., "d<param>", ...} in `dtype` by torch.autograd; parameter gradients start from `grads_in`."""
        ins = [t.to(dtype).requires_grad_(g) for t, g in zip(self.ins, self.grad_inputs)]
        ps = [t.to(dtype).requires_grad_(i < len(self.p_names)) for i, t in enumerate(self.params)]  # running statistics come last
        kw = {}
        if keep is not None:
            kw["keep"] = keep.to(dtype)
        if mutant is not None and mutant != "dv_without_keep":
            kw["mutant"] = mutant
        y = self.fn(ins, ps, **kw)
        leaves = [t for t in ins + ps if t.requires_grad]
        grads = list(torch.autograd.grad(y, leaves, self.dout.to(dtype).reshape(y.shape)))
        out = {"y": y.detach()}
        for name, t in zip(self.in_names, ins):
            if t.requires_grad:
                out["d" + name] = grads.pop(0)
        for i, name in enumerate(self.p_names):
            out["d" + name] = grads.pop(0) + (0 if grads_in is None else grads_in[i].to(dtype))
        if mutant == "dv_without_keep":  # dv_j = sum_i P_ij dout_i, the dropout of the probabilities forgotten
            q, k, _ = _heads(ins[0].detach())
            pr = (torch.einsum("bihd,bjhd->bhij", q, k) * DH ** -0.5).softmax(-1)
            dv = torch.einsum("bhij,bihd->bjhd", pr, self.dout.to(dtype).reshape(q.shape))
            out["dx"] = torch.cat([out["dx"][..., :2 * HID], dv.reshape(out["dx"][..., 2 * HID:].shape)], -1)
        if self.split_qkv:
            d = out.pop("dx")
            out.update(dq=d[..., :HID], dk=d[..., HID:2 * HID], dv=d[..., 2 * HID:])
        if self.skip_grad is not None:
            out["dx2"] = out["dx2"] + self.skip_grad.to(dtype)
        if self.stats is not None:
            out.update(self.stats([t.detach() for t in ins], [t.detach() for t in ps], mutant))
        if self.mask is not None:
            out = {k: v for k, v in out.items() if not k.startswith("d")}
        return out


def engine_keep(case):
    """The keep mask the engine draws for `case` (dyf_seed(SEED), first forward, site 0, rows ROW_OFFSET ..), rebuilt on the host."""
    if case.mask is not None:
        return case.mask.double()
    if case.keep_shape is None:
        return None
    rows = [rng_host.row_mask_nhwc(case.keep_shape, case.p, SEED, 0, 0, ROW_OFFSET + r) for r in range(case.ins[0].shape[0])]
    return torch.from_numpy(np.stack(rows).astype(np.float64))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * (int(v) + 13) for i, v in enumerate(key)) % (2 ** 31))


def _rn(g, *shape, scale=1.5):
    return torch.randn(*shape, generator=g) * scale


def _grid(hw):
    """(h, w) with h * w = hw (the ops see pixels only; 225 = 15 x 15 and 4225 = 65 x 65 are the OISST planes)."""
    r = int(math.isqrt(hw))
    while hw % r:
        r -= 1
    return r, hw // r


LINATTN_HW, ATTN_N = (1, 31, 33, 225, 257, 545), (1, 63, 65, 225)
NORM_C, GN_HW, LN_HW = (8, 24, 64, 256, 512), (1, 35, 225), (1, 33, 225)
# (k, stride, pad, cin, cout, ws, bias)
CONV_LAYERS = [(7, 1, 3, 3, 8, 0, 1), (7, 1, 3, 3, 64, 0, 1), (3, 1, 1, 8, 8, 1, 1), (3, 1, 1, 24, 40, 1, 1), (3, 1, 1, 64, 64, 1, 1),
               (3, 1, 1, 128, 64, 1, 1), (1, 1, 0, 16, 8, 0, 1), (1, 1, 0, 128, 64, 0, 1), (1, 1, 0, 64, 1, 0, 1)]
CONV_GRIDS = [(11, 13), (16, 16)]
LINEAR = [(1, 16, 4, 0), (5, 17, 6, 1), (17, 256, 130, 1), (33, 64, 512, 0)]
# unet_simple: (C, activation) -- both activations of a UNetBlock at the channel count that straddles quads
US_NORM_C, US_PLANES = [(8, "leaky"), (24, "leaky"), (24, "relu"), (64, "relu")], [(1, 1), (3, 5), (15, 15)]
US_KINDS = ("bn_batch", "bn_running", "gn8")
UP2_PLANES, UP2_SOURCES = [(1, 1), (2, 3), (5, 4), (16, 16)], [(4, 0), (12, 0), (4, 8), (8, 4)]


def conv_form(ci, co):
    """Which forward the training step runs for a channel pair: the fp32 matrix-core implicit GEMM (csrc/train_gemm.hip: input channels
    in stages of 16, output channels in tiles of 64) or the plain VALU kernel.  The GPU test checks the name against the engine."""
    return "mfma" if ci % 16 == 0 and co % 64 == 0 else "valu"


def specs(op):
    """The (id, arguments) of every case of `op`, cheap to list; `build` draws the tensors."""
    S = []
    if op == "linattn":
        S = [(f"hw{hw}-nb{nb}-{kind}", (hw, nb, kind)) for hw in LINATTN_HW for nb in (1, 3) for kind in ("randn", "wide")]
    elif op == "attention":
        S = [(f"N{n}-nb{nb}-p{p}-{kind}", (n, nb, p, kind)) for n in ATTN_N for nb in (1, 3) for p in (0.0, 0.15) for kind in ("randn", "wide")]
    elif op == "gn_act":
        S = [(f"C{c}-hw{hw}-nb{nb}-{'film' if f else 'plain'}-p{p}", (c, hw, nb, f, p))
             for c in NORM_C for hw in GN_HW for nb in (1, 3) for f in (0, 1) for p in (0.0, 0.2)]
        S.append(("C8-hw4225-nb8-film-p0.2", (8, 4225, 8, 1, 0.2)))  # pixels per workgroup: 17 (hw / 256 rounded up) instead of 16
    elif op == "layernorm":
        S = [(f"C{c}-hw{hw}-nb{nb}-p{p}", (c, hw, nb, p)) for c in NORM_C for hw in LN_HW for nb in (1, 3) for p in (0.0, 0.1)]
    elif op == "conv":
        for k, s, pd, ci, co, ws, bias in CONV_LAYERS:
            S += [(f"k{k}s{s}p{pd}-{ci}to{co}{'-ws' if ws else ''}-{h}x{w}-nb{nb}-{conv_form(ci, co)}", (k, s, pd, ci, co, ws, bias, h, w, nb, 0))
                  for h, w in CONV_GRIDS for nb in (1, 3)]
        S += [(f"k4s2p1-64to64-{h}x{w}-nb{nb}-mfma", (4, 2, 1, 64, 64, 0, 1, h, w, nb, 0)) for h, w in ((12, 16), (11, 13)) for nb in (1, 3)]
        S.append(("k3s1p1-8to8-ws-var0-11x13-nb3-valu", (3, 1, 1, 8, 8, 1, 1, 11, 13, 3, 1)))
    elif op == "linear":
        S = [(f"rows{r}-K{k}-O{o}-pre{pre}", (r, k, o, pre)) for r, k, o, pre in LINEAR]
    elif op == "norm_act":  # (kind, C, h, w, nb, film, p, act, drop): drop "mask" = an injected keep mask (forward only), "gen" = the generator
        S = [(f"{kind}-C{c}-{act}-{h}x{w}-nb{nb}-{'film' if f else 'plain'}-p{p}", (kind, c, h, w, nb, f, p, act, "mask"))
             for kind in US_KINDS for c, act in US_NORM_C for h, w in US_PLANES for nb in (1, 3) for f in (0, 1) for p in (0.0, 0.1)]
        S += [(f"{kind}-C8-leaky-65x65-nb2-film-p0.0", (kind, 8, 65, 65, 2, 1, 0.0, "leaky", "mask")) for kind in US_KINDS]  # 17 pixels per workgroup
        # dropout from the generator, with its gradients: the quad (8, 64) and the straddling (24) channel paths of the adjoint's kernels
        S += [(f"{kind}-C{c}-{act}-{h}x{w}-nb3-{'film' if f else 'plain'}-p0.1-gen", (kind, c, h, w, 3, f, 0.1, act, "gen"))
              for kind in US_KINDS for c, act, h, w, f in ((24, "relu", 3, 5, 1), (8, "leaky", 15, 15, 0), (64, "relu", 3, 5, 1))]
    elif op == "up2_bilinear":  # (h, w, ca, cb, nb, skip_grad)
        S = [(f"{h}x{w}-{ca}+{cb}-nb{nb}", (h, w, ca, cb, nb, 0)) for h, w in UP2_PLANES for ca, cb in UP2_SOURCES for nb in (1, 3)]
        S += [(f"{h}x{w}-{ca}+{cb}-nb3-onto-skip-grad", (h, w, ca, cb, 3, 1)) for h, w in ((5, 4), (16, 16)) for ca, cb in ((4, 8), (8, 4))]
        S += [("5x4-3+3-nb3-fallback", (5, 4, 3, 3, 3, 0)), ("5x4-3+3-nb3-fallback-onto-skip-grad", (5, 4, 3, 3, 3, 1)), ("5x4-6+0-nb3-fallback", (5, 4, 6, 0, 3, 0))]
    elif op == "resize":  # (h, w, oh, ow, nearest)
        S = [(f"{h}x{w}-to-{oh}x{ow}-{'nearest' if n else 'bilinear'}", (h, w, oh, ow, n)) for h, w, oh, ow in ((11, 13, 16, 16), (16, 16, 11, 13)) for n in (0, 1)]
        S.append(("11x13-identity", (11, 13, 11, 13, 0)))
    elif op == "convt":  # (dim, C, h, w, nb)
        S = [(f"{d}to{c}-{h}x{w}-nb{nb}", (d, c, h, w, nb)) for d in (8, 64) for c in (1, 3) for h, w in ((4, 4), (11, 13)) for nb in (1, 3)]
        S.append(("64to3-64x64-nb1", (64, 3, 64, 64, 1)))  # 4096 pixels: the small-channel matrix-core forms of the real step's readout
    elif op == "small":
        S = [("learned_sinu-half8", ("learned_sinu", 8)), ("learned_sinu-half5", ("learned_sinu", 5)), ("dropout-3x5x7", ("dropout",)),
             ("gelu", ("gelu",)), ("add-a-b", ("add", 0)), ("add-a-a", ("add", 1)), ("cat-8+24", ("cat", 8, 24)), ("cat-3+5", ("cat", 3, 5)),
             ("up2-3x5x8", ("up2_nearest", 3, 5, 8)), ("up2-1x1x4", ("up2_nearest", 1, 1, 4))]
    return S


def build(op, args):
    """Draw the tensors of one case: inputs randn * 1.5 from a CPU generator seeded by the case."""
    if op == "linattn":
        hw, nb, kind = args
        g = _gen(1, hw, nb, kind == "wide")
        qkv = _rn(g, nb, *_grid(hw), 3 * HID)
        if kind == "wide":  # k over a wide range, every channel's maximum in the LAST pixel: the running (max, sum) merges do work
            k = qkv[..., HID:2 * HID]
            k *= 4.0
            k[:, -1, -1, :] = k.reshape(nb, hw, HID).amax(1) + 2.0
        c = Case(None, op, [qkv], [], lambda i, p, **kw: linattn(i[0], **kw), split_qkv=True)
        c.dout = torch.randn(nb, *_grid(hw), HID, generator=g)
    elif op == "attention":
        n, nb, p, kind = args
        g = _gen(2, n, nb, kind == "wide")  # the same draw with and without dropout
        qkv = _rn(g, nb, *_grid(n), 3 * HID)
        if kind == "wide":
            qkv[..., :HID] *= 4.0
        c = Case(None, op, [qkv], [], lambda i, ps, **kw: attention(i[0], p=p, **kw), dict(p=p), p, (HEADS, n, n) if p else None, split_qkv=True)
        c.dout = torch.randn(nb, *_grid(n), HID, generator=g)
    elif op == "gn_act":
        C, hw, nb, f, p = args
        g = _gen(3, C, hw, nb, f)
        z = _rn(g, nb, *_grid(hw), C)
        ins = [z] + ([_rn(g, nb, 2 * C, scale=0.5)] if f else [])
        params = [1.0 + _rn(g, C, scale=0.5), _rn(g, C, scale=0.5)]
        c = Case(None, op, ins, params, lambda i, ps, **kw: gn_act(i[0], ps[0], ps[1], 8, i[1] if f else None, p=p, **kw), dict(groups=8, p=p), p,
                 (*_grid(hw), C) if p else None, ("z", "ss")[:len(ins)], ("gamma", "beta"))
        c.dout = torch.randn(z.shape, generator=g)
    elif op == "layernorm":
        C, hw, nb, p = args
        g = _gen(4, C, hw, nb)
        x = _rn(g, nb, *_grid(hw), C)
        c = Case(None, op, [x], [1.0 + _rn(g, 1, C, 1, 1, scale=0.5)], lambda i, ps, **kw: layernorm(i[0], ps[0], p=p, **kw), dict(p=p), p,
                 (*_grid(hw), C) if p else None, p_names=("g",))
        c.dout = torch.randn(x.shape, generator=g)
    elif op == "conv":
        k, s, pd, ci, co, ws, bias, h, w, nb, var0 = args
        g = _gen(5, k, s, ci, co, h, w, nb, var0)
        x = _rn(g, nb, h, w, ci)
        wt = _rn(g, co, ci, k, k, scale=1.5 / math.sqrt(ci * k * k))
        if var0:
            wt[1] = 0.25  # a constant weight row: variance 0, the standardised row is 0 and rstd = 1e-5 ** -0.5
        params = [wt] + ([_rn(g, co, scale=0.5)] if bias else [])
        c = Case(None, op, [x], params, lambda i, ps, **kw: conv(i[0], ps[0], ps[1] if bias else None, s, pd, bool(ws), **kw),
                 dict(k=k, stride=s, pad=pd, ws=bool(ws)), p_names=("weight", "bias")[:len(params)])
        c.dout = torch.randn(nb, (h + 2 * pd - k) // s + 1, (w + 2 * pd - k) // s + 1, co, generator=g)
    elif op == "linear":
        rows, K, O, pre = args
        g = _gen(6, rows, K, O)
        c = Case(None, op, [_rn(g, rows, K)], [_rn(g, O, K, scale=1.5 / math.sqrt(K)), _rn(g, O, scale=0.5)],
                 lambda i, ps: linear(i[0], ps[0], ps[1], bool(pre)), dict(pre=bool(pre)), p_names=("weight", "bias"))
        c.dout = torch.randn(rows, O, generator=g)
    elif op == "norm_act":
        kind, C, h, w, nb, f, p, act, drop = args
        g = _gen(9, US_KINDS.index(kind), C, h, w, nb, f)
        z = _rn(g, nb, h, w, C)
        ins = [z] + ([_rn(g, nb, 2 * C, scale=0.5)] if f else [])
        params = [1.0 + _rn(g, C, scale=0.5), _rn(g, C, scale=0.5)]
        bn = kind != "gn8"
        if bn:
            params += [_rn(g, C, scale=0.5), 0.5 + torch.rand(C, generator=g)]
        groups, running = (0 if bn else 8), kind == "bn_running"
        c = Case(None, op, ins, params,
                 lambda i, ps, **kw: norm_act(i[0], ps[0], ps[1], *(ps[2:] if bn else (None, None)), groups, running, act, i[1] if f else None, p=p, **kw),
                 dict(groups=groups, p=p, act=act, running=running), p, (h, w, C) if p and drop == "gen" else None, ("z", "ss")[:len(ins)], ("gamma", "beta"))
        if kind == "bn_batch":
            c.stats = lambda i, ps, mutant: dict(zip(("running_mean", "running_var"), bn_running_update(i[0], ps[2], ps[3], mutant)))
        if p and drop == "mask":
            c.mask = (torch.rand(nb, h, w, C, generator=g) >= p).to(torch.uint8)
        c.dout = torch.randn(z.shape, generator=g)
    elif op == "up2_bilinear":
        h, w, ca, cb, nb, sg = args
        g = _gen(10, h, w, ca, cb, nb)
        ins = [_rn(g, nb, h, w, ca)] + ([_rn(g, nb, h, w, cb)] if cb else [])
        c = Case(None, op, ins, [], lambda i, ps, **kw: up2_bilinear(*i, **kw), in_names=("x", "x2")[:len(ins)])
        c.dout = torch.randn(nb, 2 * h, 2 * w, ca + cb, generator=g)
        if sg:
            c.skip_grad = torch.randn(ins[1].shape, generator=g)
    elif op == "resize":
        h, w, oh, ow, near = args
        g = _gen(11, h, w, oh, ow, near)
        c = Case(None, op, [_rn(g, 3, h, w, 5)], [], lambda i, ps, **kw: resize(i[0], oh, ow, bool(near), **kw), dict(size=(oh, ow), nearest=bool(near)))
        c.dout = torch.randn(3, oh, ow, 5, generator=g)
    elif op == "convt":
        d, C, h, w, nb = args
        g = _gen(12, d, C, h, w, nb)
        c = Case(None, op, [_rn(g, nb, h, w, d)], [_rn(g, d, C, 4, 4, scale=1.5 / math.sqrt(4 * d)), _rn(g, C, scale=0.5)],
                 lambda i, ps, **kw: conv_transpose4s2(i[0], ps[0], ps[1], **kw), p_names=("weight", "bias"))
        c.dout = torch.randn(nb, 2 * h, 2 * w, C, generator=g)
    elif args[0] == "learned_sinu":
        half = args[1]
        g = _gen(7, half)
        c = Case(None, "learned_sinu", [torch.rand(3, generator=g) * 2.0], [_rn(g, half, scale=1.0)], lambda i, ps: learned_sinu(i[0], ps[0]),
                 in_names=("t",), p_names=("weights",))
        c.grad_inputs = [False]
        c.dout = torch.randn(3, 2 * half + 1, generator=g)
    else:
        kind = args[0]
        g = _gen(8, len(kind), *args[1:])
        x = _rn(g, 3, 3, 5, 7)
        if kind == "dropout":
            c = Case(None, kind, [x], [], lambda i, ps, **kw: dropout(i[0], p=0.25, **kw), dict(p=0.25), 0.25, (3, 5, 7))
        elif kind == "gelu":
            c = Case(None, kind, [x], [], lambda i, ps: gelu(i[0]))
        elif kind == "add" and args[1]:
            c = Case(None, kind, [x], [], lambda i, ps: i[0] + i[0])
        elif kind == "add":
            c = Case(None, kind, [x, _rn(g, 3, 3, 5, 7)], [], lambda i, ps: i[0] + i[1], in_names=("a", "b"))
        elif kind == "cat":
            c = Case(None, kind, [_rn(g, 3, 3, 5, args[1]), _rn(g, 3, 3, 5, args[2])], [], lambda i, ps: torch.cat(i, -1), in_names=("a", "b"))
        else:
            c = Case(None, kind, [_rn(g, 3, *args[1:])], [], lambda i, ps: up2_nearest(i[0]))
        c.dout = torch.randn(c.fn([t.double() for t in c.ins], [], **({"keep": torch.ones(c.ins[0].shape)} if kind == "dropout" else {})).shape,
                             generator=g)
    return c
