"""A restated model of the engine's `train_precision="bf16x3"` convolutions (csrc/train_gemm.hip, csrc/train_halo16.hip) -- test
infrastructure, no GPU.

Every operand value v of a conv the 16-bit dispatch takes is staged as two bf16 values, hi = bf16(v) and lo = bf16(v - hi) (the
subtraction is exact in fp32), and a product a * b is computed as a_lo * b_hi + a_hi * b_lo + a_hi * b_hi with fp32 accumulation; the
a_lo * b_lo term (2^-16 of the product) is dropped.  The forward (x, w), the data gradient (dz, w) and the weight gradient (dz, x) are
split each on their own, and `oracle.losses.conv_operand_rules` -- the channel rules of the 16-bit forms -- says which of the three
are split for a layer; the others, the bias gradient and everything that is not a conv stay fp32, as under train_precision=32.

`terms=` counts the products kept, for the tests that show what the bound tells apart: 3 = the mode, 2 = one cross term dropped,
1 = plain bf16 operands (the bf16-mixed mode).  The functions compute in the dtype `acc` (float64 in the pinning tests: the error of
the split alone; float32 under autograd: the model of the engine's step).
"""
import torch

from oracle import losses, nets


def split(x):
    """(hi, lo): hi = bf16(x), lo = bf16(x - hi), both returned as float32 tensors holding bf16 values."""
    x = x.to(torch.float32)
    hi = x.to(torch.bfloat16).to(torch.float32)
    lo = (x - hi).to(torch.bfloat16).to(torch.float32)
    return hi, lo


def _three(fn, a, b, terms, acc):
    """fn is bilinear in (a, b): the sum of the kept products, cross terms first, then hi x hi (the kernels' order)."""
    (ah, al), (bh, bl) = split(a), split(b)
    ah, al, bh, bl = (t.to(acc) for t in (ah, al, bh, bl))
    out = fn(ah, bh)
    if terms >= 2:
        out = fn(ah, bl) + out
    if terms >= 3:
        out = fn(al, bh) + out
    return out


def conv_forward(x, w, bias=None, stride=1, padding=0, terms=3, acc=torch.float32):
    """x (n, cin, h, w), w (cout, cin, k, k) -> y (n, cout, ho, wo)."""
    y = _three(lambda a, b: torch.nn.functional.conv2d(a, b, None, stride=stride, padding=padding), x, w, terms, acc)
    return y if bias is None else y + bias.to(acc)[None, :, None, None]


def conv_input_grad(x_shape, w, dz, stride=1, padding=0, terms=3, acc=torch.float32):
    return _three(lambda a, b: torch.nn.grad.conv2d_input(x_shape, b, a, stride=stride, padding=padding), dz, w, terms, acc)


def conv_weight_grad(x, w_shape, dz, stride=1, padding=0, terms=3, acc=torch.float32):
    return _three(lambda a, b: torch.nn.grad.conv2d_weight(b, w_shape, a, stride=stride, padding=padding), dz, x, terms, acc)


class _Conv2dSplit3(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, w, bias, stride, padding):
        cout, cin = w.shape[0], w.shape[1]
        f3, d3, w3 = losses.conv_operand_rules(cin, cout)
        ctx.save_for_backward(x, w)
        ctx.cfg = (stride, padding, d3, w3, bias is not None)
        if f3:
            return conv_forward(x, w, bias, stride, padding)
        return torch.nn.functional.conv2d(x, w, bias, stride=stride, padding=padding)

    @staticmethod
    def backward(ctx, dz):
        x, w = ctx.saved_tensors
        stride, padding, d3, w3, has_bias = ctx.cfg
        dz = dz.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = (conv_input_grad(x.shape, w, dz, stride, padding) if d3
                  else torch.nn.grad.conv2d_input(x.shape, w, dz, stride=stride, padding=padding))
        if ctx.needs_input_grad[1]:
            dw = (conv_weight_grad(x, w.shape, dz, stride, padding) if w3
                  else torch.nn.grad.conv2d_weight(x, w.shape, dz, stride=stride, padding=padding))
        if has_bias and ctx.needs_input_grad[2]:
            db = dz.sum(dim=(0, 2, 3))  # the bias gradient is a plain fp32 reduction of dz in the engine too
        return dx, dw, db, None, None


class split3_operands:
    """`with split3_operands(): ...` -- every nn.Conv2d of the restated backbones (oracle.nets.conv2d) runs as the engine's bf16x3
    training convolution for the duration of the block (the way oracle.losses.training_operand_rounding patches the bf16-mixed one in)."""

    def __enter__(self):
        self._prev = nets._CONV2D[0]
        nets._CONV2D[0] = lambda x, w, bias=None, stride=1, padding=0: _Conv2dSplit3.apply(x, w, bias, stride, padding)
        return self

    def __exit__(self, *exc):
        nets._CONV2D[0] = self._prev
        return False
