"""The host side of `train_precision="bf16x3"` (dyf_train_set_precision(48)): the parser, the header's constant, and the restated
three-term model tests/split3_refs.py, pinned on the matrix-core conv cases of tests/train_op_refs.py.

The pin: with float64 accumulation (the error of the split alone) the three-term forward, data gradient and weight gradient sit at
<= 6e-6 rel-RMS of float64 on every `-mfma` conv case without weight standardisation (measured 4.5e-6), one term -- plain bf16
operands -- at >= 1e-3 (measured 2.4e-3), and two terms, a dropped cross term, at >= 1e-4: the dropped a_lo * b_hi has |a_lo| up to
2^-9 |a|, an rms of about 2^-9 / sqrt(3) * 0.7 ~ 8e-4 of the product, ten times the bound at the least.  So the GPU test's 1e-5
(train_op_refs.TOL) tells the mode from bf16-mixed AND from a kernel that forgot a cross term.
"""
import os
import re

import pytest
import torch

from dyffusion_amd import _lib
from dyffusion_amd.engine import parse_train_precision
from oracle import losses, nets
from tests import split3_refs as S3
from tests import train_op_refs as T
from tests.helpers import rel_rms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (k, stride, pad, cin, cout, ws, bias, h, w, nb, var0): the matrix-core cases whose weights are the operand as stored
MFMA_PLAIN = [(cid, a) for cid, a in T.specs("conv") if cid.endswith("-mfma") and not a[5]]


def test_parser_accepts_bf16x3():
    assert parse_train_precision("bf16x3") == parse_train_precision(48) == parse_train_precision("48") == 48
    assert _lib.DYF_TRAIN_PRECISION_BF16X3 == 48
    assert parse_train_precision(None) == 0 and parse_train_precision(32) == 32 and parse_train_precision("bf16-mixed") == 16
    with pytest.raises(ValueError):
        parse_train_precision("8")
    with pytest.raises(ValueError):
        parse_train_precision("bf16x2")


def test_header_defines_the_constant_and_the_abi_version_stays():
    with open(os.path.join(ROOT, "include", "dyffusion_hip.h")) as f:
        h = f.read()
    assert re.search(r"^#define\s+DYF_TRAIN_PRECISION_BF16X3\s+48\s*$", h, re.M)
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", h, re.M)
    assert _lib.DYF_ABI_VERSION == 9


def test_split_is_exact_to_sixteen_bits():
    x = torch.randn(4096, generator=torch.Generator().manual_seed(3)) * 3.0
    hi, lo = S3.split(x)
    assert torch.equal(hi, losses.bf16_round(x)) and torch.equal(lo, losses.bf16_round(x - hi))
    # hi + lo keeps 16 mantissa bits: half an ulp of the lo image, 2^-9 (lo <= half an ulp of hi) * 2^-9, relative to |x|
    assert float(((hi + lo - x).abs() / x.abs()).max()) <= 2.0 ** -17


def test_there_are_eight_plain_matrix_core_cases():
    assert len(MFMA_PLAIN) == 8


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in MFMA_PLAIN])
def test_three_terms_meet_the_fp32_bound_and_fewer_do_not(args, request):
    k, s, pd, ci, co, ws, bias, h, w, nb, _ = args
    assert all(losses.conv_operand_rules(ci, co))
    case = T.build("conv", args)
    want = case.run()
    x, wt, dz = case.ins[0].permute(0, 3, 1, 2).contiguous(), case.params[0], case.dout.permute(0, 3, 1, 2).contiguous()
    b = case.params[1] if bias else None
    errs = {}
    for terms in (3, 2, 1):
        kw = dict(stride=s, padding=pd, terms=terms, acc=torch.float64)
        got = {"y": S3.conv_forward(x, wt, b, **kw).permute(0, 2, 3, 1),
               "dx": S3.conv_input_grad(x.shape, wt, dz, **kw).permute(0, 2, 3, 1),
               "dweight": S3.conv_weight_grad(x, wt.shape, dz, **kw)}
        errs[terms] = {n: rel_rms(got[n], want[n]) for n in got}
    worst = {t: max(e, key=e.get) for t, e in errs.items()}
    print(f"bf16x3 model {request.node.callspec.id}: three terms {errs[3][worst[3]]:.3e} ({worst[3]}), two {min(errs[2].values()):.3e} (best), "
          f"one {min(errs[1].values()):.3e} (best)")
    assert max(errs[3].values()) <= 6e-6 < T.TOL, errs[3]
    assert min(errs[2].values()) >= 1e-4 >= 10 * T.TOL, errs[2]
    assert min(errs[1].values()) >= 1e-3, errs[1]


def test_the_context_manager_patches_the_restated_convs_by_the_operand_rules():
    g = torch.Generator().manual_seed(5)
    prev = nets._CONV2D[0]
    for ci, co, split in ((64, 64, True), (3, 64, False)):
        x = torch.randn(2, ci, 8, 8, generator=g, requires_grad=True)
        w = (torch.randn(co, ci, 3, 3, generator=g) * 0.1).requires_grad_()
        b = torch.randn(co, generator=g).requires_grad_()
        dz = torch.randn(2, co, 8, 8, generator=g)
        plain = torch.autograd.grad(torch.nn.functional.conv2d(x, w, b, padding=1), (x, w, b), dz)
        with S3.split3_operands():
            assert nets._CONV2D[0] is not prev
            y = nets._CONV2D[0](x, w, b, stride=1, padding=1)
            got = torch.autograd.grad(y, (x, w, b), dz)
        assert rel_rms(got[2], plain[2]) <= 1e-6  # the bias gradient is never split: a plain fp32 sum of dz
        if split:  # fp32-grade, and not the fp32 kernel's bits
            assert all(rel_rms(a, p) <= 1e-5 for a, p in zip(got[:2], plain[:2]))
            assert not torch.equal(got[1], plain[1])
            assert torch.equal(y, S3.conv_forward(x.detach(), w.detach(), b.detach(), 1, 1))
        else:  # outside the channel rules: the fp32 conv itself
            assert torch.equal(y, torch.nn.functional.conv2d(x, w, b, padding=1))
            assert all(rel_rms(a, p) <= 1e-6 for a, p in zip(got, plain))
    assert nets._CONV2D[0] is prev
