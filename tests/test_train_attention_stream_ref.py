"""No GPU: the head-by-head closed-form float64 Attention forward + backward (tests/train_attention_stream_ref.py), the reference of the
streaming training kernels at 4225 tokens, equals tests/train_op_refs.attention + torch.autograd.  Bound 1e-10 rel-RMS: both sides are
float64 (2e-16 per operation) over sums of at most 97 terms."""
import pytest
import torch

from tests import train_op_refs as T
from tests.helpers import rel_rms
from tests.train_attention_stream_ref import attention_fwd_bwd64


@pytest.mark.parametrize("masked", [False, True], ids=["no-mask", "keep-mask"])
@pytest.mark.parametrize("n", [33, 97])
def test_closed_form_equals_autograd(n, masked):
    nb, p = 2, 0.15
    g = torch.Generator().manual_seed(1000 + n)
    qkv = torch.randn(nb, n, 384, generator=g) * 1.5
    dout = torch.randn(nb, n, 128, generator=g)
    keep = (torch.rand(nb, 4, n, n, generator=g) >= p).double() if masked else None
    x = qkv.double().reshape(nb, 1, n, 384).requires_grad_(True)
    y = T.attention(x, keep=keep, p=p if masked else 0.0)
    (dx,) = torch.autograd.grad(y, x, dout.double().reshape(y.shape))
    dx = dx.reshape(nb, n, 384)
    want = {"y": y.detach().reshape(nb, n, 128), "dq": dx[..., :128], "dk": dx[..., 128:256], "dv": dx[..., 256:]}
    got = attention_fwd_bwd64(qkv, dout, keep, p if masked else 0.0)
    errs = {k: rel_rms(got[k], want[k]) for k in want}
    print(f"closed form vs autograd N={n} masked={masked}: {errs}")
    assert max(errs.values()) <= 1e-10, errs
    if masked:  # the mask did something
        assert rel_rms(got["y"], attention_fwd_bwd64(qkv, dout)["y"]) > 0.1
