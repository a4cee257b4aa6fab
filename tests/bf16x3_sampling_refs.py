"""Fixtures and CPU models shared by tests/test_bf16x3_sampling_host.py and tests/test_gpu_bf16x3_sampling.py -- test infrastructure.

The sampling mode `dtype="bf16x3"` (dyf_set_sample_precision(48)) is the fp32 sampling forward with the three-term bf16 operands of
tests/split3_refs.py in every conv that `oracle.losses.conv_operand_rules` marks for the forward.  `split_forward_convs(terms)` patches
exactly that into the restated backbones (terms = 3: the mode; 2: one cross term dropped; 1: plain bf16 operands), with fp32
accumulation as the kernels have it.  Every fixture is built once per process and never modified.
"""
import torch

from oracle import losses, nets
from tests import split3_refs as S3

TOL32 = 1e-4  # the project's fp32 sampling line (tests/test_gpu_fp32_sampling.py)

# the dim-64 pair and plan of tests/test_gpu_fp32_sampling.py
HP4 = dict(timesteps=4, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only",
           sampling_type="cold", refine_intermediate_predictions=True, enable_interpolator_dropout=False, num_input_channels=3)
MK64 = dict(dim=64, upsample_dims=[64, 64], outer_sample_mode="bilinear", with_time_emb=True, dropout=0.15)
MK128 = dict(MK64, upsample_dims=[128, 128])
# unet.Unet dim 64, mults (1, 2), 2 -> 1 channels
RESNET_CFG = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0,
                  resnet_block_groups=8, input_dropout=0.0, upsample_dims=None)


class split_forward_convs:
    """`with split_forward_convs(terms): ...` -- every conv of the restated backbones whose forward the 16-bit dispatch takes runs as
    the sum of `terms` bf16 products (fp32 accumulation); the others stay fp32 convs."""

    def __init__(self, terms):
        self.terms = terms

    def __enter__(self):
        self._prev = nets._CONV2D[0]
        terms = self.terms

        def conv(x, w, bias=None, stride=1, padding=0):
            if losses.conv_operand_rules(w.shape[1], w.shape[0])[0]:
                return S3.conv_forward(x, w, bias, stride, padding, terms=terms)
            return torch.nn.functional.conv2d(x, w, bias, stride=stride, padding=padding)

        nets._CONV2D[0] = conv
        return self

    def __exit__(self, *exc):
        nets._CONV2D[0] = self._prev
        return False


_MEMO = {}


def _memo(key, fn):
    if key not in _MEMO:
        _MEMO[key] = fn()
    return _MEMO[key]


def simple_inputs():
    """(PF, PI, x0, c): the seeded dim-64 unet_simple pair and the 3 rows of 23 x 11 of the fp32 rollout test."""
    def make():
        from tests.gpu_common import seeded_pair
        PF, PI = seeded_pair(64, 3, 2)
        g = torch.Generator().manual_seed(2)
        return PF, PI, torch.randn(3, 3, 23, 11, generator=g), torch.rand(3, 2, 23, 11, generator=g)
    return _memo("simple_inputs", make)


def simple_rollout(mk, terms=None):
    """The HP4 rollout of the pair on the CPU: the fp32 oracle (terms None) or the `terms`-product model.  mk: MK64 | MK128."""
    def make():
        from tests.gpu_common import oracle_rollout
        PF, PI, x0, c = simple_inputs()
        if terms is None:
            return oracle_rollout(PF, PI, mk, HP4, x0, c)
        with split_forward_convs(terms):
            return oracle_rollout(PF, PI, mk, HP4, x0, c)
    return _memo(("simple", mk["upsample_dims"][0], terms), make)


def resnet_inputs():
    """(P, x, t): unet.Unet dim 64, mults (1, 2), 2 -> 1 channels, seed 91; 4 rows of 64 x 96."""
    def make():
        from tests.test_gpu_unet_resnet import seeded_unet
        P = seeded_unet(64, (1, 2), 2, 1, seed=91)
        g = torch.Generator().manual_seed(91)
        return P, torch.randn(4, 2, 64, 96, generator=g), torch.tensor([0.0, 1.0, 2.0, 3.0])
    return _memo("resnet_inputs", make)


def resnet_forward(terms=None):
    def make():
        P, x, t = resnet_inputs()
        with torch.no_grad():
            if terms is None:
                return nets.resnet_unet_forward(P, RESNET_CFG, x, t, None)
            with split_forward_convs(terms):
                return nets.resnet_unet_forward(P, RESNET_CFG, x, t, None)
    return _memo(("resnet", terms), make)


def worst(got, want):
    from tests.helpers import rel_rms
    if torch.is_tensor(want):
        return rel_rms(got, want)
    assert sorted(got) == sorted(want)
    return max(rel_rms(got[k], want[k]) for k in want)

