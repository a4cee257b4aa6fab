"""The host side of the sampling mode `dtype="bf16x3"` (dyf_set_sample_precision(48)): the dtype surface, and what the 1e-4 rollout
bound of tests/test_gpu_bf16x3_sampling.py tells apart.

The bound is the project's fp32 sampling line (TOL32 = 1e-4 per field), not a figure taken from the mode.  The three-term
model of tests/split3_refs.py, applied to every conv `oracle.losses.conv_operand_rules` marks for the forward, sits about 6x inside it
over the rollouts the GPU tests run (1.6e-5 .. 1.7e-5; one unet.Unet forward 1.2e-5); a model that drops one cross term or keeps one
bf16 product sits at 4e-3 .. 9e-3, 40x or more outside.  So the GPU bound holds the mode and fails a kernel that forgot a term.
"""
import os
import re

import pytest

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from tests import bf16x3_sampling_refs as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _pair(**kw):
    F = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=4, num_output_channels=4, num_conditional_channels=1)
    I = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=8, num_output_channels=4, num_conditional_channels=1)
    return D.DYffusion(F, D.InterpolatorHandle(I, 4), timesteps=4, forward_conditioning="none", interpolate_before_t1=True, **kw)


def test_dtype_surface():
    for spelling in ("bf16x3", "BF16X3", "48"):
        m = _pair(dtype=spelling)
        assert m._engine_opts["dtype"] == "bf16x3" and m._engine is None  # engines are built lazily
    assert L.canonical_dtype("bf16x3") == L.canonical_dtype(48) == "bf16x3"
    assert L.storage_dtype("bf16x3") == "bf16" and L.storage_dtype("fp32") == "bf16" and L.storage_dtype("fp16") == "fp16"
    assert L.SAMPLE_PRECISION_BITS == {"fp32": 32, "bf16x3": 48} and L.DYF_SAMPLE_PRECISION_BF16X3 == 48
    with pytest.raises(ValueError):
        L.canonical_dtype("fp17")
    with pytest.raises(ValueError):
        _pair(dtype="fp17")
    assert L.DYF_ABI_VERSION == 9
    with open(os.path.join(ROOT, "include", "dyffusion_hip.h")) as f:
        h = f.read()
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", h, re.M)
    assert re.search(r"^#define\s+DYF_SAMPLE_PRECISION_BF16X3\s+48\s*$", h, re.M)
    doc = h[h.index("Sampling precision (ABI 9)"):h.index("dyf_status dyf_set_sample_precision")]
    assert "bits = 48" in doc and "returns 16, 32 or 48" in doc
    with open(os.path.join(ROOT, "include", "dyffusion_hip_testing.h")) as f:
        assert re.search(r"^#define\s+DYF_TOP_SAMPLE\s+8192\s*$", f.read(), re.M)
    assert L.TOP_SAMPLE == 8192


CASES = {
    "unet_simple-64x64-rollout": lambda terms: B.simple_rollout(B.MK64, terms),
    "unet_simple-128x128-rollout": lambda terms: B.simple_rollout(B.MK128, terms),
    "unet_resnet-64x96-forward": B.resnet_forward,
}


@pytest.mark.parametrize("case", list(CASES))
def test_the_rollout_bound_holds_three_terms_and_fails_fewer(case):
    run = CASES[case]
    want = run(None)
    errs = {terms: B.worst(run(terms), want) for terms in (3, 2, 1)}
    print(f"bf16x3 sampling model {case}: three terms {errs[3]:.3e}, two {errs[2]:.3e}, one {errs[1]:.3e} (worst rel-RMS per field vs the fp32 oracle)")
    assert errs[3] <= B.TOL32, errs
    assert errs[2] >= 1e-3 and errs[1] >= 1e-3, errs
