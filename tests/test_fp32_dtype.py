"""CPU: the fp32 sampling mode in the binding and in `DYffusion(dtype=...)` (no GPU needed: engines are built lazily)."""
import pytest

import dyffusion_amd as D
from dyffusion_amd import _lib as L


def _pair(**kw):
    F = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=4, num_output_channels=4,
               num_conditional_channels=1)
    I = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=8, num_output_channels=4,
               num_conditional_channels=1)
    return D.DYffusion(F, D.InterpolatorHandle(I, 4), timesteps=4, forward_conditioning="none", interpolate_before_t1=True, **kw)


@pytest.mark.parametrize("name", ["fp32", "float32", "32", "FP32"])
def test_dyffusion_accepts_fp32(name):
    m = _pair(dtype=name)
    assert m._engine_opts["dtype"] == "fp32" and m._engine is None


def test_unknown_dtype_is_a_value_error_at_construction():
    with pytest.raises(ValueError):
        _pair(dtype="fp17")
    assert _pair()._engine_opts["dtype"] == "bf16" and _pair(dtype="half")._engine_opts["dtype"] == "fp16"


def test_abi_9_declares_the_sample_precision_calls():
    assert L.DYF_ABI_VERSION == 9
    names = [s[0] for s in L.SYMBOLS]
    assert "dyf_set_sample_precision" in names and "dyf_sample_precision" in names
    assert L.storage_dtype("float32") == "bf16" and L.canonical_dtype("32") == "fp32"
