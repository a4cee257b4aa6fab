"""CPU: the deterministic training mode (dyf_train_set_deterministic, the reference's `trainer.deterministic`) up to the GPU -- the rule
that resolves a `train_deterministic` setting, the C ABI of both builds of the library, and the option on DYffusion / UNet / Unet.
What the mode computes is tests/test_gpu_train_deterministic.py."""
import os
import re

import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from dyffusion_amd.engine import resolve_train_deterministic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_none_follows_torchs_flag_and_a_bool_wins_over_it():
    before = torch.are_deterministic_algorithms_enabled()
    try:
        for flag in (True, False):
            torch.use_deterministic_algorithms(flag)
            assert resolve_train_deterministic(None) is flag
            assert resolve_train_deterministic(True) is True
            assert resolve_train_deterministic(False) is False
    finally:
        torch.use_deterministic_algorithms(before)


@pytest.mark.parametrize("bad", [0, 1, "true", "on", 1.0, [True]])
def test_anything_but_a_bool_or_none_is_refused(bad):
    with pytest.raises(ValueError):
        resolve_train_deterministic(bad)


def test_the_header_declares_the_two_functions_next_to_the_precision_switch():
    with open(os.path.join(ROOT, "include", "dyffusion_hip.h")) as f:
        header = f.read()
    setter = re.search(r"dyf_status\s+dyf_train_set_deterministic\(dyf_engine\*\s*engine,\s*int32_t\s+on\);", header)
    getter = re.search(r"int32_t\s+dyf_train_deterministic\(const dyf_engine\*\s*engine\);", header)
    assert setter and getter
    assert header.index("dyf_train_set_precision(") < setter.start() < getter.start()
    assert re.search(r"#define DYF_ABI_VERSION 9\b", header)


@pytest.mark.parametrize("storage", ["bf16", "fp16"])
def test_both_builds_export_the_two_functions(storage):
    lib = L.lib(storage)
    assert lib.dyf_abi_version() == 9
    for name in ("dyf_train_set_deterministic", "dyf_train_deterministic"):
        assert hasattr(lib, name), name
    assert lib.dyf_train_set_deterministic(None, 1) == L.DYF_ERR_INVALID_ARGUMENT
    assert lib.dyf_train_deterministic(None) == -1


def _unet_simple():
    return D.UNet(dim=4, with_time_emb=True, upsample_dims=None, num_input_channels=1, num_output_channels=1, num_conditional_channels=1,
                  spatial_shape=(8, 8), verbose=False)


def test_the_models_accept_and_carry_the_option():
    for make in (_unet_simple, lambda: D.Unet(dim=8, dim_mults=(1, 2), num_input_channels=1, num_output_channels=1, spatial_shape=(8, 8))):
        net = make()
        assert net.train_deterministic is None  # the default follows torch
        net.train_deterministic = True
        assert net.train_deterministic is True and make().train_deterministic is None
    F, I = _unet_simple(), _unet_simple()
    for value in (None, True, False):
        m = D.DYffusion(F, D.InterpolatorHandle(I, 4), timesteps=4, interpolate_before_t1=True, train_deterministic=value)
        assert m.train_deterministic is value and m._engine_opts["train_deterministic"] is value
    m.train_set_deterministic(True)  # no engine yet: kept for the engine the first call creates
    assert m.train_deterministic is True and m._engine_opts["train_deterministic"] is True
    with pytest.raises(ValueError):
        D.DYffusion(F, D.InterpolatorHandle(I, 4), timesteps=4, interpolate_before_t1=True, train_deterministic="yes")
    with pytest.raises(ValueError):
        m.train_set_deterministic(1)
