"""-m gpu: the 16-bit sampling kernels between the convs (csrc/unet_kernels.hip, csrc/kernels.hip), ONE launch at a time through the
launchers themselves (HipEngine.op_sample -> dyf_op_sample16), against float64 torch on the CPU -- for the bf16 and the fp16 build.

The network tests hold these kernels to 2e-2 (bf16) / 4e-3 (fp16) on a network output, or compare one kernel form with another: a
statistic that misses the last pixel, a slot of the conv-epilogue partials that is not added, a LayerNorm tail lane on the wrong pixel or
a mirrored border tap would pass all of them.  Here every launcher runs at the smallest shapes where its branches change (cases,
references and the reasoning of the bound: tests/sample_op_refs.py; that the bound tells those mistakes from the reference:
tests/test_sample_op_refs.py):

  16-bit outputs   excess = rms(got - round16(ref)) / rms(ref)  <=  floor = rms(round16(ref) - ref) / rms(ref), outputs finite
  fp32 output      (head) rel-RMS <= 1e-5
  copies           (nearest upsample, drop16) equal element for element

Every test prints excess, floor and the form the launcher noted; where a launcher notes its form, the case asserts it.  Generator
dropout masks are rebuilt on the host (tests/rng_host.py).
"""
import pytest
import torch

import dyffusion_amd as D
from tests import sample_op_refs as S
from tests.gpu_common import DEV
from tests.helpers import rel_rms

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def eng(request):
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False, dtype=request.param)
    yield e
    e.close()


def run(eng, b):
    dev = lambda v: v.to(DEV) if torch.is_tensor(v) else v
    if b.gen is not None:
        eng.seed(S.SEED)
    eng.form_log(True)
    try:
        y = eng.op_sample(b.op, [t.to(DEV) for t in b.xs], b.params, **{k: dev(v) for k, v in b.kw.items()})
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    return y.cpu(), forms


def check(eng, op, args, cid, form_switch):
    b = S.build(op, args, eng.dtype)
    for k, v in b.switch.items():
        form_switch.setenv(k, v)
    got, forms = run(eng, b)
    ref = b.ref()
    tag = f"sample-op {op} {cid}"  # (the id carries the build)
    noted = sorted(f for f in forms if f == b.form or f in b.quiet)
    assert bool(torch.isfinite(got.float()).all()), tag
    assert got.dtype == (torch.float32 if b.kind == "f32" else eng.torch_dtype) and tuple(got.shape) == tuple(ref.shape)
    if b.kind == "exact":
        want = S.round16(ref, eng.torch_dtype)
        diff = int((got.double() != want.double()).sum())  # equality of values: a dropped element is +0 in the kernel, x * 0 keeps x's sign
        print(f"{tag}: {diff} of {want.numel()} elements differ; form {noted or '-'}")
        assert diff == 0
    elif b.kind == "f32":
        err = rel_rms(got, ref)
        print(f"{tag}: rel-RMS {err:.3e} (bound {S.TOL_F32:.0e}; fp32 torch {rel_rms(b.ref(torch.float32), ref):.3e}); form {noted or '-'}")
        assert err <= S.TOL_F32
    else:
        excess, floor = S.excess_floor(got, ref, eng.torch_dtype)
        print(f"{tag}: excess {excess:.3e}, floor {floor:.3e}, excess / floor {excess / floor:.3f}; form {noted or '-'}")
        assert excess <= floor
    # the branch the case names, where the launcher notes one: its form, for this launch's rows, and no other form of the launcher
    assert noted == ([b.form] if b.form else []), (tag, forms)
    if b.form:
        assert forms[b.form] == {b.xs[0].shape[0]: 1}, (tag, forms)


def cases(op):
    return [pytest.param(args, id=cid) for cid, args in S.specs(op)]


@pytest.mark.parametrize("args", cases("gn_act"))
def test_gn_act(eng, args, request, form_switch):
    check(eng, "gn_act", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("layernorm_c"))
def test_layernorm_c(eng, args, request, form_switch):
    check(eng, "layernorm_c", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("head"))
def test_head(eng, args, request, form_switch):
    check(eng, "head", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("up2_nearest"))
def test_up2_nearest(eng, args, request, form_switch):
    check(eng, "up2_nearest", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("drop16"))
def test_drop16(eng, args, request, form_switch):
    check(eng, "drop16", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("stem_conv"))
def test_stem_conv(eng, args, request, form_switch):
    check(eng, "stem_conv", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("groupnorm_f32"))
def test_groupnorm_f32(eng, args, request, form_switch):
    check(eng, "groupnorm_f32", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("up2_bilinear"))
def test_up2_bilinear(eng, args, request, form_switch):
    check(eng, "up2_bilinear", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("up2_epilogue"))
def test_up2_epilogue(eng, args, request, form_switch):
    check(eng, "up2_epilogue", args, request.node.callspec.id, form_switch)


def test_what_the_seam_cannot_express_is_refused(eng):
    dt = eng.torch_dtype
    x = torch.zeros(1, 2, 2, 8, dtype=dt, device=DEV)
    one, zero = torch.ones(8), torch.zeros(8)
    with pytest.raises(ValueError):
        eng.op_sample("gn_act", x, [one, zero], groups=3)                                    # groups must divide c
    with pytest.raises(NotImplementedError):                                                 # 3 chunks: gn_part_supported says no
        eng.op_sample("gn_act", torch.zeros(1, 2, 2, 24, dtype=dt, device=DEV), [torch.ones(24), torch.zeros(24)], groups=3,
                      part=torch.zeros(1, 1, 3, 2, device=DEV))
    with pytest.raises(NotImplementedError):                                                 # 4 channels per group: no octet partials
        eng.op_sample("gn_act", torch.zeros(1, 2, 2, 32, dtype=dt, device=DEV), [torch.ones(32), torch.zeros(32)], groups=8,
                      part=torch.zeros(1, 1, 4, 2, device=DEV))
    with pytest.raises(ValueError):                                                          # 9 rows > 2 max_batch of the row-key table
        eng.op_sample("gn_act", torch.zeros(9, 2, 2, 8, dtype=dt, device=DEV), [one, zero], groups=1, p=0.3, rng_site=0)
    with pytest.raises(ValueError):                                                          # one keep word per PAIR of a row
        eng.op_sample("drop16", torch.zeros(2, 1, 3, 3, dtype=dt, device=DEV), mask=torch.ones(2, 1, 3, 3, dtype=torch.uint8, device=DEV), p=0.5)
    with pytest.raises(ValueError):                                                          # an op without a dropout
        eng.op_sample("up2_nearest", x, mask=torch.ones(1, 4, 4, 8, dtype=torch.uint8, device=DEV), p=0.5)
    with pytest.raises(NotImplementedError):                                                 # the epilogue dispatch has no GELU
        eng.op_sample("gn_act", x, [one, zero], groups=1, act="gelu")
    with pytest.raises(NotImplementedError):                                                 # channels four at a time
        eng.op_sample("up2_epilogue", torch.zeros(1, 2, 2, 6, device=DEV), film_a=torch.ones(1, 8, device=DEV), film_c=torch.zeros(1, 8, device=DEV))
