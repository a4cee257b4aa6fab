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

The launchers around the networks (csrc/kernels.hip) go through the same seam: the readout in all of its kernel forms, pixel orders and
the compact-column input, its tap tables against the reference stencil, both stems, the time MLP and FiLM heads, the cold update, the
noisy condition (injected noise, and the generator's field against the host mirror's float64 Box-Muller of the same words) and the
generator's forward start / clone (equal).  fp32 outputs: rel-RMS <= 1e-5 against float64.
"""
import numpy as np
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
    with pytest.raises(ValueError):                                                          # a keyword of the launchers around the networks
        eng.op_sample("up2_nearest", x, out_hw=(4, 4))
    cmap = torch.tensor([0, -1, 1, -1], dtype=torch.int16, device=DEV)
    w32, w64 = torch.zeros(32, 2, 4, 4), torch.zeros(64, 2, 4, 4)
    with pytest.raises(NotImplementedError):                                                 # a compact input without fragments: launch_readout refuses
        eng.op_sample("readout", torch.zeros(1, 2, 2, 32, dtype=dt, device=DEV), [w32, torch.zeros(2)], out_hw=(3, 3), col_map=cmap)
    with pytest.raises(ValueError):                                                          # a stored column outside the compact row
        eng.op_sample("readout", torch.zeros(1, 2, 1, 64, dtype=dt, device=DEV), [w64, torch.zeros(2)], out_hw=(3, 3), col_map=cmap)
    with pytest.raises(NotImplementedError):                                                 # more output channels than the readout takes
        eng.op_sample("readout", torch.zeros(1, 2, 2, 8, dtype=dt, device=DEV), [torch.zeros(8, 9, 4, 4), torch.zeros(9)], out_hw=(3, 3))
    with pytest.raises(NotImplementedError):                                                 # the fused stem has 15 channels and the bias slot
        eng.op_sample("stem16", [torch.zeros(1, 16, 2, 2, device=DEV)], out_hw=(2, 2))
    with pytest.raises(ValueError):                                                          # a keyword of another op is not dropped
        eng.op_sample("readout", torch.zeros(1, 2, 2, 8, dtype=dt, device=DEV), [torch.zeros(8, 2, 4, 4), torch.zeros(2)], out_hw=(3, 3), tau=0.5)
    with pytest.raises(ValueError):                                                          # 9 rows > 2 max_batch of the row-key table
        eng.op_sample("rng_begin", [], nb=9)
    with pytest.raises(ValueError):
        eng.op_sample("stem16", [torch.zeros(9, 3, 2, 2, device=DEV)], out_hw=(2, 2), fold_rng=True)


# ------------------------------------------------------------------------------------------- the launchers around the networks
def check_net(eng, op, args, cid, form_switch):
    b = S.build(op, args, eng.dtype)
    for k, v in b.switch.items():
        form_switch.setenv(k, v)
    dev = lambda v: v.to(DEV) if torch.is_tensor(v) else v
    if b.seed:
        eng.seed(S.SEED)
    eng.form_log(True)
    try:
        calls = [eng.op_sample(b.op, [t.to(DEV) for t in b.xs], b.params, **{k: dev(v) for k, v in b.kw.items()}) for _ in range(b.repeat)]
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    got = [o.cpu() for call in calls for o in S.outputs(call) if o is not None]
    refs = S.outputs(b.ref())
    kinds = S.outputs(b.kind) if len(refs) > 1 else [b.kind if isinstance(b.kind, str) else b.kind[0]]
    tag = f"sample-op {op} {cid}"
    noted = sorted(f for f in forms if f == b.form or f in b.quiet)
    assert len(got) == len(refs) == len(kinds), tag
    for i, (y, ref, kind) in enumerate(zip(got, refs, kinds)):
        assert tuple(y.shape) == tuple(ref.shape), (tag, i)
        if kind == "eq":
            diff = int((y != ref).sum())
            print(f"{tag} [{i}]: {diff} of {ref.numel()} words differ")
            assert y.dtype == ref.dtype and diff == 0, (tag, i, y, ref)
            continue
        assert bool(torch.isfinite(y.float()).all()), (tag, i)
        if kind == "f32":
            err = rel_rms(y, ref)
            print(f"{tag} [{i}]: rel-RMS {err:.3e} (bound {S.TOL_F32:.0e}); form {noted or '-'}")
            assert y.dtype == torch.float32 and err <= S.TOL_F32, (tag, i)
        else:
            excess, floor = S.excess_floor(y, ref, eng.torch_dtype)
            print(f"{tag} [{i}]: excess {excess:.3e}, floor {floor:.3e}, excess / floor {excess / floor:.3f}; form {noted or '-'}")
            assert y.dtype == eng.torch_dtype and excess <= floor, (tag, i)
    assert noted == ([b.form] if b.form else []), (tag, forms)
    if b.form:
        assert forms[b.form] == {b.rows: b.repeat}, (tag, forms)
    return b, got


@pytest.mark.parametrize("args", cases("readout"))
def test_readout(eng, args, request, form_switch):
    check_net(eng, "readout", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("stem"))
def test_stem(eng, args, request, form_switch):
    check_net(eng, "stem", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("stem16"))
def test_stem16(eng, args, request, form_switch):
    b, got = check_net(eng, "stem16", args, request.node.callspec.id, form_switch)
    y = got[0].float()
    # what the composed enc0 weights rely on, exactly: a zero border, slot cin = 1 inside the image, zeros above it
    assert int((y[:, 0] != 0).sum() + (y[:, -1] != 0).sum() + (y[:, :, 0] != 0).sum() + (y[:, :, -1] != 0).sum()) == 0
    assert bool((y[:, 1:-1, 1:-1, b.cin] == 1).all()) and int((y[..., b.cin + 1:] != 0).sum()) == 0


@pytest.mark.parametrize("args", cases("time_mlp"))
def test_time_mlp(eng, args, request, form_switch):
    check_net(eng, "time_mlp", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("film"))
def test_film(eng, args, request, form_switch):
    check_net(eng, "film", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("cold_update"))
def test_cold_update(eng, args, request, form_switch):
    b, got = check_net(eng, "cold_update", args, request.node.callspec.id, form_switch)
    if args["copy"]:
        assert torch.equal(got[0], got[1])  # the second destination holds the new x_s itself


@pytest.mark.parametrize("args", cases("noisy_condition"))
def test_noisy_condition(eng, args, request, form_switch):
    b, got = check_net(eng, "noisy_condition", args, request.node.callspec.id, form_switch)
    if args["gen"]:
        assert not torch.equal(got[0], got[1])


@pytest.mark.parametrize("args", cases("rng_begin"))
def test_rng_begin(eng, args, request, form_switch):
    check_net(eng, "rng_begin", args, request.node.callspec.id, form_switch)


@pytest.mark.parametrize("args", cases("rng_clone"))
def test_rng_clone(eng, args, request, form_switch):
    check_net(eng, "rng_clone", args, request.node.callspec.id, form_switch)


def test_folded_forward_start_equals_the_kernel_of_its_own(eng):
    """stem16's block 0 and rng_begin_forward_kernel leave the same row-key table and the same generator state."""
    srcs = [torch.zeros(2, 3, 5, 40, device=DEV)]
    for fuw in (256, 9):  # stem16_rows_kernel, stem16_kernel
        eng.seed(S.SEED)
        _, keys, state = eng.op_sample("stem16", srcs, out_hw=(8, fuw), nb=4, src_rows=2, fold_rng=True, rng_row_offset=9, rng_forward=3)
        eng.seed(S.SEED)
        keys2, state2 = eng.op_sample("rng_begin", [], nb=4, src_rows=2, rng_row_offset=9, rng_forward=3)
        assert torch.equal(keys, keys2) and torch.equal(state, state2) and int(state[2]) == 5 and int(state[3]) == 9


TABLE_GEOMS = [((2, 3), (4, 6), 0), ((6, 8), (5, 7), 0), ((6, 8), (5, 7), 1), ((2, 2), (9, 11), 0), ((2, 2), (9, 11), 1), ((1, 1), (3, 3), 0),
               ((8, 8), (192, 192), 0), ((6, 16), (5, 3), 0), ((6, 16), (5, 3), 1)]


# compact: where the stencil leaves decoder columns unread
TABLE_CASES = [pytest.param(g, c, id=f"{g[0][0]}x{g[0][1]}-{g[1][0]}x{g[1][1]}{'-nearest' if g[2] else ''}{'-compact' if c else ''}")
               for g in TABLE_GEOMS for c in (0, 1) if not c or len(S.readout_columns(g[0][1], g[1][1], bool(g[2]))[0]) < g[0][1]]


@pytest.mark.parametrize("geom,compact", TABLE_CASES)
def test_readout_tables(eng, geom, compact):
    """row_tab / col_tab against the reference stencil (S.readout_taps): byte offsets of the input row / stored column of every kernel tap
    that contributes, -1 outside the image, and the bilinear weight.  The weight's tolerance: the source coordinate (at most 2 n_in) takes
    three fp32 roundings in bilinear_coord."""
    (ih, iw), (oh, ow), near = geom
    used, cmap = S.readout_columns(iw, ow, bool(near))
    iws = len(used) if compact else iw
    kw = dict(col_map=cmap.to(DEV), iw_store=iws) if compact else {}
    row_tab, col_tab = eng.op_sample("readout_tables", [], in_hw=(ih, iw), out_hw=(oh, ow), nearest=bool(near), **kw)
    for tab, n_in, n_out, pitch, cm in ((row_tab, ih, oh, iws * 128, None), (col_tab, iw, ow, 128, cmap if compact else None)):
        tab = tab.cpu()
        off, wgt = tab[:, :4].long(), torch.from_numpy(tab[:, 4:].contiguous().numpy().view(np.float32)).double()
        idx, want = S.readout_taps(n_in, n_out, bool(near))
        inside = (idx >= 0) & (idx < n_in)
        stored = idx.clamp(0, n_in - 1) if cm is None else cm.long()[idx.clamp(0, n_in - 1)]
        live = inside & (want != 0)
        assert bool((stored[live] >= 0).all())
        eff = torch.where(off >= 0, wgt, torch.zeros_like(wgt))
        tol = 3 * 2.0 ** -24 * 2 * n_in
        err = float((eff - torch.where(inside, want, torch.zeros_like(want))).abs().max())
        print(f"readout tables {geom} {'compact' if compact else 'dense'}: max weight error {err:.2e} (tolerance {tol:.2e}), {int(live.sum())} live taps")
        assert err <= tol
        assert torch.equal(off[live], stored[live] * pitch), (off, stored)
        assert bool((off[~inside & (wgt != 0)] == -1).all())  # a tap outside the image is marked, never clamped in
