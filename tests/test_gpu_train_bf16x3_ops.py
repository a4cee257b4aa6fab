"""-m gpu: the training convolutions under `train_precision="bf16x3"` (dyf_train_set_precision(48)), ONE op at a time through the
training step's own launch code (dyf_op_train_f32), against float64 torch on the CPU -- cases, references and bound of
tests/test_gpu_train_ops.py (tests/train_op_refs.py: rel-RMS <= 1e-5 per tensor, the project's bound for fp32 kernels).

The convs the 16-bit dispatch takes stage every operand as hi = bf16(v), lo = bf16(v - hi) and sum a_lo b_hi + a_hi b_lo + a_hi b_hi
(csrc/train_gemm.hip t_gemm_mfma16<.., SPLIT>, csrc/train_halo16.hip in three accumulating passes).  The three-term arithmetic itself
sits at 4.5e-6 of float64, one term (bf16-mixed) at 2.4e-3 and a dropped cross term at 1.6e-3 (tests/test_train_bf16x3_host.py), so the
bound tells the mode from either; the same cases under precision 16 must EXCEED 1e-4 here (the discrimination check).

Shapes: every `-mfma` case of specs("conv"), and the shapes where the launch changes (SHAPES below).  The form log must name a `16x3`
form for forward, data gradient and weight gradient and no fp32 matrix-core form (`t_gemm_mfma<`).  A `valu` case is bitwise the op
under 32 (deterministic mode).  Parameter gradients accumulate onto random incoming values; a halo forward must not depend on what its output buffer held
(the passes after the first accumulate INTO it): op_train allocates its outputs with torch.empty, so the case is run a second time
right after NaN-filled tensors of the outputs' sizes were freed -- the caching allocator hands those blocks out again.  Deterministic
mode: bitwise repeatable, the bound still holds, `:det` forms only.
"""
import pytest
import torch

import dyffusion_amd as D
from tests import train_op_refs as T
from tests.gpu_common import DEV
from tests.helpers import rel_rms

pytestmark = pytest.mark.gpu

# (k, stride, pad, cin, cout, ws, bias, h, w, nb, var0)
MFMA = [(cid, a) for cid, a in T.specs("conv") if cid.endswith("-mfma")]
SHAPES = [
    ("1x1-128to64-11x13-nb3", (1, 1, 0, 128, 64, 0, 1, 11, 13, 3, 0), None),
    ("4x4s2-64to64-12x16-nb4", (4, 2, 1, 64, 64, 0, 1, 12, 16, 4, 0), None),       # even plane, too few tiles for the parity-class data gradient
    ("4x4s2-64to64-11x13-nb4", (4, 2, 1, 64, 64, 0, 1, 11, 13, 4, 0), None),       # odd plane: no parity classes at any size
    ("4x4s2-64to64-128x128-nb2", (4, 2, 1, 64, 64, 0, 1, 128, 128, 2, 0), ("p",)),  # 64 tiles per class: the parity-class data gradient from here
    ("3x3-64to64-32x32-nb4", (3, 1, 1, 64, 64, 0, 1, 32, 32, 4, 0), None),         # split-K forward / dgrad, pixel splits of the wgrad
    ("3x3-64to64-64x96-nb4", (3, 1, 1, 64, 64, 0, 1, 64, 96, 4, 0), ("fd", "w")),  # 192 tiles: the halo forward and dgrad from here
    ("3x3-64to64-61x93-nb4", (3, 1, 1, 64, 64, 0, 1, 61, 93, 4, 0), ("fd", "w")),  # the same tile count, ragged edges
    ("3x3-64to64-64x32-nb4", (3, 1, 1, 64, 64, 0, 1, 64, 32, 4, 0), ("w",)),       # 64 tiles: the halo weight gradient from here
    ("3x3-64to128-64x48-nb4", (3, 1, 1, 64, 128, 0, 1, 64, 48, 4, 0), ("f", "w")),  # two column blocks of the halo forward
]
HALO_FWD, HALO_WGRAD, TWO_BLOCKS, SPLITK = SHAPES[5], SHAPES[7], SHAPES[8], SHAPES[4]
VALU = ("3x3-24to40-ws-11x13-nb3", (3, 1, 1, 24, 40, 1, 1, 11, 13, 3, 0))
ACCUMULATE = [(3, 1, 1, 24, 40, 1, 1, 11, 13, 3, 0), (1, 1, 0, 128, 64, 0, 1, 11, 13, 3, 0), (7, 1, 3, 3, 8, 0, 1, 11, 13, 1, 0)]  # test_gpu_train_ops


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False)
    e.train_set_precision("bf16x3")
    assert e.train_precision == 48
    e.form_log(True)
    yield e
    e.form_log(False)
    e.close()


_REFS = {}


def reference(args, accumulate):
    """(case, float64 results, incoming parameter gradients) of a conv case: computed once, shared, never modified."""
    key = (args, accumulate)
    if key not in _REFS:
        case = T.build("conv", args)
        g = torch.Generator().manual_seed(11)
        gin = [torch.randn(p.shape, generator=g) for p in case.params] if accumulate else None
        _REFS[key] = (case, case.run(grads_in=gin), gin)
    return _REFS[key]


def run(eng, args, accumulate=False):
    """One op_train call of the case -> (results by name, form log of the call)."""
    case, _, gin = reference(args, accumulate)
    eng.form_log(True)  # clears
    r = eng.op_train(case.op, [t.to(DEV) for t in case.ins], case.params, case.dout.to(DEV), gin, **case.kw)
    forms = eng.form_log_read()
    got = {"y": r["y"].cpu(), "dx": r["dinputs"][0].cpu()}
    got.update({"d" + n: t for n, t in zip(case.p_names, r["dparams"])})
    return got, forms


def errors(got, args, accumulate=False):
    _, want, _ = reference(args, accumulate)
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
    return {k: rel_rms(got[k].reshape(w.shape), w) for k, w in want.items()}


def held(eng, args, cid, accumulate=False):
    """The case under the engine's current setting, held to the fp32 bound; -> (results, forms)."""
    got, forms = run(eng, args, accumulate)
    errs = errors(got, args, accumulate)
    worst = max(errs, key=errs.get)
    print(f"bf16x3 conv {cid}: max err {errs[worst]:.3e} ({worst}); forms {sorted(forms)}")
    assert errs[worst] <= T.TOL, errs
    return got, forms


def split_forms_only(forms, halo=()):
    names = sorted(forms)
    fwd = [k for k in names if "16x3" in k and "forward" in k]
    dgr = [k for k in names if "16x3" in k and "dgrad" in k]
    wgr = [k for k in names if "16x3" in k and "wgrad" in k]
    assert fwd and dgr and wgr, names
    assert not any(k.startswith("t_gemm_mfma<") for k in names), names
    if "f" in halo or "fd" in halo:
        assert "t_halo3x3_16x3:forward" in names, names
    if "fd" in halo:
        assert "t_halo3x3_16x3:dgrad" in names, names
    if "p" in halo:
        assert "t_gemm_mfma16x3:dgrad_parity" in names, names
    if "w" in halo:
        assert "t_wgrad3x3_16x3" in names and "t_wgrad3x3_16x3:atomic" in names, names


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in MFMA])
def test_matrix_core_cases_hold_the_fp32_bound_on_the_split_forms(eng, args, request):
    _, forms = held(eng, args, request.node.callspec.id)
    split_forms_only(forms)


@pytest.mark.parametrize("args,halo", [pytest.param(a, hl or (), id=cid) for cid, a, hl in SHAPES])
def test_shapes_where_the_launch_changes(eng, args, halo, request):
    _, forms = held(eng, args, request.node.callspec.id)
    split_forms_only(forms, halo)


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in MFMA + [(c, a) for c, a, _ in SHAPES]])
def test_bf16_mixed_operands_miss_the_bound_on_the_same_cases(eng, args, request):
    """The discrimination check: one bf16 term per product is two orders above the bound on every compared product."""
    eng.train_set_precision(16)
    try:
        got, forms = run(eng, args)
    finally:
        eng.train_set_precision("bf16x3")
    errs = errors(got, args)
    errs.pop("dbias", None)  # a plain fp32 sum of dz in every mode
    print(f"bf16-mixed conv {request.node.callspec.id}: min err {min(errs.values()):.3e}; forms {sorted(forms)}")
    assert not any("16x3" in k for k in forms), sorted(forms)
    assert min(errs.values()) > 1e-4, errs


def test_a_conv_outside_the_channel_rules_is_the_fp32_op_bit_for_bit(eng):
    """In the deterministic mode, where the same op twice is bitwise equal at all (the default weight gradient merges with atomics)."""
    cid, args = VALU
    eng.train_set_deterministic(True)
    try:
        got, forms = held(eng, args, cid)
        eng.train_set_precision(32)
        ref, _ = run(eng, args)
    finally:
        eng.train_set_precision("bf16x3")
        eng.train_set_deterministic(False)
    assert not any("16x3" in k for k in forms), sorted(forms)
    assert all(torch.equal(got[k], ref[k]) for k in ref), [k for k in ref if not torch.equal(got[k], ref[k])]


@pytest.mark.parametrize("args", ACCUMULATE + [HALO_WGRAD[1]], ids=lambda a: "-".join(str(v) for v in a))
def test_parameter_gradients_accumulate(eng, args, request):
    """The gradient buffers hold random values when the op runs: the result is incoming + gradient, through every pass."""
    _, forms = held(eng, args, request.node.callspec.id, accumulate=True)
    if args == HALO_WGRAD[1]:
        assert "t_wgrad3x3_16x3" in forms, sorted(forms)


def test_a_halo_forward_does_not_depend_on_what_its_buffers_held(eng):
    cid, args, _ = HALO_FWD
    first, forms = held(eng, args, cid)
    assert "t_halo3x3_16x3:forward" in forms and "t_halo3x3_16x3:dgrad" in forms, sorted(forms)
    # dirty the blocks torch.empty will hand to the next call's y and dx: NaN survives any accumulation
    junk = [torch.full(first[k].shape, float("nan"), device=DEV) for k in ("y", "dx") for _ in range(2)]
    torch.cuda.synchronize()
    del junk
    again, _ = held(eng, args, cid + " (dirty buffers)")
    assert torch.equal(first["y"], again["y"]) and torch.equal(first["dx"], again["dx"])
    # and another op in between: recycled pool memory of the engine's own buffers
    held(eng, TWO_BLOCKS[1], TWO_BLOCKS[0])
    third, _ = held(eng, args, cid + " (after another op)")
    assert torch.equal(first["y"], third["y"]) and torch.equal(first["dx"], third["dx"])


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a, _ in (SPLITK, HALO_WGRAD)])
def test_deterministic_mode_is_repeatable_and_free_of_atomics(eng, args, request):
    eng.train_set_deterministic(True)
    try:
        a, forms = held(eng, args, request.node.callspec.id + "-det")
        b, _ = run(eng, args)
    finally:
        eng.train_set_deterministic(False)
    names = sorted(forms)
    assert any(k.endswith(":det") for k in names) and not any(k.endswith(":atomic") for k in names), names
    assert any("16x3" in k and "wgrad" in k and k.endswith(":det") for k in names), names
    assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]


def test_form_switch_selects_the_split_forms_for_an_engine_that_did_not_say(form_switch):
    """DYF_TRAIN_OPERANDS=bf16x3 is to 48 what =bf16 is to 16: read for engines at precision 0 only; a set precision wins."""
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False)
    cid, args, _ = SHAPES[0]
    try:
        assert e.train_precision == 0
        form_switch.setenv("DYF_TRAIN_OPERANDS", "bf16x3")
        _, forms = held(e, args, cid + " (form switch)")
        split_forms_only(forms)
        took = [e.train_conv_check(kind, args[9], args[7], args[8], args[3], args[4], args[0], args[1], args[2]) for kind in (0, 1, 2)]
        print(f"conv_check under the switch (rel max err with / without workspace, took): {took}")
        # unrounded operands against the fp32 VALU kernels, max |difference| / max |reference|: a product is off by at most 3 * 2^-17 = 2.3e-5
        # of itself (two roundings to 16 bits and the dropped lo x lo term), a sum by less relative to its largest element; pre-rounded or
        # one-term operands would read 2^-9 = 2e-3
        assert all(t[2] and max(t[0], t[1]) <= 5e-5 for t in took), took
        e.train_set_precision(32)
        _, forms = held(e, args, cid + " (form switch, engine set to 32)")
        assert not any("16x3" in k for k in forms), sorted(forms)
        e.train_set_precision("bf16x3")
        form_switch.setenv("DYF_TRAIN_OPERANDS", "bf16")  # the other way round: 48 does not read the switch either
        _, forms = held(e, args, cid + " (engine set to 48, switch says bf16)")
        split_forms_only(forms)
        with pytest.raises(Exception):
            e._check(e._lib.dyf_train_set_precision(e._h, 8))
        assert e.train_precision == 48
    finally:
        e.form_log(False)
        e.close()
