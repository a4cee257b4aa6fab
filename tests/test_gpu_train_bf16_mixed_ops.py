"""-m gpu: the training convolutions under `train_precision="bf16-mixed"` (dyf_train_set_precision(16)), ONE op at a time through the
training step's own launch code (dyf_op_train_f32), against the float64 operand-rounding reference of tests/mixed16_refs.py: the same
operands rounded to bf16 (RNE) in the same passes (`oracle.losses.conv_operand_rules`), everything else in float64.  Products of two
bf16 values are exact in fp32, so the engine differs from that reference by its fp32 summation order alone and the project's bound for
fp32 kernels applies unchanged: rel-RMS <= train_op_refs.TOL = 1e-5 on every returned tensor.  The mode itself sits 2.3e-3 from
unrounded float64, truncation instead of RNE 7.0e-3 from the reference, one unrounded operand 1.7e-3, a pass on the wrong channel rule
2.3e-3 (tests/test_train_bf16_mixed_refs.py): the bound separates "bf16-mixed done right" from each by two orders of magnitude.

Cases (tests/mixed16_refs.py): every `-mfma` case of specs("conv") -- bias, weight standardisation, stride 2; the shapes where the
launch changes (split-K, the halo forward / data gradient / weight gradient of csrc/train_halo16.hip, ragged planes, two column
blocks, the parity-class data gradient); layers where only SOME of the three passes take the 16-bit form; parameter gradients
accumulated onto random incoming values; the deterministic forms; the fp16 build of the library (the operands are bf16 in both).
The form log is held per pass: a mode-16 form (`t_halo3x3_16:forward` / `:dgrad`, `t_wgrad3x3_16`, `t_gemm_mfma16<forward | dgrad |
wgrad>`, `t_gemm_mfma16:dgrad_parity`) exactly where the channel rules give the pass to 16 bit, the halo forms exactly at the shapes
that reach them, no `16x3` form, no fp32 `t_gemm_mfma<` form for a 16-bit pass.

Bitwise operand probes, no tolerance: with identity weights y == bf16(x) and dx == bf16(dz); a one-hot x (dz) reads bf16(w) out of
the forward (data gradient), all nine taps of a 3x3 from a single unit pixel, which pins the tap orientation too; a one-hot dz (x)
reads bf16(x) (bf16(dz)) out of the weight gradient.  Every other product is an exact zero, so the result does not depend on the
summation order, split-K or atomics.  The probed operand holds exact ties both ways, one fp32 ulp either side of a tie, a mantissa
carry, negatives, 2^40 and 2^-40 multiples (outside fp16's range) and randn -- no NaN, Inf or subnormals (their products with zero
are not zero).

Measured on the MI355X (worst rel-RMS of any tensor per group): the `-mfma` cases 1.3e-7, but 1.08e-6 (dx) on `k3s1p1-128to64-ws-16x16-nb1`,
where two of 73 728 standardised weights sit so close to a bf16 rounding boundary that the engine's fp32 standardisation and the
float64 one round them apart -- the 1.07e-6 tests/test_train_bf16_mixed_refs.py predicts for that case from the inputs alone; the
launch-change shapes 4.0e-7; the mixed-rule layers 6.2e-7 (dbias of 64->1); accumulation 3.3e-7, deterministic 2.0e-7; the fp16 build
4.6e-7; the form switches 4.2e-7.  The probes: 0 differing elements of every tensor, both shapes, both builds.  49 tests in 4 s.
"""
import pytest
import torch

import dyffusion_amd as D
from oracle import losses
from tests import mixed16_refs as M
from tests import train_op_refs as T
from tests.gpu_common import DEV
from tests.helpers import rel_rms

pytestmark = pytest.mark.gpu

FWD16 = {"t_halo3x3_16:forward", "t_gemm_mfma16<forward>"}
DGRAD16 = {"t_halo3x3_16:dgrad", "t_gemm_mfma16<dgrad>", "t_gemm_mfma16:dgrad_parity"}
WGRAD16 = {"t_wgrad3x3_16", "t_gemm_mfma16<wgrad>:atomic", "t_gemm_mfma16<wgrad>:det"}


def _engine(dtype="bf16", precision=16):
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False, dtype=dtype)
    if precision:
        e.train_set_precision(precision)
        assert e.train_precision == precision
    return e


@pytest.fixture(scope="module")
def eng():
    e = _engine()
    yield e
    e.form_log(False)
    e.close()


@pytest.fixture(scope="module")
def eng_f16():
    """The fp16 build of the library: its training operands are bf16 all the same (csrc/train_internal.h)."""
    e = _engine("fp16")
    yield e
    e.form_log(False)
    e.close()


@pytest.fixture(params=["bf16", "fp16"])
def either(request, eng, eng_f16):
    return eng if request.param == "bf16" else eng_f16


_REFS = {}


def reference(args, accumulate=False):
    """(case, float64 operand-rounding reference, incoming parameter gradients) of a conv case: computed once, shared, never modified."""
    key = (args, accumulate)
    if key not in _REFS:
        case = T.build("conv", args)
        g = torch.Generator().manual_seed(11)
        gin = [torch.randn(p.shape, generator=g) for p in case.params] if accumulate else None
        _REFS[key] = (case, M.reference(case, grads_in=gin), gin)
    return _REFS[key]


def op(eng, case, gin=None):
    """One op_train call -> (results by name on the CPU, form log of the call)."""
    eng.form_log(True)  # clears
    r = eng.op_train(case.op, [t.to(DEV) for t in case.ins], case.params, case.dout.to(DEV), gin, **case.kw)
    forms = eng.form_log_read()
    got = {"y": r["y"].cpu(), "dx": r["dinputs"][0].cpu()}
    got.update({"d" + n: t for n, t in zip(case.p_names, r["dparams"])})
    return got, forms


def held(eng, args, cid, accumulate=False):
    """The case under the engine's current setting, every tensor finite and held to the fp32 bound; -> (results, forms)."""
    case, want, gin = reference(args, accumulate)
    got, forms = op(eng, case, gin)
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
    errs = {k: rel_rms(got[k].reshape(w.shape), w) for k, w in want.items()}
    worst = max(errs, key=errs.get)
    print(f"bf16-mixed conv {cid}: max err {errs[worst]:.3e} ({worst}); forms {sorted(forms)}")
    assert errs[worst] <= T.TOL, errs
    return got, forms


def forms_follow_the_rules(forms, args, marks=None):
    """Per pass: a mode-16 form ran exactly when the channel rules give the pass to 16 bit.  `marks` (a SHAPES entry): the halo / parity
    forms the shape must reach -- and it must reach no other: the implicit-GEMM form takes the remaining passes."""
    names = set(forms)
    f16, d16, w16 = losses.conv_operand_rules(args[3], args[4])
    assert bool(names & FWD16) == f16 and bool(names & DGRAD16) == d16 and bool(names & WGRAD16) == w16, sorted(names)
    assert not any("16x3" in k for k in names), sorted(names)
    if w16:
        assert not any(k.startswith("t_gemm_mfma<wgrad>") for k in names), sorted(names)
    if f16 and d16 and w16:
        assert not any(k.startswith("t_gemm_mfma<") for k in names), sorted(names)
    if marks is not None:
        assert f16 and d16 and w16
        assert ("t_halo3x3_16:forward" in names) == ("f" in marks or "fd" in marks), sorted(names)
        assert ("t_gemm_mfma16<forward>" in names) != ("t_halo3x3_16:forward" in names), sorted(names)
        assert ("t_halo3x3_16:dgrad" in names) == ("fd" in marks) and ("t_gemm_mfma16:dgrad_parity" in names) == ("p" in marks), sorted(names)
        assert ("t_gemm_mfma16<dgrad>" in names) == ("fd" not in marks and "p" not in marks), sorted(names)
        assert ("t_wgrad3x3_16" in names) == ("t_wgrad3x3_16:atomic" in names) == ("w" in marks), sorted(names)
        assert ("t_gemm_mfma16<wgrad>:atomic" in names) == ("w" not in marks), sorted(names)


# ---------------------------------------------------------------------------------------------------------------- (i) - (iii)
@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in M.MFMA])
def test_matrix_core_cases_hold_the_fp32_bound_against_rounded_operands(eng, args, request):
    _, forms = held(eng, args, request.node.callspec.id)
    forms_follow_the_rules(forms, args, marks=())  # planes of 11 x 13 and 16 x 16: the implicit-GEMM forms throughout


@pytest.mark.parametrize("args,marks", [pytest.param(a, mk or (), id=cid) for cid, a, mk in M.SHAPES])
def test_shapes_where_the_launch_changes(eng, args, marks, request):
    """The thresholds of thalo_conv3x3 / thalo_wgrad3x3 / the parity-class data gradient are those of the bf16x3 forms (they do not read the
    mode), so the shapes are the ones tests/test_gpu_train_bf16x3_ops.py runs."""
    _, forms = held(eng, args, request.node.callspec.id)
    forms_follow_the_rules(forms, args, marks)


def test_the_shapes_are_those_of_the_bf16x3_file():
    from tests import test_gpu_train_bf16x3_ops as X3
    assert M.SHAPES == X3.SHAPES and M.ACCUMULATE == X3.ACCUMULATE and M.MFMA == X3.MFMA


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in M.MIXED])
def test_layers_where_only_some_passes_are_16_bit(eng, args, request):
    """The dispatch of tgemm_conv_fwd / _dgrad / _wgrad IS the product; `conv_operand_rules` restates it for the step-level model.  Each
    pass is held to the rule twice: by the form log, and by the bound -- a pass rounded (or not) against the rule is 2e-3 away."""
    assert losses.conv_operand_rules(args[3], args[4]) == M.MIXED_RULES[(args[3], args[4])]
    _, forms = held(eng, args, request.node.callspec.id)
    forms_follow_the_rules(forms, args)


# ------------------------------------------------------------------------------------------------------------------------ (iv)
@pytest.mark.parametrize("args", M.ACCUMULATE + [M.HALO_WGRAD[1]], ids=lambda a: "-".join(str(v) for v in a))
def test_parameter_gradients_accumulate(eng, args, request):
    """The gradient buffers hold random values when the op runs: the result is incoming + gradient."""
    _, forms = held(eng, args, request.node.callspec.id, accumulate=True)
    forms_follow_the_rules(forms, args)
    if args == M.HALO_WGRAD[1]:
        assert "t_wgrad3x3_16" in forms, sorted(forms)


@pytest.mark.parametrize("args,wgrad", [pytest.param(M.SPLITK[1], "t_gemm_mfma16<wgrad>:det", id=M.SPLITK[0]),
                                        pytest.param(M.HALO_WGRAD[1], "t_wgrad3x3_16:det", id=M.HALO_WGRAD[0])])
def test_deterministic_mode_is_repeatable_and_free_of_atomics(eng, args, wgrad, request):
    eng.train_set_deterministic(True)
    try:
        a, forms = held(eng, args, request.node.callspec.id + "-det")
        case, _, _ = reference(args)
        b, _ = op(eng, case)
    finally:
        eng.train_set_deterministic(False)
    names = sorted(forms)
    forms_follow_the_rules(forms, args)
    assert wgrad in names and not any(k.endswith(":atomic") for k in names), names
    assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]


# ------------------------------------------------------------------------------------------------------------------------- (v)
@pytest.mark.parametrize("args,marks", [pytest.param(a, mk or (), id=cid) for cid, a, mk in M.FP16_BUILD])
def test_the_fp16_build_rounds_to_bf16_too(eng_f16, args, marks, request):
    _, forms = held(eng_f16, args, request.node.callspec.id + " (fp16 build)")
    forms_follow_the_rules(forms, args, marks)


def test_form_switches_reach_the_same_arithmetic(form_switch):
    """DYF_TRAIN_OPERANDS=bf16 gives an engine that did not say the mode-16 forms; DYF_TRAIN_HALO16=0 sends the halo shape to the
    tap-by-tap implicit GEMM, at a plane too large for split-K: the same reference, the same bound."""
    e = _engine(precision=0)
    cid, args, _ = M.HALO_FWD
    try:
        assert e.train_precision == 0
        form_switch.setenv("DYF_TRAIN_OPERANDS", "bf16")
        _, forms = held(e, args, cid + " (form switch)")
        forms_follow_the_rules(forms, args, M.HALO_FWD[2])
        form_switch.setenv("DYF_TRAIN_HALO16", "0")
        _, forms = held(e, args, cid + " (form switch, no halo forms)")
        forms_follow_the_rules(forms, args, ())
    finally:
        e.form_log(False)
        e.close()


# -------------------------------------------------------------------------------------------------------- bitwise operand probes
PROBES = [("1x1-64to64-11x13-nb3", (1, 1, 0, 64, 64, 0, 1, 11, 13, 3, 0), ()), ("3x3-64to64-64x96-nb4", M.HALO_FWD[1], M.HALO_FWD[2])]


def probe_values(shape, seed):
    """A tensor of `shape`: a third of it the values where a rounding goes wrong, the rest randn, shuffled."""
    u = 2.0 ** -23  # an fp32 ulp in [1, 2)
    base = [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8,                                         # exact ties: down to even, up to even
            1 + 2.0 ** -8 + u, 1 + 2.0 ** -8 - u, 1 + 3 * 2.0 ** -8 + u, 1 + 3 * 2.0 ** -8 - u,  # one fp32 ulp either side of a tie
            2 - u, 1.0, 1 + 2.0 ** -7, 0.0]                                           # a mantissa carry; exact bf16 values
    special = torch.tensor([s * v * m for v in base for s in (1.0, -1.0) for m in (1.0, 2.0 ** 40, 2.0 ** -40, 3.0)], dtype=torch.float32)
    g = torch.Generator().manual_seed(seed)
    n = int(torch.tensor(shape).prod())
    t = torch.randn(n, generator=g)
    k = n // 3
    t[:k] = special[torch.arange(k) % special.numel()]
    t = t[torch.randperm(n, generator=g)].reshape(shape)
    assert bool(torch.isfinite(t).all()) and float(t.abs().max()) < 2.0 ** 100
    assert bool(((t == 0) | (t.abs() > 2.0 ** -100)).all())  # no subnormals, before or after rounding
    return t


def one_hot(nb, h, w, c, k):
    """(nb, h, w, c) zeros with ONE unit pixel per channel, the pixels `k` apart (their k x k footprints disjoint) away from the plane's
    edge and spread over the whole batch."""
    lo = k // 2
    spots = [(n, r, q) for n in range(nb) for r in range(lo, h - lo, k) for q in range(lo, w - lo, k)]
    assert len(spots) >= c
    t = torch.zeros(nb, h, w, c)
    for ch in range(c):
        n, r, q = spots[ch * len(spots) // c]
        t[n, r, q, ch] = 1.0
    return t


_PROBES = {}


def probe_set(args):
    """The four probe calls of a shape, as (name, x, weight, dz, {result name: expected tensor}); the expectations are float64 torch
    convolutions of the ROUNDED probed operand with the one-hot one -- one non-zero product per element, so they are exact."""
    if args in _PROBES:
        return _PROBES[args]
    k, s, pd, ci, co, _, _, h, w, nb, _ = args
    assert s == 1 and ci == co
    nchw, nhwc, r16 = M._nchw, M._nhwc, M.bf16_rne
    eye = torch.zeros(co, ci, k, k)
    eye[torch.arange(co), torch.arange(ci), k // 2, k // 2] = 1.0
    xv, zv, wv = probe_values((nb, h, w, ci), 1), probe_values((nb, h, w, co), 2), probe_values((co, ci, k, k), 3)
    xh, zh = one_hot(nb, h, w, ci, k), one_hot(nb, h, w, co, k)
    zero_w = torch.zeros(co, ci, k, k)
    conv = lambda a, b: nhwc(torch.nn.functional.conv2d(nchw(a).double(), b.double(), None, stride=1, padding=pd)).float()
    dgrad = lambda z, b: nhwc(torch.nn.grad.conv2d_input((nb, ci, h, w), b.double(), nchw(z).double(), stride=1, padding=pd)).float()
    wgrad = lambda z, a: torch.nn.grad.conv2d_weight(nchw(a).double(), (co, ci, k, k), nchw(z).double(), stride=1, padding=pd).float()
    out = [
        ("identity weights: y = bf16(x), dx = bf16(dz)", xv, eye, zv, {"y": r16(xv), "dx": r16(zv)}),
        ("one-hot x and dz: y and dx read bf16(w)", xh, wv, zh, {"y": conv(xh, r16(wv)), "dx": dgrad(zh, r16(wv))}),
        ("one-hot dz: dweight reads bf16(x)", xv, zero_w, zh, {"dweight": wgrad(zh, r16(xv))}),
        ("one-hot x: dweight reads bf16(dz)", xh, zero_w, zv, {"dweight": wgrad(r16(zv), xh)}),
    ]
    # the one-hot probes do read every weight / a full footprint: as many non-zeros as the probed tensor has (its zeros apart)
    assert int((out[1][4]["y"] != 0).sum()) == int((out[1][4]["dx"] != 0).sum()) == int((r16(wv) != 0).sum())
    assert int((out[2][4]["dweight"] != 0).sum()) > 0.9 * wv.numel() and int((out[3][4]["dweight"] != 0).sum()) > 0.9 * wv.numel()
    _PROBES[args] = out
    return out


@pytest.mark.parametrize("args,marks", [pytest.param(a, mk, id=cid) for cid, a, mk in PROBES])
def test_staged_operands_are_bf16_rne_bit_for_bit(either, args, marks, request):
    k, _, pd, ci, co = args[:5]
    for name, x, wt, dz, want in probe_set(args):
        either.form_log(True)
        r = either.op_train("conv", [x.to(DEV)], [wt, torch.zeros(co)], dz.to(DEV), None, k=k, stride=1, pad=pd, ws=False)
        forms = either.form_log_read()
        forms_follow_the_rules(forms, args, marks)
        got = {"y": r["y"].cpu(), "dx": r["dinputs"][0].cpu(), "dweight": r["dparams"][0]}
        for key, w in want.items():
            g = got[key].reshape(w.shape)
            bad = int((g != w).sum())
            print(f"probe {request.node.callspec.id}, {name}: {key} {bad} of {w.numel()} elements differ")
            assert torch.equal(g, w), (name, key, bad, g[g != w][:8], w[g != w][:8])
