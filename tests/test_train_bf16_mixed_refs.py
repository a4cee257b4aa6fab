"""The float64 reference of the bf16-mixed training convs (tests/mixed16_refs.py) on the cases of tests/test_gpu_train_bf16_mixed_ops.py
-- no GPU.  Three things make the GPU test's bound (train_op_refs.TOL = 1e-5 rel-RMS per tensor) mean something:

(a) the reference agrees with the model the engine's whole step is held to (`oracle.losses.training_operand_rounding`, run in float32
    on the same tensors): both round the same operands in the same passes, so they differ by float32 summation alone -- worst 7.4e-7
    (dweight, 3x3 64->64 61x93 nb4) over the cases without weight standardisation;
(b) its own noise floor: a weight-standardised layer rounds the fp32 standardised weight, and a float32 and a float64 standardisation
    can land on either side of a bf16 rounding boundary, one bf16 ulp apart.  Between the reference and its variant that standardises
    in the engine's float32 order y / dx move by at most 1.0e-6 / 1.1e-6 (3x3 128->64 ws 16x16 nb1, two flipped weights of
    73 728 -- the engine reads 1.08e-6 on that case and 1e-7 on the others; seven of the eight cases have no flip at all) -- under TOL / 4, so the inputs leave the bound to the engine;
(c) every mutant of the reference moves a compared tensor by more than 10 TOL: truncation instead of RNE 7.0e-3, an unrounded
    forward weight 1.7e-3, an unrounded x in the weight gradient 1.7e-3, the forward's channel rule on the data gradient 2.3e-3 (on
    the layers where the two rules differ, and exactly 0 elsewhere), no rounding at all 2.4e-3.  Swapping the reference of the GPU test for any of them fails it.
"""
import pytest
import torch

from oracle import losses
from tests import mixed16_refs as M
from tests import train_op_refs as T
from tests.helpers import rel_rms

_CASES = {}


def case_of(args):
    if args not in _CASES:
        c = T.build("conv", args)
        _CASES[args] = (c, M.reference(c))
    return _CASES[args]


ALL = M.all_cases()
PLAIN = [(cid, a) for cid, a in ALL if not a[5]]
WS = [(cid, a) for cid, a in ALL if a[5] and all(losses.conv_operand_rules(a[3], a[4]))]
# the mutants are shown on small cases: one layer all three passes of which round, a weight-standardised one, a strided one and the
# mixed-rule layers
MUTANT_CASES = [(cid, a) for cid, a in ALL if a[7:10] == (11, 13, 3) and (a[3], a[4]) in ((128, 64), (64, 64), (96, 64), (64, 96), (64, 40))]


def test_the_case_lists_hold_what_the_gpu_test_states():
    assert len(M.MFMA) == 16 and all(a[3] % 16 == 0 and a[4] % 64 == 0 for _, a in M.MFMA)
    assert [(a[3], a[4]) for _, a in M.MIXED[::2]] == list(M.MIXED_RULES)
    for (ci, co), rules in M.MIXED_RULES.items():
        assert losses.conv_operand_rules(ci, co) == rules, (ci, co)
    assert all(all(losses.conv_operand_rules(a[3], a[4])) for _, a in M.MFMA + [(c, a) for c, a, _ in M.SHAPES])
    assert WS and len(MUTANT_CASES) >= 6


def test_rounding_helpers():
    t = torch.tensor([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -23, 2 - 2.0 ** -23, -(1 + 3 * 2.0 ** -8), 2.0 ** 40, 2.0 ** -40])
    assert M.bf16_rne(t).tolist() == [1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, 2.0, -(1 + 2.0 ** -6), 2.0 ** 40, 2.0 ** -40]
    assert M.bf16_truncate(t).tolist() == [1.0, 1 + 2.0 ** -7, 1.0, 2 - 2.0 ** -7, -(1 + 2.0 ** -7), 2.0 ** 40, 2.0 ** -40]
    g = torch.randn(4096, generator=torch.Generator().manual_seed(3))
    assert torch.equal(M.bf16_rne(M.bf16_truncate(g)), M.bf16_truncate(g))  # truncated values are bf16 values


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in PLAIN])
def test_a_reference_agrees_with_the_oracle_model_of_the_mode(args, request):
    case, want = case_of(args)
    got = M.oracle_model(case)
    assert sorted(got) == sorted(want)
    errs = {k: rel_rms(got[k], want[k]) for k in want}
    print(f"oracle.losses model in float32 vs mixed16 reference, {request.node.callspec.id}: {errs}")
    assert max(errs.values()) <= T.TOL, errs


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in ALL if a in M.ACCUMULATE])
def test_a_reference_accumulates_onto_incoming_parameter_gradients(args):
    case, want = case_of(args)
    gin = [torch.randn(p.shape, generator=torch.Generator().manual_seed(11)) for p in case.params]
    got = M.reference(case, grads_in=gin)
    assert torch.equal(got["y"], want["y"]) and torch.equal(got["dx"], want["dx"])
    for name, g in zip(case.p_names, gin):
        assert torch.equal(got["d" + name], want["d" + name] + g.double())


def _floor(args, fp32_as):
    """(rel-RMS of y and dx between the reference and its variant with a float32 standardisation, flipped bf16 weights)."""
    case, want = case_of(args)
    other = M.reference(case, ws_fp32_as=fp32_as)
    w = case.params[0].double()
    flips = int((M.bf16_rne(M.standardise(w)) != M.bf16_rne(M.standardise(w, fp32_as))).sum())
    return {k: rel_rms(other[k], want[k]) for k in ("y", "dx")}, flips


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in WS])
def test_b_standardised_weights_leave_the_bound_to_the_engine(args, request):
    """A condition on the INPUTS, not a measurement of the engine: how far the reference itself moves when the standardised weight is
    computed in float32 the way the engine's kernel does (M.standardise "engine") instead of in float64.  A weight a hair from a bf16
    rounding boundary flips by one bf16 ulp; every weight-standardised case must keep that under a quarter of the bound."""
    errs, flips = _floor(args, "engine")
    print(f"engine-order float32 vs float64 standardisation, {request.node.callspec.id}: {errs}, {flips} flipped weights")
    assert max(errs.values()) <= T.TOL / 4, errs


@pytest.mark.parametrize("args", [pytest.param(a, id=cid) for cid, a in WS if a[3:5] + a[7:10] in ((128, 64, 16, 16, 3), (64, 64, 11, 13, 3))])
def test_b_the_same_with_every_step_in_float32(args, request):
    """The variant whose statistics are float32 sums too (torch's own order), on the two cases the bound was planned with.  It is not
    what the engine computes -- its kernel sums in fp64 -- and on `k3s1p1-128to64-ws-11x13-nb1` it flips ONE weight of 73 728, a large
    one (-0.4717), which alone moves y / dx by 7.5e-6 / 6.9e-6; the engine's order flips none there (printed for all cases)."""
    for cid, a in WS:
        print(f"all-float32 vs float64 standardisation, {cid}: {_floor(a, 'torch')}")
    errs, _ = _floor(args, "torch")
    assert max(errs.values()) <= T.TOL / 4, errs


@pytest.mark.parametrize("mutant", M.MUTANTS)
def test_c_every_mutant_is_visible(mutant):
    seen = {}
    for cid, args in MUTANT_CASES:
        case, want = case_of(args)
        got = M.reference(case, mutant=mutant)
        seen[cid] = {k: rel_rms(got[k], want[k]) for k in want if k != "dbias"}
        assert torch.equal(got["dbias"], want["dbias"])  # a plain sum of dz whatever the operands do
    for cid, errs in seen.items():
        print(f"mutant {mutant}, {cid}: " + ", ".join(f"{k} {v:.2e}" for k, v in errs.items()))
    worst = max(max(e.values()) for e in seen.values())
    assert worst >= 10 * T.TOL, seen
    if mutant == "dgrad_uses_fwd_rule":  # invisible where all three passes round: a mixed-rule layer has to catch it
        mixed = {cid: e for (cid, a), e in zip(MUTANT_CASES, seen.values()) if not all(losses.conv_operand_rules(a[3], a[4]))}
        assert mixed and max(e["dx"] for e in mixed.values()) >= 10 * T.TOL, mixed
        assert all(max(e.values()) == 0 for cid, e in seen.items() if cid not in mixed), seen
