"""The references and the bound of tests/test_gpu_sample_ops.py, on the CPU (tests/sample_op_refs.py).

1. The reference alone sits well inside the bound: every listed case, evaluated in fp32 torch and rounded ONCE to the 16-bit type, has
   excess <= floor / 2 (fp32 outputs: rel-RMS <= TOL / 2; copies: equal) -- for bf16 and for fp16.  A case that does not gets other
   inputs, never a looser bound.
2. The bound tells wrong from right: every (case, mutant) pair of S.MUTANTS -- at least one case per kernel form for each mistake a kernel
   here could make -- rounded once, has excess > floor in BOTH types.  S.INVISIBLE lists pairs the bound cannot see at that shape (one
   pixel of 8281 against the bf16 floor, eps next to a variance of order one): they are printed, not asserted.
"""
import pytest
import torch

from tests import sample_op_refs as S
from tests.helpers import rel_rms

ALL = [pytest.param(op, cid, args, id=f"{op}-{cid}") for op in S.OPS for cid, args in S.specs(op)]


def _case(op, cid):
    return dict(S.specs(op))[cid]


def test_round16_rounds_once_to_nearest_even():
    for dt, ulp1 in ((torch.bfloat16, 2.0 ** -7), (torch.float16, 2.0 ** -10)):
        one = torch.tensor([1.0], dtype=torch.float64)
        assert float(S.round16(one + 0.5 * ulp1, dt)) == 1.0                 # a tie goes to the even neighbour ...
        assert float(S.round16(one + 1.5 * ulp1, dt)) == 1.0 + 2 * ulp1
        # ... and a value just above a tie goes up, although rounding through fp32 first lands ON the tie and then goes down
        assert float(S.round16(one + 0.5 * ulp1 + 2.0 ** -40, dt)) == 1.0 + ulp1
        assert float(S.round16(one + 0.5 * ulp1 - 2.0 ** -40, dt)) == 1.0
        x = torch.randn(4096, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
        assert torch.equal(S.round16(x.to(dt).double(), dt), x.to(dt))       # values of the type are kept
        assert float((S.round16(x, dt).double() - x).abs().max()) <= float((x.float().to(dt).double() - x).abs().max())


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
@pytest.mark.parametrize("op,cid,args", ALL)
def test_fp32_reference_sits_inside_half_the_bound(op, cid, args, dtname):
    b = S.build(op, args, dtname)
    dt = S.DTYPES[dtname]
    ref, f32 = b.ref(), b.ref(torch.float32)
    assert ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
    if b.kind == "exact":
        assert torch.equal(S.round16(f32.double(), dt), S.round16(ref, dt))
    elif b.kind == "f32":
        err = rel_rms(f32, ref)
        print(f"sample-op ref {op} {cid} {dtname}: fp32 torch rel-RMS {err:.3e}")
        assert err <= S.TOL_F32 / 2
    else:
        excess, floor = S.excess_floor(S.round16(f32.double(), dt), ref, dt)
        print(f"sample-op ref {op} {cid} {dtname}: fp32 torch excess {excess:.3e}, floor {floor:.3e}")
        assert floor > 0.0 and excess <= floor / 2


def _mutant_excess(op, cid, mutant, dtname):
    b = S.build(op, _case(op, cid), dtname)
    dt = S.DTYPES[dtname]
    ref, bad = b.ref(), b.ref(mutant=mutant)
    if b.kind == "f32":
        return rel_rms(bad, ref), S.TOL_F32
    return S.excess_floor(S.round16(bad, dt), ref, dt)


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
@pytest.mark.parametrize("op,cid,mutant", [pytest.param(op, c, m, id=f"{op}-{c}-{m}") for op, pairs in S.MUTANTS.items() for c, m in pairs])
def test_bound_tells_a_mutant_from_the_reference(op, cid, mutant, dtname):
    excess, floor = _mutant_excess(op, cid, mutant, dtname)
    print(f"sample-op mutant {op} {cid} {mutant} {dtname}: excess {excess:.3e}, floor {floor:.3e}")
    assert excess > floor


@pytest.mark.parametrize("op,cid,mutant", [pytest.param(op, c, m, id=f"{op}-{c}-{m}") for op, pairs in S.INVISIBLE.items() for c, m in pairs])
def test_mutants_the_bound_cannot_see_at_a_shape_are_said_so(op, cid, mutant):
    """Not an assertion about the kernels: these pairs are why the sensitivity list names other shapes for the same mutant."""
    for dtname in ("bf16", "fp16"):
        excess, floor = _mutant_excess(op, cid, mutant, dtname)
        print(f"sample-op mutant {op} {cid} {mutant} {dtname}: excess {excess:.3e} against floor {floor:.3e}: "
              f"{'invisible at this shape' if excess <= floor else 'visible'}")
    assert any(m == mutant and c != cid for c, m in S.MUTANTS[op])  # the mutant is held at another shape


def test_every_op_and_form_has_a_sensitivity_case():
    listed = {(op, m) for op, pairs in S.MUTANTS.items() for _, m in pairs}
    for need in [("gn_act", "last_pixel"), ("gn_act", "slot_dropped"), ("gn_act", "unbiased"), ("gn_act", "no_eps"), ("gn_act", "film_shift"),
                 ("gn_act", "residual_before_drop"), ("layernorm_c", "unbiased"), ("layernorm_c", "no_eps"), ("groupnorm_f32", "last_pixel"),
                 ("groupnorm_f32", "unbiased"), ("groupnorm_f32", "no_eps"), ("groupnorm_f32", "film_shift"), ("up2_bilinear", "border_mirrored"),
                 ("up2_bilinear", "second_source_shift8"), ("up2_epilogue", "border_mirrored"), ("up2_epilogue", "film_shift"), ("stem_conv", "tap_dropped")]:
        assert need in listed, need
    for op, pairs in list(S.MUTANTS.items()) + list(S.INVISIBLE.items()):
        ids = dict(S.specs(op))
        assert all(c in ids for c, _ in pairs), op
