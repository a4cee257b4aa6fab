"""The references and the bound of tests/test_gpu_sample_ops.py, on the CPU (tests/sample_op_refs.py).

1. The reference alone sits well inside the bound: every listed case, evaluated in fp32 torch and rounded ONCE to the 16-bit type, has
   excess <= floor / 2 (fp32 outputs: rel-RMS <= TOL / 2; copies: equal) -- for bf16 and for fp16.  A case that does not gets other
   inputs, never a looser bound.
2. The bound tells wrong from right: every (case, mutant) pair of S.MUTANTS -- at least one case per kernel form for each mistake a kernel
   here could make -- rounded once, has excess > floor in BOTH types.  S.INVISIBLE lists pairs the bound cannot see at that shape (one
   pixel of 8281 against the bf16 floor, eps next to a variance of order one): they are printed, not asserted.
3. The launchers around the networks (readout, stems, time MLP, FiLM, sampler kernels; an op may have several outputs, each with its own
   kind): the same two properties, and the statements the GPU file leans on -- the 16-tap readout stencil equals conv_transpose2d + resample,
   every nearest geometry floors in fp32 as it does exactly, compact cases really store fewer columns, the row-key table of a forward start.
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
    refs, f32s = S.outputs(b.ref()), S.outputs(b.ref(torch.float32))
    kinds = S.outputs(b.kind) if len(refs) > 1 else [b.kind if isinstance(b.kind, str) else b.kind[0]]
    assert len(refs) == len(f32s) == len(kinds)
    for ref, f32, kind in zip(refs, f32s, kinds):
        if kind == "eq":
            assert not ref.dtype.is_floating_point and torch.equal(ref, f32)
            continue
        assert ref.dtype == torch.float64 and bool(torch.isfinite(ref).all())
        if kind == "exact":
            assert torch.equal(S.round16(f32.double(), dt), S.round16(ref, dt))
        elif kind == "f32":
            err = rel_rms(f32, ref)
            print(f"sample-op ref {op} {cid} {dtname}: fp32 torch rel-RMS {err:.3e}")
            assert f32.dtype == torch.float32 and err <= S.TOL_F32 / 2
        else:
            excess, floor = S.excess_floor(S.round16(f32.double(), dt), ref, dt)
            print(f"sample-op ref {op} {cid} {dtname}: fp32 torch excess {excess:.3e}, floor {floor:.3e}")
            assert floor > 0.0 and excess <= floor / 2


def _mutant_excess(op, cid, mutant, dtname):
    b = S.build(op, _case(op, cid), dtname)
    dt = S.DTYPES[dtname]
    refs, bads = S.outputs(b.ref()), S.outputs(b.ref(mutant=mutant))
    kinds = S.outputs(b.kind) if len(refs) > 1 else [b.kind if isinstance(b.kind, str) else b.kind[0]]
    seen = []  # an op with several outputs: the output that shows the mistake most
    for ref, bad, kind in zip(refs, bads, kinds):
        if kind == "f32":
            seen.append((rel_rms(bad, ref), S.TOL_F32))
        elif kind != "eq":
            seen.append(S.excess_floor(S.round16(bad, dt), ref, dt))
    return max(seen, key=lambda ef: ef[0] / ef[1])


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
                 ("up2_bilinear", "second_source_shift8"), ("up2_epilogue", "border_mirrored"), ("up2_epilogue", "film_shift"), ("stem_conv", "tap_dropped"),
                 ("readout", "border_mirrored"), ("readout", "border_clamped"), ("readout", "parity_swapped"), ("readout", "not_flipped"),
                 ("readout", "no_bias"), ("readout", "col_map_ignored"), ("stem", "second_source_offset"), ("stem", "src_rows_ignored"),
                 ("stem", "no_bias"), ("stem16", "second_source_offset"), ("stem16", "src_rows_ignored"), ("stem16", "no_bias_slot"),
                 ("film", "rows_swapped"), ("film", "blk_off_single"), ("time_mlp", "tanh_gelu"), ("time_mlp", "sincos_swapped"),
                 ("time_mlp", "half_for_half_minus_1"), ("noisy_condition", "same_field_twice")]:
        assert need in listed, need
    for op, pairs in list(S.MUTANTS.items()) + list(S.INVISIBLE.items()):
        ids = dict(S.specs(op))
        assert all(c in ids for c, _ in pairs), op


# ------------------------------------------------------------------------------------------- the launchers around the networks
def test_readout_stencil_is_the_transposed_conv_and_the_resample():
    """The 16-tap stencil (S.readout_taps: what the tap tables are compared with, and what the readout mutants edit) IS
    conv_transpose2d(k4, s2, p1) followed by the resample, on every case small enough to gather."""
    n = 0
    for cid, args in S.specs("readout"):
        b = S.build("readout", args, "bf16")
        if not b.stencil:
            continue
        assert rel_rms(b.ref(mutant="stencil"), b.ref()) <= 1e-14, cid  # ("stencil": the other statement, nothing edited)
        n += 1
    assert n >= 60


def test_nearest_geometries_floor_as_the_kernel_floors():
    """bilinear_coord floors dst * scale in fp32: every nearest case here has that floor equal to the exact floor(dst n_in / n_out), and
    the float64 / fp32 resample matrices of the references pick those indices too."""
    from tests import train_op_refs as T
    seen = set()
    for op in ("readout", "stem", "stem16"):
        for cid, a in S.specs(op):
            if not a.get("nearest"):
                continue
            pairs = [(2 * a["ih"], a["oh"]), (2 * a["iw"], a["ow"])] if op == "readout" else [(a["h"], a["uh"]), (a["w"], a["uw"])]
            for n_in, n_out in pairs:
                seen.add((n_in, n_out))
                assert S.nearest_floor_is_exact(n_in, n_out), (op, cid, n_in, n_out)
                want = (torch.arange(n_out) * n_in) // n_out
                for dtype in (torch.float64, torch.float32):
                    assert torch.equal(T._resample_matrix(n_in, n_out, True, dtype).argmax(1), want), (op, cid, dtype)
    assert len(seen) >= 8
    assert not S.nearest_floor_is_exact(26, 22)  # (what the check is for: 11 * fl(26 / 22) in fp32 lands just under 13)


def test_compact_cases_store_fewer_columns_than_the_decoder_has():
    for cid, a in S.specs("readout"):
        if a.get("compact"):
            used, cmap = S.readout_columns(a["iw"], a["ow"], bool(a.get("nearest")))
            b = S.build("readout", a, "bf16")
            assert 0 < len(used) < a["iw"] and b.xs[0].shape[2] == len(used) and int((cmap >= 0).sum()) == len(used), cid
            assert sorted(int(v) for v in cmap[cmap >= 0]) == list(range(len(used)))


def test_begin_keys_follow_the_forward_and_row_of_every_launch_row():
    keys, state = S.begin_keys(2, 5, 5, 2)
    k = keys.numpy().view("uint32")
    from tests import rng_host as R
    assert tuple(k[4]) == tuple(int(v) for v in R.row_key(S.SEED, 4, 5)) and tuple(k[3]) == tuple(int(v) for v in R.row_key(S.SEED, 3, 6))
    assert state.numpy().view("uint32")[2] == 5 and len({tuple(r) for r in k}) == 5
