"""The reference, the cases and the mutants of tests/upconv_refs.py, on the CPU: (a) the operand model with unrounded taps IS
F.interpolate + F.conv2d in float64; (b) fp32 arithmetic rounded once sits inside half the bound on every case and region the GPU test
runs; (c) every mutant fails the bound on every case and region it applies to (the ones the bound cannot see are named, with the
reason, and shown to be invisible for that reason); (d) the NS column set is what the sparse cases claim.  No GPU.

(b) is a statement about draws: the corner region of a case holds 4 N cout elements (768 .. 2304), and ONE element whose float64 value lies
within fp32 precision of a 16-bit rounding boundary costs such a region up to 0.6 floor when it is a 2-sigma SiLU output.  The first
draw of the epilogue parameters had one such element (2.02343720 against the tie 2.0234375, bf16, 1 region of 1212 over floor / 2);
the generator key of upconv_refs.Built was changed once for it, before any kernel ran."""
import pytest
import torch

from tests import sample_op_refs as S
from tests import upconv_refs as R
from tests.test_gpu_conv_forms import epilogue_f64

# one case per distinct operand set (n, plane, channels, needed set) and feature kind: the matrix repeats operands across its form rows
def _distinct(cases):
    seen, out = set(), []
    for c in cases:
        k = (c["n"], c["h"], c["w"], c["c0"], c["c1"], c["cout"], c["feature"], c["needed"])
        if k not in seen:
            seen.add(k)
            out.append(c)
    return out


DISTINCT = _distinct(R.CASES)


def test_phase_factors_come_out_of_the_resample_matrix():
    E = R.phase_factors()
    # every upsampled sample is a convex mix: per kernel tap the stencil coefficients add up to one
    assert torch.equal(E[:, :3].sum(1), torch.ones(2, 3, dtype=torch.float64))
    # the correction removes exactly the kernel tap that looks into the zero padding: k = 0 on the first output, k = 2 on the last
    assert E[0, 3].tolist() == [-1.0, 0.0, 0.0] and E[1, 3].tolist() == [0.0, 0.0, -1.0]


def test_a_with_unrounded_taps_is_interpolate_then_conv2d():
    """(a) on every distinct operand set: rel-max 1e-12."""
    seen = set()
    for case in R.CASES:
        b = R.build(case, "bf16")
        if b.key in seen:
            continue
        seen.add(b.key)
        xs = [t.double() for t in b.xs]
        A, B = R.upconv_acc(xs, R.taps(b.wt)), R.model_b(xs, b.wt.double())
        err = float((A - B).abs().max()) / float(B.abs().max())
        assert err <= 1e-12, (case["id"], err)
    assert len(seen) >= 12


def test_the_epilogue_is_the_conv_forms_chain():
    for cid in ("rows0-8x32-64+0>128-n3-coefdiv", "mixed-32x128-64+0>64-n3-mask2", "halo0-24x48-64+0>128-n3-act3"):
        b = R.build(R.BY_ID[cid], "fp16")
        want, _, _ = epilogue_f64(b.acc(torch.float64), b.scale, b.shift, b.coef_div, b.act, b.keep, R.P_DROP if b.keep is not None else 0.0)
        assert torch.equal(b.ref(dense=True), want), cid


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_fp32_rounded_once_sits_inside_half_the_bound_on_every_case_and_region(dtname):
    dt = S.DTYPES[dtname]
    worst = 0.0
    for case in DISTINCT:
        b = R.build(case, dtname)
        got = b.ref(torch.float32).to(dt)  # (fp32 -> 16 bit: one rounding)
        for name, (excess, floor) in b.excess(got).items():
            worst = max(worst, excess / floor)
            assert excess <= floor / 2, (case["id"], name, excess, floor)
    print(f"[upconv refs] {dtname}: worst fp32 excess / floor over {len(DISTINCT)} cases and their regions = {worst:.3f}")


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_every_mutant_fails_the_bound_on_every_case_and_region_it_applies_to(dtname):
    dt = S.DTYPES[dtname]
    hit = {m: 0 for m in R.MUTANTS}
    seen = set()
    for case in DISTINCT:
        b = R.build(case, dtname)
        have = set(R.regions(2 * case["h"], 2 * case["w"], b.cols))
        for mutant in R.MUTANTS:
            where = [r for r in R.applies(mutant, case) if r in have]
            # a mutant of the accumulator does not depend on the epilogue: once per operand set and column set
            once = (mutant, b.key, case["needed"])
            if not where or (mutant in R.ACC_MUTANTS and once in seen):
                continue
            seen.add(once)
            res = b.excess(b.ref(mutant=mutant).float().to(dt), where)  # (a mutant is far off: how it is rounded does not matter)
            for r in where:
                excess, floor = res[r]
                if mutant in R.INVISIBLE:  # named, with the reason: the mutant is the reference there
                    assert excess <= floor / 2, (mutant, case["id"], r, excess, floor)
                    continue
                assert not excess <= floor, (mutant, case["id"], r, excess, floor)
                hit[mutant] += 1
    print(f"[upconv refs] {dtname}: (case, region) pairs that see each mutant: {hit}")
    assert all(hit[m] > 0 for m in R.MUTANTS if m not in R.INVISIBLE), hit


def test_the_mutants_reach_every_kind_of_case():
    """Every mutant applies somewhere; the sparse-only and the dropout-only ones have a case of each sparse plan / dropout mode."""
    for m in R.MUTANTS:
        ids = [c["id"] for c in R.CASES if R.applies(m, c)]
        assert ids, m
    for form in ("mixed", "uniform32", "halo1", "ragged", "edges", "edges-halo1"):
        assert any(c["form"] == form and R.applies("slot_shifted", c) for c in R.CASES), form
    for form in ("mixed", "mixed-2grids", "uniform32", "halo1"):
        for ft in ("mask2", "rng1"):
            assert any(c["form"] == form and c["feature"] == ft and R.applies("drop_compact_pos", c) for c in R.CASES), (form, ft)
    # a 32-column seam needs more than 32 low-res columns; the 8 x 32 and 16 x 32 planes have a 16-column one only
    assert not R.applies("seam32", R.BY_ID["rows0-8x32-64+0>128-n3-base"]) and R.applies("seam16", R.BY_ID["rows0-8x32-64+0>128-n3-base"])
    assert R.applies("seam32", R.BY_ID["rows0-32x64-64+0>64-n3-base"])


def test_the_ns_column_set_is_what_the_sparse_cases_claim():
    """(d) 104 of dec5's 256 output columns, 52 per horizontal phase; neither the first nor the last column: the `edges` set adds them."""
    m = R.ns_needed()
    assert int(m.sum()) == 104 and int(m[0::2].sum()) == 52 and int(m[1::2].sum()) == 52
    assert not bool(m[0]) and not bool(m[-1])
    used, cmap = S.readout_columns(R.NS_IW, R.NS_OW, False)
    assert m.nonzero().flatten().tolist() == used and cmap[m].tolist() == list(range(104))
    rag = R.needed_of("ragged", 256)
    assert int(rag[0::2].sum()) == 52 and int(rag[1::2].sum()) == 49 and bool((m | ~rag).all())
    edg = R.needed_of("edges", 256)
    assert int(edg[0::2].sum()) == 54 and int(edg[1::2].sum()) == 54 and bool(edg[0]) and bool(edg[-1])
    e16 = R.needed_of("edges16", 256)
    assert int(e16[0::2].sum()) == 52 and int(e16[1::2].sum()) == 52 and bool(e16[0]) and bool(e16[-1])
    dec = R.needed_of("declined", 256)
    assert int(dec[0::2].sum()) == 128  # every even column: as many list entries as the dense form has columns
    for form, plan in R.PLANS.items():
        if "wo_store" in plan:
            assert plan["wo_store"] == int(R.needed_of(R.FORMS[form][2], 256).sum()) == plan["nvalid0"] + plan["nvalid1"], form
    # 52 entries = 3 x 16 + 4 (mixed), two tiles of 32 or four of 16 (uniform)
    assert R.PLANS["mixed"]["npad"] == 3 * 16 + 4 and R.PLANS["uniform32"]["npad"] == 2 * 32 and R.PLANS["halo1"]["npad"] == 4 * 16


def test_the_cases_cover_the_form_rows_and_feature_columns():
    assert {c["form"] for c in R.CASES} == set(R.FORMS)
    for form in R.ROWS:
        assert {c["feature"] for c in R.MATRIX if c["form"] == form} == set(R.FEATURES), form
    # the coefdiv column leaves a short last coefficient row; the ring's 8 + 1 grouping needs nine samples
    assert all(c["n"] % 2 == 1 for c in R.CASES if c["feature"] == "coefdiv")
    assert all(c["n"] == 9 for c in R.CASES if c["form"] in ("border8", "border8-nsel80", "ring4"))
