"""The reference, the cases and the mutants of tests/conv_gn_refs.py, on the CPU: the reference is the composition of PyTorch's own
conv2d and group_norm; fp32 arithmetic rounded once sits inside half the bound on every case the GPU test runs; every mutant fails
the bound on a named case of every kernel form it applies to.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

from tests import conv_gn_refs as R
from tests import sample_op_refs as S


def test_the_reference_is_conv2d_then_group_norm_in_float64():
    for cid in ("gn16-20x36-128+64>64-g8", "bm128-15x15-128+0>128-g2", "halo5-30x30-64+0>64-g1"):
        b = R.build(R.BY_ID[cid], "bf16")
        x = torch.cat([t.double() for t in b.xs], 3).permute(0, 3, 1, 2)
        y = F.conv2d(x, b.wt.to(torch.bfloat16).double(), b.bias.double(), 1, 1)
        want = F.silu(F.group_norm(y, b.case["groups"], b.gamma.double(), b.beta.double(), 1e-5)).permute(0, 2, 3, 1)
        got = b.ref()
        assert float((got - want).abs().max()) <= 1e-11 * float(want.abs().max()), cid
        # the statistics taken from per-slot partials of the form's slot geometry are the same statement
        assert float((b.ref(mutant="partials") - got).abs().max()) <= 1e-9 * float(want.abs().max()), cid


def test_the_cases_name_every_form_and_the_slot_counts_are_the_ladders():
    assert len(R.BY_ID) == len(R.CASES)
    assert {c["form"] for c in R.CASES} == set(R.FORMS)
    slots = {c["id"]: R.slots_of(c["form"], c["h"], c["w"]) for c in R.CASES}
    assert slots["gn16-20x36-64+0>64-g8"] == 6 and slots["gn16-16x16-64+0>64-g8"] == 1 and slots["halo5-16x32-64+0>64-g8"] == 4
    assert slots["halo5-30x30-64+0>64-g8"] == 8 and slots["bm256-15x15-128+0>128-g8"] == 3 and slots["bm128-15x15-128+0>128-g8"] == 5
    assert slots["bm256-16x32-128+0>128-g8"] == 4 and slots["bm128-16x32-128+0>128-g8"] == 8 and slots["prod>bm128-40x40-256+0>256-g8"] == 26
    assert all(0 < s <= 64 for s in slots.values())  # far below the sweep's 64 slots
    assert all(R.slots_of(c["form"], c["h"], c["w"]) == 0 for c in R.UNSERVED)
    # 15 x 15 with N = 3: samples start at rows 0 / 225 / 450 of the flattened axis, so slabs of 128 and of 64 rows straddle samples
    for rows in (128, 64):
        owner, _, _ = R._slot_owner(("slab", rows), 3, 15, 15, straddle_first=True)
        assert not torch.equal(owner, torch.arange(3)[:, None].expand(3, 225))


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_fp32_rounded_once_sits_inside_half_the_bound_on_every_case(dtname):
    dt = S.DTYPES[dtname]
    worst = 0.0
    for case in R.CASES:
        b = R.build(case, dtname)
        ref = b.ref()
        excess, floor = S.excess_floor(S.round16(b.ref(torch.float32), dt), ref, dt)
        worst = max(worst, excess / floor)
        assert excess <= floor / 2, (case["id"], excess, floor)
    print(f"[conv_gn refs] {dtname}: worst fp32 excess / floor over {len(R.CASES)} cases = {worst:.3f}")


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_every_mutant_fails_the_bound_on_every_form_it_applies_to(dtname):
    dt = S.DTYPES[dtname]
    assert set(R.VISIBLE) == set(R.MUTANTS)
    for mutant, ids in R.VISIBLE.items():
        forms = {R.kernel_of(R.BY_ID[i]["form"]) for i in ids}
        applies = {"gn16", "halo5", "bm128", "bm256"} if mutant != "straddle_first" else {"bm128", "bm256"}  # (only flattened slabs straddle)
        assert forms == applies, (mutant, forms)
        for cid in ids:
            b = R.build(R.BY_ID[cid], dtname)
            ref = b.ref()
            excess, floor = S.excess_floor(S.round16(b.ref(mutant=mutant), dt), ref, dt)
            print(f"[conv_gn refs] {dtname} {mutant} on {cid}: excess / floor = {excess / floor:.1f}")
            if dtname == "bf16" and cid in R.INVISIBLE_BF16.get(mutant, ()):
                assert excess <= floor, (mutant, cid, excess, floor)  # listed as invisible in this build: say so if that changes
                continue
            assert not excess <= floor, (mutant, cid, excess, floor)  # (a NaN -- a negative variance -- does not pass either)


def test_the_invisible_pairs_are_invisible_for_the_reason_given():
    for mutant, ids in R.INVISIBLE.items():
        for cid in ids:
            b = R.build(R.BY_ID[cid], "fp16")
            ref = b.ref()
            excess, floor = S.excess_floor(S.round16(b.ref(mutant=mutant), torch.float16), ref, torch.float16)
            assert excess <= floor / 2, (mutant, cid, excess, floor)  # the mutant is the reference there (up to float64 rounding)


def test_the_statistics_bound_holds_for_fp32_sums_of_the_reference():
    """The partials of the statistics entry, formed by plain fp32 arithmetic on the CPU, fit stats_bound."""
    for case in R.STATS_CASES:
        b = R.build(case, "bf16")
        wq = b.wt.to(torch.bfloat16)
        z64 = b.acc(torch.float64) + b.bias.double()
        absc = R.conv3x3([t.double().abs() for t in b.xs], wq.double().abs())
        n, h, w, C = z64.shape
        z32 = (b.acc(torch.float32) + b.bias).reshape(n, h * w, C // 8, 8)
        got = torch.stack([z32.sum((1, 3)), z32.pow(2).sum((1, 3))], -1).double()
        z8 = z64.reshape(n, h * w, C // 8, 8)
        want = torch.stack([z8.sum((1, 3)), z8.pow(2).sum((1, 3))], -1)
        bound = R.stats_bound(absc, b.bias, 9 * (case["c0"] + case["c1"]))
        assert bool(((got - want).abs() <= bound).all()), case["id"]


@pytest.mark.parametrize("dtname", ["bf16", "fp16"])
def test_the_two_step_chain_pays_for_its_intermediate_rounding(dtname):
    """GN_ACT behind the statistics entry reads y = conv + bias AFTER its rounding to 16 bit: even with float64 arithmetic and exact
    statistics that chain misses excess <= floor against the fused reference -- the GPU test therefore holds it to the float64 chain of
    the same two steps, and to the fused reference at floor + this figure."""
    for case in R.STATS_CASES:
        b = R.build(case, dtname)
        twice, floor = R.two_step_excess(b), S.excess_floor(b.ref(), b.ref(), S.DTYPES[dtname])[1]
        print(f"[conv_gn refs] {dtname} {case['id']}: two-step chain in float64: excess / floor = {twice / floor:.2f}")
        assert twice > floor, (case["id"], twice, floor)
