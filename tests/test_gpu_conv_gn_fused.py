"""-m gpu: every kernel FORM of the fused-GroupNorm ladder (csrc/conv_dispatch.hip choose_gn_fused: conv_gn16_kernel, conv_up_halo_kernel<5, 2>,
conv_igemm2_kernel<2, true> on 256- and on 128-pixel tiles) and the statistics epilogue of launch_conv_stats, as ONE op through
HipEngine.op_conv_gn (dyf_op_conv_gn: the entry points themselves, so form choice, slots and tile height are the ladder's), against the
float64 reference of tests/conv_gn_refs.py, in both builds (bf16, fp16), with the form of every case pinned by the form log.

The bound is tests/sample_op_refs.py's: excess <= floor against the float64 reference (what the kernel adds to rounding ONCE must not
exceed what rounding once costs); no number comes from the kernels.  tests/test_conv_gn_refs.py shows on the CPU that fp32 arithmetic
sits inside floor / 2 on every case and that each mutant of the reference -- a wrong pixel count on a ragged tile, a dropped slot, a
slab credited to the neighbouring sample, 64 channels per group assumed, the FiLM row per sample, ... -- fails it on every form.
Every case runs twice on one granule buffer (the second forward must not read the first one's granules) and must repeat bit for bit.

One known limit of a check, not of a kernel: GN_ACT fed the statistics entry's partials normalises the conv output AFTER its rounding
to 16 bit, so against the fused reference (which never rounds in between) it carries that rounding too; the case is asserted against
the float64 chain of the same two steps at excess <= floor, and against the fused reference at floor + what that two-step chain
itself costs in float64 (conv_gn_refs.two_step_excess, shown by the host test).
"""
import pytest
import torch

from tests import conv_gn_refs as R
from tests import sample_op_refs as S
from tests.test_gpu_conv_forms import exact_mask

pytestmark = pytest.mark.gpu

SENTINEL = 123.0
_worst = {}


@pytest.fixture(scope="module")
def engines():
    import dyffusion_amd as D
    made = {}

    def get(dtype):
        if dtype not in made:
            cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
            made[dtype] = D.HipEngine(cfg, cfg, 16, 16, max_batch=16, use_graph=False, dtype=dtype)  # row-key table: 32 rows
        return made[dtype]
    yield get
    for k in sorted(_worst):
        print(f"[conv_gn] worst excess / floor on {k[0]} ({k[1]}): {_worst[k][0]:.3f} at {_worst[k][1]}")


def buffers(b, n=None, max_slots=None):
    """A granule buffer and an epoch word as a forward owns them: zeroed once."""
    words = (n or b.case["n"]) * (max_slots or b.max_slots) * (b.case["cout"] // 8) * 2
    return torch.zeros(words, dtype=torch.int64, device="cuda"), torch.zeros(1, dtype=torch.int32, device="cuda")


def launch(eng, b, buf, tag=1, new_forward=True, rows=None, roll=0, **over):
    """One fused launch of case `b` (rows: a slice of its samples; roll: its samples rotated) -> (y, info)."""
    pick = lambda t: None if t is None else t.roll(roll, 0)[rows if rows is not None else slice(None)].contiguous().cuda()
    kw = dict(groups=b.case["groups"], x1=pick(b.xs[1]) if len(b.xs) > 1 else None, residual=pick(b.residual), coef_div=b.coef_div, n_sel=b.n_sel,
              gran=buf[0], epoch=buf[1], conv_tag=tag, max_slots=b.max_slots, new_forward=new_forward)
    if b.film is not None:
        kw.update(film_a=b.film[0].cuda(), film_c=b.film[1].cuda())
    if b.gen:
        eng.seed(S.SEED)
        kw.update(p=R.P_DROP, rng_site=S.SITE, rng_row_offset=S.ROW_OFFSET, rng_forward=S.FORWARD)
    kw.update(over)
    return eng.op_conv_gn(pick(b.xs[0]), b.wt, b.bias, b.gamma, b.beta, **kw)


def logged(eng, fn):
    eng.form_log(True)
    try:
        out = fn()
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    return out, {k for k in forms if k.startswith("conv_")}


def pinned(eng, form, fn):
    """Run fn() with the form log on: the launch noted exactly the +gn_fused notes of `form` and no other conv form."""
    out, conv = logged(eng, fn)
    assert {k for k in conv if k.endswith("+gn_fused")} == R.FORMS[form][0] and conv <= R.FORMS[form][0] | {R.SH3}, (form, sorted(conv))
    return out


def switches(form_switch, form):
    for k, v in R.FORMS[form][1].items():
        form_switch.setenv(k, v)


def bound(y, ref, dtype, tag, form):
    excess, floor = S.excess_floor(y.cpu(), ref, S.DTYPES[dtype])
    print(f"[conv_gn] {tag} {dtype}: excess {excess:.3e} floor {floor:.3e} ratio {excess / floor:.3f}")
    key = (R.kernel_of(form), dtype)
    if key not in _worst or excess / floor > _worst[key][0]:
        _worst[key] = (excess / floor, tag)
    assert excess <= floor, (tag, excess, floor)


def expect_info(b):
    return dict(fused=1, slots=b.slots, bm={"bm128": 128, "bm256": 256}.get(R.kernel_of(b.case["form"]), 0))


def same_info(info, want, tag):
    if info["slow_sweep"]:  # not a failure: the sample's workgroups were not co-scheduled (a shared GPU); the result is still checked
        print(f"[conv_gn] {tag}: a sweep needed more than 1024 passes")
    assert {k: info[k] for k in want} == want, (tag, info, want)


# ------------------------------------------------------------------------------------------------ forms and features
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c["id"])
def test_fused_form_meets_float64(engines, form_switch, case, dtype):
    eng, b = engines(dtype), R.build(case, dtype)
    switches(form_switch, case["form"])
    buf = buffers(b)
    y, info = pinned(eng, case["form"], lambda: launch(eng, b, buf))
    same_info(info, expect_info(b), case["id"])
    bound(y, b.ref(), dtype, case["id"], case["form"])
    again, info2 = pinned(eng, case["form"], lambda: launch(eng, b, buf))  # the next forward on the same granules
    same_info(info2, expect_info(b), case["id"])
    assert torch.equal(y, again), case["id"]
    if b.gen and b.residual is None:  # the zeros are exactly the dropped elements
        exact_mask(y, b.keep, b.ref(keep=None), case["id"])


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.UNSERVED, ids=lambda c: c["id"])
def test_planes_no_fused_form_serves_launch_nothing(engines, form_switch, case, dtype):
    eng, b = engines(dtype), R.build(case, dtype)
    switches(form_switch, case["form"])
    y = torch.full((case["n"], case["h"], case["w"], case["cout"]), SENTINEL, dtype=S.DTYPES[dtype], device="cuda")
    (out, info), conv = logged(eng, lambda: launch(eng, b, buffers(b, max_slots=8), max_slots=8, y=y))
    same_info(info, dict(fused=0, slots=0, bm=0), case["id"])
    assert not conv and bool((out == SENTINEL).all()), (case["id"], sorted(conv))


# ------------------------------------------------------------------------------------------------ the ladder's refusals
REFUSALS = {"mask": lambda b: dict(mask=torch.ones(b.ref().shape, dtype=torch.uint8).cuda(), p=R.P_DROP), "act": lambda b: dict(act=2),
            "group-crosses-block": lambda b: dict(groups=3), "max_slots": lambda b: dict(max_slots=b.slots - 1)}


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("what", sorted(REFUSALS))
def test_the_ladder_refuses_and_leaves_the_output_alone(engines, form_switch, what, dtype):
    """An injected mask (dropout mode 2), an activation other than SiLU, a group that crosses a 64-channel block (cout 64, groups 3)
    and more slots than the granule buffer's stride: fused = 0, nothing launched, y untouched."""
    eng = engines(dtype)
    b = R.build(R.BY_ID["gn16-20x36-64+0>64-g8"], dtype)
    switches(form_switch, "gn16")
    y = torch.full(tuple(b.ref().shape), SENTINEL, dtype=S.DTYPES[dtype], device="cuda")
    (out, info), conv = logged(eng, lambda: launch(eng, b, buffers(b), y=y, **REFUSALS[what](b)))
    same_info(info, dict(fused=0, slots=0, bm=0), what)
    assert not conv and bool((out == SENTINEL).all()), (what, sorted(conv))


def test_the_seam_refuses_what_the_descriptor_cannot_express(engines):
    eng = engines("bf16")
    b = R.build(R.BY_ID["gn16-16x16-64+0>64-g8"], "bf16")
    buf = buffers(b)
    for over in (dict(conv_tag=0), dict(conv_tag=256), dict(max_slots=0), dict(groups=0), dict(act=5), dict(max_slots=b.slots + 1),  # (gran too small)
                 dict(coef_div=2), dict(film_a=torch.ones(3, 32).cuda(), film_c=torch.ones(3, 32).cuda())):
        with pytest.raises(ValueError):
            launch(eng, b, buf, **over)
    part = torch.zeros(3 * 4 * 8 * 2 - 1, device="cuda")  # one float short of 3 samples x 4 slots x 8 octets x 2
    with pytest.raises(ValueError):
        eng.op_conv_gn(b.xs[0].cuda(), b.wt, b.bias, want="stats", part=part)


# ------------------------------------------------------------------------------------------------ the tag protocol
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("form", sorted(R.FEATURE_BASE))
def test_granules_of_another_conv_or_forward_are_never_read(engines, form_switch, form, dtype):
    """On ONE granule buffer: data A as conv 1 of forward 1, data B as conv 2 of the same forward, data C as conv 1 of the next forward
    (B, C: A's samples rotated, so every slot holds a different value).  Each result is that of its own data: the float64 bound, and
    bit for bit what the same launch gives on a fresh buffer."""
    eng = engines(dtype)
    b = R.build(R.BY_ID[R._case(form, *R.FEATURE_BASE[form], 8)["id"]], dtype)
    switches(form_switch, form)
    buf, ref = buffers(b), b.ref()
    for step, (roll, tag, new) in enumerate(((0, 1, True), (1, 2, False), (2, 1, True))):
        y, _ = pinned(eng, form, lambda: launch(eng, b, buf, tag=tag, new_forward=new, roll=roll))
        bound(y, ref.roll(roll, 0), dtype, f"{form} tags step {step}", form)
        fresh, _ = launch(eng, b, buffers(b), tag=tag, roll=roll)
        assert torch.equal(y, fresh), (form, step)
    assert int(buf[1].item()) == 2  # two forwards began


# ------------------------------------------------------------------------------------------------ position in the launch
POSITION_FREE = [R._case("gn16", 20, 36, 64, 0, 64, 8), R._case("halo5", 30, 30, 64, 0, 64, 8), R._case("bm128", 16, 32, 128, 0, 128, 8),
                 R._case("bm256", 16, 32, 128, 0, 128, 8), R._case("bm128", 8, 8, 128, 0, 128, 8), R._case("bm256", 8, 16, 128, 0, 128, 8)]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", POSITION_FREE, ids=lambda c: c["id"])
def test_a_sample_does_not_depend_on_its_position(engines, form_switch, case, dtype):
    """conv_gn16, conv_up_halo<5>, the 2-D tiles and slab-aligned planes (8 x 8 = one 64-row slab, 8 x 16 = one 128-row slab of the
    flattened axis): row r launched alone, its form chosen for the same rows (n_sel), equals row r of the N-row launch bit for bit --
    what GnFuse::invariant promises a batch_invariant engine, which these forms therefore still serve (the ladder asks plane % 128 == 0 of
    every flattened form, so the 64-row slab of 8 x 8 runs without the flag)."""
    eng, b = engines(dtype), R.build(case, dtype)
    switches(form_switch, case["form"])
    n, inv = case["n"], (case["h"], case["w"]) != (8, 8)
    full, info = pinned(eng, case["form"], lambda: launch(eng, b, buffers(b), n_sel=n, invariant=inv))
    same_info(info, expect_info(b), case["id"])
    bound(full, b.ref(), dtype, case["id"] + " invariant", case["form"])
    for r in range(n):
        alone, _ = pinned(eng, case["form"], lambda: launch(eng, b, buffers(b, n=1), rows=slice(r, r + 1), n_sel=n, invariant=inv))
        assert torch.equal(alone[0], full[r]), (case["id"], r)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("form", ["bm128", "bm256"])
def test_flattened_slabs_are_refused_to_an_invariant_engine(engines, form_switch, form, dtype):
    eng = engines(dtype)
    b = R.build(R.BY_ID[R._case(form, 15, 15, 128, 0, 128, 8)["id"]], dtype)
    switches(form_switch, form)
    y = torch.full(tuple(b.ref().shape), SENTINEL, dtype=S.DTYPES[dtype], device="cuda")
    (out, info), conv = logged(eng, lambda: launch(eng, b, buffers(b), invariant=True, y=y))
    same_info(info, dict(fused=0, slots=0, bm=0), form)
    assert not conv and bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the statistics entry
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.STATS_CASES, ids=lambda c: "stats-" + c["id"])
def test_conv_statistics_partials_and_the_gn_act_behind_them(engines, form_switch, case, dtype):
    """launch_conv_stats on conv_up_halo_kernel<5>: the partials, summed over the slots, are the float64 (sum, sum of squares) of
    y = conv + bias per (sample, octet) inside the forward bound of an fp32 sum (conv_gn_refs.stats_bound); y meets the 16-bit bound;
    GN_ACT fed these partials meets the float64 chain of the same two steps, and the fused reference up to the intermediate rounding."""
    eng, b, dt = engines(dtype), R.build(case, dtype), S.DTYPES[dtype]
    for k, v in R.STATS_SWITCH.items():
        form_switch.setenv(k, v)
    n, h, w, C = case["n"], case["h"], case["w"], case["cout"]
    slots = R.slots_of("halo5", h, w)
    part = torch.full((n, slots, C // 8, 2), float("nan"), device="cuda")
    (y, info), conv = logged(eng, lambda: eng.op_conv_gn(b.xs[0].cuda(), b.wt, b.bias, want="stats", part=part))
    assert conv == {R.STATS_FORM}, sorted(conv)
    same_info(info, dict(fused=1, slots=slots, bm=0), case["id"])
    z = b.acc(torch.float64) + b.bias.double()
    z8 = z.reshape(n, h * w, C // 8, 8)
    want = torch.stack([z8.sum((1, 3)), z8.pow(2).sum((1, 3))], -1)
    absc = R.conv3x3([t.double().abs() for t in b.xs], b.wt.to(dt).double().abs())
    ratio = (part.double().sum(1).cpu() - want).abs() / R.stats_bound(absc, b.bias, 9 * case["c0"])
    print(f"[conv_gn] stats {case['id']} {dtype}: worst err / bound: sum {float(ratio[..., 0].max()):.4f}, squares {float(ratio[..., 1].max()):.4f}")
    assert bool((ratio <= 1.0).all()), (case["id"], float(ratio.max()))
    bound(y, z, dtype, "stats y " + case["id"], "stats")
    out = eng.op_sample("gn_act", [y], [b.gamma, b.beta], groups=case["groups"], act="silu", part=part)
    two_step = S.group_norm(y.cpu().double(), b.gamma.double(), b.beta.double(), case["groups"], "silu", part=part.cpu().double())
    bound(out, two_step, dtype, "stats gn_act (two-step chain) " + case["id"], "stats")
    excess, floor = S.excess_floor(out.cpu(), b.ref(), dt)
    twice = R.two_step_excess(b)
    print(f"[conv_gn] stats gn_act vs the fused reference {case['id']} {dtype}: excess {excess:.3e} floor {floor:.3e}, the float64 two-step chain itself {twice:.3e}")
    assert excess <= floor + twice, (case["id"], excess, floor, twice)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_a_form_without_statistics_reports_no_slots(engines, form_switch, dtype):
    eng, b = engines(dtype), R.build(R.STATS_CASES[0], dtype)
    form_switch.setenv("DYF_HALO5", 0)
    part = torch.zeros(3, 4, 8, 2, device="cuda")
    (y, info), conv = logged(eng, lambda: eng.op_conv_gn(b.xs[0].cuda(), b.wt, b.bias, want="stats", part=part))
    assert conv and R.STATS_FORM not in conv, sorted(conv)
    same_info(info, dict(fused=1, slots=0, bm=0), "no statistics")
    assert not bool(part.any())
    bound(y, b.acc(torch.float64) + b.bias.double(), dtype, "plain conv + bias", "stats")
