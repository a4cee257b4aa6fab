"""-m gpu: every kernel FORM of the fused Upsample(x2, bilinear) + Conv2d(3x3, pad 1) family -- conv_igemm_kernel<.., UP>,
conv_up_halo_kernel<0> (also one column block per XCD), conv_halo_rows_kernel<0> (+tr2 / +tr1 / +splitk 2 and 4), the three border-ring
kernels, and the sparse-column forms conv_halo_rows_kernel<1> (mixed plan in one grid and in two, uniform 32-slot tiles) and
conv_up_halo_kernel<1> -- as ONE op through HipEngine.op_upconv2d_ex (dyf_op_upconv2d_ex: the ConvArgs of a decoder block, launch_conv:
the form is the ladder's), against the float64 operand model of tests/upconv_refs.py, in both builds (bf16, fp16), with the form of
every case pinned by the form log (conv_* and up_border* notes) and the sparse plan the seam reports asserted.

Every case is checked four ways: excess <= floor against the reference PER REGION (interior, first / last row, first / last column, the
four corner pixels together: tests/sample_op_refs.py's bound -- what the kernel adds to rounding once must not exceed what rounding once
costs; no number comes from the kernels); the output buffer holds a sentinel before the launch that must be gone (and the seam fills the
border scratch with NaN: a ring pixel the border kernel leaves out is a NaN here); the same call twice is bit-equal; the batch rolled
by one sample gives the rolled output bit for bit (halo rows leaking across samples, the border ring's groups of eight / four).  The
roll is left out where the operation itself is not roll-invariant: coef_div = 2 with an odd batch (the rows pair other samples) and the
generator's masks (they follow the GLOBAL row).  tests/test_upconv_refs.py shows on the CPU that fp32 arithmetic sits inside floor / 2 on
every case and region and that each mutant of the reference fails the bound where it applies.

Sparse against dense, bit for bit on the stored columns: no kernel header promises one K order for the sparse and the dense forms.
tests/test_gpu_nets.py (test_sparse_last_decoder_block_...) relies on conv_halo_rows_kernel<1> against <0> at full size, so the rows
plans (mixed, two grids, uniform 32, ragged, edges) are ASSERTED equal to conv_halo_rows_kernel<0> here; conv_up_halo_kernel<1> against
<0> is compared and the outcome printed, the float64 bound alone holds for it (on an MI355X it came out equal on every case, both builds).

Measured on an MI355X, worst excess / floor over the cases of a kernel, interior | ring regions: bf16 at most 0.04 | 0.18 (the one-row
tiles' first column), fp16 at most 0.13 | 0.35 (a corner region of the two-row tiles); fp32 torch on the CPU: 0.16 / 0.25.
"""
import pytest
import torch

from dyffusion_amd import _lib
from tests import sample_op_refs as S
from tests import upconv_refs as R
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
        print(f"[upconv] worst excess / floor on {k[0]} ({k[1]}): {_worst[k][0]:.3f} at {_worst[k][1]}")


def launch(eng, b, roll=0, **over):
    """One launch of case `b` (roll: its samples rotated) -> y, or (y, plan) for a sparse case."""
    pick = lambda t: None if t is None else t.roll(roll, 0).contiguous().cuda()
    kw = dict(x1=pick(b.xs[1]) if len(b.xs) > 1 else None, coef_div=b.coef_div, n_sel=b.case["n_sel"], fill=SENTINEL)
    if b.mask is not None:
        kw.update(mask=pick(b.mask), p=R.P_DROP)
    if b.gen:
        eng.seed(S.SEED)
        kw.update(p=R.P_DROP, rng_site=S.SITE, rng_row_offset=S.ROW_OFFSET, rng_forward=S.FORWARD)
    if b.needed is not None:
        kw.update(needed=b.needed)
    kw.update(over)
    return eng.op_upconv2d_ex(pick(b.xs[0]), b.wt, pick(b.scale), pick(b.shift), b.act, **kw)


def pinned(eng, form, fn):
    """Run fn() with the form log on: the launch noted exactly the conv_* / up_border* notes of `form`."""
    eng.form_log(True)
    try:
        out = fn()
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    noted = {k for k in forms if k.startswith("conv_") or k.startswith("up_border")}
    assert noted == R.FORMS[form][0], (form, sorted(noted))
    return out


def switches(form_switch, form):
    for k, v in R.FORMS[form][1].items():
        form_switch.setenv(k, v)


def bound(b, y, tag, dtype):
    form = b.case["form"]
    for name, (excess, floor) in b.excess(y.cpu()).items():
        print(f"[upconv] {tag} {dtype} {name}: excess {excess:.3e} floor {floor:.3e} ratio {excess / floor:.3f}")
        key = (R.KERNEL_OF.get(form, form) + (" ring" if name != "interior" else ""), dtype)
        if key not in _worst or excess / floor > _worst[key][0]:
            _worst[key] = (excess / floor, f"{tag} {name}")
        assert excess <= floor, (tag, name, excess, floor)


def check_plan(b, plan):
    """The plan the seam reports is the one the case is there for; col_map is the increasing enumeration of `needed`."""
    form = b.case["form"]
    want = R.PLANS[form]
    assert {k: plan[k] for k in want} == want, (form, plan, want)
    if plan["planned"]:
        cm = torch.full((b.needed.numel(),), -1, dtype=torch.int16)
        cm[b.needed] = torch.arange(int(b.needed.sum()), dtype=torch.int16)
        assert torch.equal(plan["col_map"], cm), form


def roll_invariant(b):
    return not b.gen and not b.coef_div


def four_ways(eng, b, dtype):
    case = b.case
    out = pinned(eng, case["form"], lambda: launch(eng, b))
    y, plan = out if b.needed is not None else (out, None)
    if plan is not None:
        check_plan(b, plan)
    assert tuple(y.shape) == tuple(b.ref().shape), (case["id"], tuple(y.shape))
    assert not bool((y == SENTINEL).any()) and bool(torch.isfinite(y.float()).all()), case["id"]  # every element written, no ring pixel left NaN
    bound(b, y, case["id"], dtype)
    again = launch(eng, b)
    assert torch.equal(y, again[0] if plan is not None else again), case["id"]
    if roll_invariant(b):
        rolled = launch(eng, b, roll=1)
        assert torch.equal(rolled[0] if plan is not None else rolled, y.roll(1, 0)), case["id"]
    if b.keep is not None:  # the zeros are exactly the dropped elements, at the DENSE position also in a compact tensor
        exact_mask(y, b.gather(b.keep), b.ref(keep=None), case["id"])
    return y


# ------------------------------------------------------------------------------------------------ form rows x feature columns
@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.MATRIX + R.EXTRA, ids=lambda c: c["id"])
def test_form_meets_float64_per_region(engines, form_switch, case, dtype):
    eng, b = engines(dtype), R.build(case, dtype)
    switches(form_switch, case["form"])
    y = four_ways(eng, b, dtype)
    dense_form = R.DENSE_OF.get(case["form"])
    if dense_form is None:
        return
    # the dense launch of the same kernel family, same operands and epilogue (the dense mask / generator stream): the stored columns
    _lib.set_form(None)
    for k, v in R.FORMS[dense_form][1].items():
        form_switch.setenv(k, v)
    dense = pinned(eng, dense_form, lambda: launch(eng, b, needed=None))
    same = torch.equal(b.gather(dense), y)
    print(f"[upconv] {case['id']} {dtype}: stored columns of {case['form']} bit-equal to {dense_form}: {same}")
    if dense_form == "rows0":
        assert same, case["id"]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("case", R.FALLS, ids=lambda c: c["id"])
def test_unequal_sources_fall_to_the_implicit_gemm_form(engines, form_switch, case, dtype):
    """128 + 64 channels: the halo forms take c1 == c0 or 0; without any switch the ladder falls to conv_igemm_kernel<.., UP> (no ring)."""
    eng, b = engines(dtype), R.build(case, dtype)
    four_ways(eng, b, dtype)


# ------------------------------------------------------------------------------------------------ the seam refuses, never truncates
def test_the_seam_refuses_what_the_arguments_cannot_express(engines):
    eng = engines("bf16")
    x = torch.zeros(2, 8, 32, 64, dtype=torch.bfloat16).cuda()
    wt = torch.zeros(64, 64, 3, 3)
    ones = torch.ones(2, 64).cuda()
    with pytest.raises(ValueError):
        eng.op_upconv2d_ex(x, wt, act=5)
    with pytest.raises(ValueError):
        eng.op_upconv2d_ex(x, wt, coef_div=2)  # coefficient rows per pair of samples, but no coefficients
    with pytest.raises(ValueError):
        eng.op_upconv2d_ex(x, wt, ones, ones, p=1.0, mask=torch.ones(2, 16, 64, 64, dtype=torch.uint8).cuda())
    with pytest.raises(ValueError):  # mode 1 draws from the engine's row-key table: 2 max_batch = 32 rows
        eng.op_upconv2d_ex(torch.zeros(33, 8, 16, 64, dtype=torch.bfloat16).cuda(), torch.zeros(128, 64, 3, 3), rng_site=0, p=0.1)
    with pytest.raises(ValueError):  # a sparse launch writes the compact 16-bit tensor alone
        eng.op_upconv2d_ex(x, wt, needed=torch.ones(64, dtype=torch.uint8), out_f32=True)
    with pytest.raises(NotImplementedError):  # cout 64 tiles the low-res plane by 16 x 16
        eng.op_upconv2d_ex(x, wt)
    with pytest.raises(NotImplementedError):  # GELU has no MFMA epilogue
        eng.op_upconv2d_ex(x, torch.zeros(128, 64, 3, 3), act=4)
    with pytest.raises(NotImplementedError):
        eng.op_upconv2d_ex(x[..., :32].contiguous(), torch.zeros(128, 32, 3, 3))  # 64-channel chunks
