"""-m gpu: every conv kernel FORM of the plain ladder (csrc/conv_dispatch.hip choose_plain) against a float64 reference, with the
kernel form pinned by the form log, over the whole conv argument block (csrc/conv.h ConvArgs) through dyf_op_conv2d_ex.

Each form has its own operand gather and, around the epilogue step they share (csrc/conv_epilogue.h), its own output addressing, staging
and store path, so every feature of the argument block -- second source,
residual, fp32 output, coef_div, SiLU / GELU, injected and generated dropout masks, n_sel -- is driven on every form, in both builds
(bf16, fp16).  Where a form's admission rule turns a feature away, the test names the form the ladder falls to and checks that one.

Tolerances (none comes from the code under test), against the float64 reference of the 16-bit-rounded operands:
  * 16-bit output: max |err| <= 1.5 * 2^-8 * max|y| + 1e-3 (bf16: 8 significant bits; fp16, 11 bits: 1.5 * 2^-10), rel-RMS <= 4e-3,
    border rows / columns separately <= 5e-3 -- the bounds of tests/test_gpu_conv.py;
  * two forms on the same operands: rel-RMS <= 2.5e-3 (summation order only), bit equality where the code promises it;
  * fp32 output (act = 0, which is how the engine uses it: GroupNorm input): the forward bound of an fp32 sum of K exact products,
    |err| <= (K + 4) * 2^-24 * |A| * conv(|x|, |w|) + 2^-24 * |ref|, K = kh * kw * (c0 + c1); ATen's own fp32 conv2d is checked against
    the same bound on the same case first.  The worst err / bound ratio is printed per case.
"""
import zlib

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import rng_host
from tests.helpers import max_abs, rel_rms

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}
EPS16 = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -10}   # first term of the 16-bit bound: 1.5 * EPS16 * max|y| + 1e-3
U32 = 2.0 ** -24
SEED, FWD, SITE, ROW0, P_DROP = 0x5EED1234ABCD, 3, 5, 37, 0.25

DIRECT = "conv_direct_kernel"
IGEMM128 = "conv_igemm_kernel<128,128>"
IGEMM128_SK = "conv_igemm_kernel<128,128>+splitk"
IGEMM256 = "conv_igemm_kernel<256,64>"
IGEMM2_1 = "conv_igemm2_kernel<1>"
IGEMM2_2 = "conv_igemm2_kernel<2>"
HALO2 = "conv_up_halo_kernel<2>"
ROWS2 = "conv_halo_rows_kernel<2>"
HALO5 = "conv_up_halo_kernel<5>"
HALO3 = "conv_up_halo_kernel<3>"
HALO4 = "conv_up_halo_kernel<4>"
SKINNY = "conv_skinny_kernel"
SKINNY8 = "conv_skinny_kernel<8>"
# notes a launcher adds NEXT TO its form's name: the SH3 gather of igemm2 on raster tiles; launch_conv_skinny notes the kernel, then <8>
ALSO = {IGEMM2_1: {"conv_igemm2_kernel+sh3"}, IGEMM2_2: {"conv_igemm2_kernel+sh3"}, SKINNY8: {SKINNY}}


@pytest.fixture(scope="module")
def engines():
    import dyffusion_amd as D
    made = {}

    def get(dtype):
        if dtype not in made:
            cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
            made[dtype] = D.HipEngine(cfg, cfg, 16, 16, max_batch=16, use_graph=False, dtype=dtype)  # row-key table: 32 rows
        return made[dtype]
    return get


def pinned(eng, expect, fn):
    """Run fn() with the form log on; the launch must have noted `expect` and no other conv form."""
    eng.form_log(True)
    try:
        out = fn()
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    conv = {k for k in forms if k.startswith("conv_")}
    assert expect in conv and conv <= {expect} | ALSO.get(expect, set()), (expect, sorted(forms))
    return out


# ------------------------------------------------------------------------------------------------ the reference
def conv_f64(xs, wt, stride, pad, dt):
    """float64 conv2d of the 16-bit-rounded operands, sources concatenated on channels -> (conv, conv(|x|, |w|)), NHWC."""
    x = torch.cat([t.double() for t in xs], 3).permute(0, 3, 1, 2)
    wq = wt.to(dt).double()
    raw = F.conv2d(x, wq, None, stride, pad).permute(0, 2, 3, 1).contiguous()
    absc = F.conv2d(x.abs(), wq.abs(), None, stride, pad).permute(0, 2, 3, 1).contiguous()
    return raw, absc


def act_f64(v, act):
    if act == 1:
        return v.clamp_min(0.0)
    if act == 2:
        return torch.where(v > 0, v, 0.2 * v)
    if act == 3:
        return v * torch.sigmoid(v)
    if act == 4:
        return 0.5 * v * (1.0 + torch.erf(v * 0.5 ** 0.5))  # csrc/common.h apply_act: the exact (erf) GELU
    assert act == 0
    return v


def epilogue_f64(raw, scale=None, shift=None, coef_div=0, act=0, keep=None, p=0.0, residual=None):
    """affine with row n // coef_div -> activation -> keep mask * 1/(1-p) -> + residual, all in float64.  Returns (result, the value
    in front of the mask, |A| broadcast to the output)."""
    n = raw.shape[0]
    rows = torch.arange(n) // coef_div if coef_div > 1 else torch.arange(n)
    A = scale.double()[rows][:, None, None, :] if scale is not None else torch.ones(1, 1, 1, 1, dtype=torch.float64)
    C = shift.double()[rows][:, None, None, :] if shift is not None else torch.zeros(1, 1, 1, 1, dtype=torch.float64)
    pre = act_f64(raw * A + C, act)
    y = pre
    if keep is not None:
        y = y * keep.double() * (1.0 / (1.0 - p))
    if residual is not None:
        y = y + residual.double()
    return y, pre, A.abs().expand_as(raw)


def check16(got, want, dtype, tag, borders=True):
    got, want = got.double().cpu(), want.double()
    tol = 1.5 * EPS16[dtype] * float(want.abs().max()) + 1e-3
    err, rr = max_abs(got, want), rel_rms(got, want)
    print(f"[16] {tag} {dtype}: max|err| {err:.3e} (tol {tol:.3e}) rel-RMS {rr:.3e}")
    assert err <= tol, (tag, err, tol)
    assert rr <= 4e-3, (tag, rr)
    if borders and got.shape[1] >= 2 and got.shape[2] >= 2:
        for sl in [(slice(None), 0), (slice(None), -1), (slice(None), slice(None), 0), (slice(None), slice(None), -1)]:
            assert rel_rms(got[sl], want[sl]) <= 5e-3, (tag, sl, rel_rms(got[sl], want[sl]))


def f32_bound(want, absc, absA, K):
    return (K + 4) * U32 * absA * absc + U32 * want.abs()


def check_f32(got, want, bound, tag, who):
    ratio = float(((got.double().cpu() - want).abs() / bound.clamp_min(1e-300)).max())
    print(f"[f32] {tag}: worst err/bound of {who} = {ratio:.4f}")
    assert ratio <= 1.0, (tag, who, ratio)
    return ratio


def rng_keep(n, ho, wo, cout, row0=ROW0):
    rows = [rng_host.row_mask_nhwc((ho, wo, cout), P_DROP, SEED, FWD, SITE, row0 + r) for r in range(n)]
    return torch.from_numpy(np.stack(rows, 0).astype(np.uint8))


def exact_mask(got, keep, pre, tag):
    """Dropout is exact: with no reference element zero in front of the mask, the zeros of the output ARE the dropped elements."""
    assert bool((pre != 0).all()), tag   # the precondition that makes the next line meaningful
    got = got.cpu()
    wrong = int(((got == 0) != (keep == 0)).sum())
    assert wrong == 0, (tag, wrong, got.numel())


# ------------------------------------------------------------------------------------------------ (i) form x feature matrix
def _case(name, expect, h, w, cout, k, s, p, switches=None, falls=None, path=1, chans=None):
    return dict(name=name, expect=expect, h=h, w=w, cout=cout, k=k, s=s, p=p, switches=switches or {}, falls=falls or {}, path=path,
                chans=chans or {"base": (192, 0), "src2a": (64, 128), "src2b": (192, 64), "srceq": (128, 128)})


def _falls(src2a, src2b, other, srceq=None):
    """Features a form's admission rule turns away -> the form the ladder falls to: unequal sources (the halo forms take c1 == c0 or
    0, halo-s2 takes c1 == 0), residual / fp32 output (halo3, halo-s2: admission rule; halo5: residual in choose_plain)."""
    d = {"src2a": src2a, "src2b": src2b, "residual": other, "f32": other, "all": src2a}
    if srceq:
        d["srceq"] = srceq
    return d


# Every case runs N = 4 (coefshort: its first 3 samples).  The switches are the ones tests/test_gpu_conv.py uses to force a form on a
# small problem; cases without switches pin the production thresholds.  Where the ladder falls (traced through choose_plain with the
# case's switches): 3x3 with 192 channels is 27 K steps (<= 32: skinny takes it below 65 tiles of 128 x 128), 256 channels are 36
# (implicit GEMM, split-K from 16 steps on); 4x4 is 48 / 64 steps (split-K); cout = 64 has neither skinny nor <128,128>.
FORM_CASES = [
    _case("direct", DIRECT, 9, 7, 48, 3, 1, 1, path=0, chans={"base": (40, 0), "src2a": (24, 40), "src2b": (40, 24), "srceq": (32, 32)}),
    _case("igemm128", IGEMM128, 10, 12, 128, 3, 1, 1, {"DYF_SKINNY": 0, "DYF_SPLITK": 0}),     # M = 480: ragged last tile
    _case("igemm128+splitk", IGEMM128_SK, 10, 12, 128, 3, 1, 1, {"DYF_SKINNY": 0}),
    _case("igemm256x64", IGEMM256, 10, 12, 64, 3, 1, 1),
    _case("igemm2<1>", IGEMM2_1, 16, 16, 64, 3, 1, 1, {"DYF_IGEMM2_MIN_TILES": 1}),              # 2-D tiles
    _case("igemm2<1>-ragged", IGEMM2_1, 15, 9, 64, 3, 1, 1, {"DYF_IGEMM2_MIN_TILES": 1}),       # raster tiles (SH3), M = 540
    _case("igemm2<2>", IGEMM2_2, 16, 16, 128, 3, 1, 1, {"DYF_IGEMM2_MIN_TILES": 1}),
    _case("igemm2<2>-ragged", IGEMM2_2, 15, 9, 128, 3, 1, 1, {"DYF_IGEMM2_MIN_TILES": 1}),
    _case("halo<2>", HALO2, 16, 16, 256, 3, 1, 1, {"DYF_HALO3_MIN_TILES": 1}, _falls(SKINNY, IGEMM128_SK, SKINNY)),
    _case("rows<2>", ROWS2, 8, 32, 256, 3, 1, 1, {"DYF_HALO3_MIN_TILES": 1, "DYF_HALO_SPLITK": 0}, _falls(SKINNY, IGEMM128_SK, SKINNY)),
    _case("halo<5>", HALO5, 16, 32, 64, 3, 1, 1, {"DYF_HALO5_MIN_TILES": 1}, _falls(IGEMM256, IGEMM256, IGEMM256)),
    _case("halo<5>-ragged", HALO5, 30, 30, 128, 3, 1, 1, {"DYF_HALO5_MIN_TILES": 1}, _falls(SKINNY, IGEMM128_SK, SKINNY)),
    _case("halo<3>", HALO3, 16, 32, 256, 4, 2, 1, {"DYF_HALO3_MIN_TILES": 1}, _falls(IGEMM128_SK, IGEMM128_SK, IGEMM128_SK, IGEMM128_SK)),
    _case("halo<4>", HALO4, 32, 32, 128, 4, 2, 1, {"DYF_HALO3_MIN_TILES": 1}, _falls(IGEMM128_SK, IGEMM128_SK, IGEMM128_SK, IGEMM128_SK)),
    _case("skinny", SKINNY, 6, 8, 128, 2, 2, 0),                                                # M = 48: ragged last tile
    _case("skinny<8>", SKINNY8, 6, 8, 128, 2, 2, 0, {"DYF_SKINNY_W8_FROM": 1}),
]
FEATURES = ["base", "src2a", "src2b", "srceq", "residual", "coefdiv", "coefshort", "silu", "gelu", "mask2", "rng1", "f32", "all"]
N_MATRIX = 4

_operands = {}


def operands(case, variant, dtype):
    """16-bit sources, fp32 weights and their float64 conv, per (case, channel variant, dtype): the features share them."""
    key = (case["name"], variant, dtype)
    if key not in _operands:
        dt = DTYPES[dtype]
        c0, c1 = case["chans"][variant]
        g = torch.Generator().manual_seed(zlib.crc32(repr(key).encode()))
        xs = [torch.randn(N_MATRIX, case["h"], case["w"], c, generator=g).to(dt) for c in (c0, c1) if c]
        wt = torch.randn(case["cout"], c0 + c1, case["k"], case["k"], generator=g) / ((c0 + c1) * case["k"] ** 2) ** 0.5
        _operands[key] = (xs, wt) + conv_f64(xs, wt, case["s"], case["p"], dt)
    return _operands[key]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("feature", FEATURES)
@pytest.mark.parametrize("case", FORM_CASES, ids=lambda c: c["name"])
def test_form_feature_matrix(engines, form_switch, case, feature, dtype):
    """One feature of the conv argument block at a time, then all together, on every form of the plain ladder.  GELU has no MFMA
    epilogue (conv_mfma_supported): every path-1 case falls to the direct kernel, as the engine's own GELU convs do."""
    eng, dt = engines(dtype), DTYPES[dtype]
    variant = feature if feature in ("src2a", "src2b", "srceq") else "src2a" if feature == "all" else "base"
    n = 3 if feature == "coefshort" else N_MATRIX
    xs, wt, raw, absc = operands(case, variant, dtype)
    xs, raw, absc = [t[:n].contiguous() for t in xs], raw[:n], absc[:n]
    _, ho, wo, cout = raw.shape
    K = wt.shape[1] * case["k"] ** 2
    expect = DIRECT if feature == "gelu" else case["falls"].get(feature, case["expect"])
    tag = f"{case['name']}/{feature}->{expect}"

    g = torch.Generator().manual_seed(zlib.crc32(tag.encode()))
    coef_div = 2 if feature in ("coefdiv", "coefshort", "all") else 0
    rows = -(-n // coef_div) if coef_div else n
    scale, shift = 1.0 + 0.3 * torch.randn(rows, cout, generator=g), 0.2 * torch.randn(rows, cout, generator=g)
    act = {"base": 1, "silu": 3, "gelu": 4, "f32": 0, "all": 3}.get(feature, 2)
    residual = torch.randn(n, ho, wo, cout, generator=g).to(dt) if feature in ("residual", "all") else None
    keep = None
    if feature == "mask2":
        keep = (torch.rand(n, ho, wo, cout, generator=g) >= P_DROP).to(torch.uint8)
    elif feature in ("rng1", "all"):
        keep = rng_keep(n, ho, wo, cout)
        eng.seed(SEED)
    want, pre, absA = epilogue_f64(raw, scale, shift, coef_div, act, keep, P_DROP if keep is not None else 0.0, residual)
    f32, out16 = feature in ("f32", "all"), feature != "f32"
    if feature == "f32":  # the bound is relied on only where ATen's own fp32 conv2d meets it
        x32 = torch.cat([t.float() for t in xs], 3).permute(0, 3, 1, 2)
        aten = F.conv2d(x32, wt.to(dt).float(), None, case["s"], case["p"]).permute(0, 2, 3, 1) * scale[:, None, None, :] + shift[:, None, None, :]
        check_f32(aten, want, f32_bound(want, absc, absA, K), tag, "ATen fp32")

    for k_, v_ in case["switches"].items():
        form_switch.setenv(k_, v_)
    out = pinned(eng, expect, lambda: eng.op_conv2d_ex(
        xs[0].cuda(), wt, case["s"], case["p"], scale.cuda(), shift.cuda(), act=act, path=case["path"],
        x1=xs[1].cuda() if len(xs) > 1 else None, residual=None if residual is None else residual.cuda(), out16=out16, out_f32=f32,
        coef_div=coef_div, mask=keep.cuda() if feature == "mask2" else None, p=P_DROP if keep is not None else 0.0,
        rng_site=SITE if feature in ("rng1", "all") else None, rng_row_offset=ROW0, rng_forward=FWD))
    if feature == "f32":
        check_f32(out, want, f32_bound(want, absc, absA, K), f"{tag} {dtype}", expect)
        return
    y16, y32 = out if f32 else (out, None)
    check16(y16, want, dtype, tag)
    if keep is not None and residual is None:
        exact_mask(y16, keep, pre, tag)
    if y32 is not None:  # both stores come from the same registers: the 16-bit tensor is the rounded fp32 one
        check16(y32, want, dtype, tag + " (fp32 store)")
        assert torch.equal(y32.to(dt), y16), tag


# ------------------------------------------------------------------------------------------------ (ii) skinny in its own right
def make(case, dtype, tag, two=None):
    """(n, h, w, cin, cout, k, s, p) -> 16-bit x (split into `two` = (c0, c1) sources if given), weights, affine rows, float64 conv."""
    n, h, w, cin, cout, k, s, p = case
    dt = DTYPES[dtype]
    g = torch.Generator().manual_seed(zlib.crc32(repr((case, dtype, tag, two)).encode()))
    xs = [torch.randn(n, h, w, c, generator=g).to(dt) for c in (two or (cin,))]
    wt = torch.randn(cout, cin, k, k, generator=g) / (cin * k * k) ** 0.5
    scale, shift = 1.0 + 0.3 * torch.randn(n, cout, generator=g), 0.2 * torch.randn(n, cout, generator=g)
    raw, absc = conv_f64(xs, wt, s, p, dt)
    return xs, wt, scale, shift, raw, absc


def launch(eng, xs, wt, case, scale, shift, act=2, **kw):
    return eng.op_conv2d_ex(xs[0].cuda(), wt, case[6], case[7], scale.cuda(), shift.cuda(), act=act, path=1,
                            x1=xs[1].cuda() if len(xs) > 1 else None, **kw)


WAVES = {"w16": (SKINNY, {}), "w8": (SKINNY8, {"DYF_SKINNY_W8_FROM": 1})}
SKINNY_CASES = [
    # K extremes: nk = 4 (the fewest steps the form takes: one k16 sub-step per wave), nk = 32 (the most: 8 / 16 per wave)
    ((3, 5, 7, 256, 128, 1, 1, 0), None),        # M = 105
    ((3, 6, 10, 512, 128, 2, 2, 0), None),       # M = 45
    # 4 nk sub-steps that do not divide by 16: 3x3 / p1 with 64 (36 sub-steps) and 128 channels (72), taps in the zero padding
    ((2, 7, 5, 64, 128, 3, 1, 1), None),
    ((2, 7, 5, 128, 256, 3, 1, 1), None),
    ((2, 8, 12, 64, 128, 4, 2, 1), None),        # 4x4 / s2 / p1: border taps lie in the zero padding, nk = 16
    # ragged M: less than one tile; planes of 4 x 4 where one 32-pixel tile spans two and three samples
    ((1, 3, 3, 256, 128, 1, 1, 0), None),        # M = 9
    ((5, 8, 8, 512, 512, 2, 2, 0), None),        # M = 80
    # a wave's share of K straddles the two sources: 2x2 / s2 with 192 + 128 (20 steps, the sources meet at step 12: wave 9 of 16
    # owns sub-steps 45..49, wave 4 of 8 owns 40..49, the boundary is sub-step 48), and the other way round
    ((3, 6, 10, 320, 128, 2, 2, 0), (192, 128)),
    ((3, 6, 10, 320, 128, 2, 2, 0), (128, 192)),
]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("waves", ["w16", "w8"])
@pytest.mark.parametrize("case,two", SKINNY_CASES, ids=lambda v: "x".join(map(str, v)) if v else "one")
def test_skinny_shapes(engines, form_switch, case, two, waves, dtype):
    """conv_skinny_kernel_t<16> and <8> at the edges of what conv_skinny_supported admits; run to run bit for bit."""
    eng = engines(dtype)
    expect, sw = WAVES[waves]
    xs, wt, scale, shift, raw, _ = make(case, dtype, "skinny", two)
    for k_, v_ in sw.items():
        form_switch.setenv(k_, v_)
    y = pinned(eng, expect, lambda: launch(eng, xs, wt, case, scale, shift))
    check16(y, epilogue_f64(raw, scale, shift, act=2)[0], dtype, f"skinny {case} {two} {waves}")
    again = pinned(eng, expect, lambda: launch(eng, xs, wt, case, scale, shift))
    assert torch.equal(y, again)


PROD = (20, 16, 16, 512, 512, 2, 2, 0)   # enc4 of unet_simple at 20 rows: 640 workgroups, 40 tiles of 128 x 128


@pytest.fixture(scope="module")
def prod():
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = make(PROD, dtype, "prod")
        return made[dtype]
    return get


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_skinny_eight_waves_at_the_production_shape(engines, form_switch, prod, dtype):
    """The shape enc4 / dec1 run at 20 rows takes conv_skinny_kernel_t<8> by the production rule (>= 513 workgroups); the same
    inputs on the 16-wave form (DYF_SKINNY_W8_FROM raised) and on split-K implicit GEMM (DYF_SKINNY=0) meet the reference too, and
    the three agree to the summation-order bound."""
    eng = engines(dtype)
    xs, wt, scale, shift, raw, _ = prod(dtype)
    want = epilogue_f64(raw, scale, shift, act=2)[0]
    y8 = pinned(eng, SKINNY8, lambda: launch(eng, xs, wt, PROD, scale, shift))
    check16(y8, want, dtype, "prod <8>")
    assert torch.equal(y8, pinned(eng, SKINNY8, lambda: launch(eng, xs, wt, PROD, scale, shift)))  # run to run
    form_switch.setenv("DYF_SKINNY_W8_FROM", 1 << 30)
    y16 = pinned(eng, SKINNY, lambda: launch(eng, xs, wt, PROD, scale, shift))
    check16(y16, want, dtype, "prod <16>")
    form_switch.delenv("DYF_SKINNY_W8_FROM")
    form_switch.setenv("DYF_SKINNY", 0)
    ysk = pinned(eng, IGEMM128_SK, lambda: launch(eng, xs, wt, PROD, scale, shift))
    check16(ysk, want, dtype, "prod split-K")
    for a, b, what in [(y8, y16, "<8> vs <16>"), (y8, ysk, "<8> vs split-K"), (y16, ysk, "<16> vs split-K")]:
        rr = rel_rms(a.float().cpu(), b.float().cpu())
        print(f"[forms] prod {dtype} {what}: rel-RMS {rr:.3e}")
        assert rr <= 2.5e-3, (what, rr)


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
def test_skinny_is_batch_invariant_bit_for_bit(engines, form_switch, prod, dtype):
    """conv_skinny.hip: "the summation order of an output element fixed whatever the batch"; launch_conv_skinny: the wave count
    follows n_sel.  Row r of an n-row launch equals the sample launched alone in the same wave-count form -- also where a 32-pixel tile
    is shared with the neighbours (4 x 4 planes: tile 0 = samples 0, 1; tile 1 = samples 2, 3; tile 2 = sample 4 alone, ragged) --
    and a one-row launch pinned to 20 rows (n_sel) runs <8> and equals row r of the 20-row launch."""
    eng = engines(dtype)
    case = (5, 8, 8, 512, 512, 2, 2, 0)
    xs, wt, scale, shift, _, _ = make(case, dtype, "invariant")
    one = (1,) + case[1:]
    for waves in ("w16", "w8"):
        expect, sw = WAVES[waves]
        for k_, v_ in sw.items():
            form_switch.setenv(k_, v_)
        full = pinned(eng, expect, lambda: launch(eng, xs, wt, case, scale, shift))
        for r in (0, 1, 2, 4):
            alone = pinned(eng, expect, lambda: launch(eng, [xs[0][r:r + 1].contiguous()], wt, one, scale[r:r + 1], shift[r:r + 1]))
            assert torch.equal(alone[0], full[r]), (waves, r)
        form_switch.delenv("DYF_SKINNY_W8_FROM")
    xs, wt, scale, shift, _, _ = prod(dtype)
    full = pinned(eng, SKINNY8, lambda: launch(eng, xs, wt, PROD, scale, shift))
    one = (1,) + PROD[1:]
    for r in (0, 7, 19):
        args = ([xs[0][r:r + 1].contiguous()], wt, one, scale[r:r + 1], shift[r:r + 1])
        alone = pinned(eng, SKINNY8, lambda: launch(eng, *args, n_sel=20))
        assert torch.equal(alone[0], full[r]), r
        pinned(eng, SKINNY, lambda: launch(eng, *args))  # without n_sel the one-row launch is the 16-wave form


# ------------------------------------------------------------------------------------------------ (iii) dropout is exact
DROP_FORMS = ["skinny", "skinny<8>", "igemm2<1>-ragged", "igemm2<2>-ragged", "halo<5>-ragged", "rows<2>", "igemm128", "direct"]


@pytest.mark.parametrize("dtype", ["bf16", "fp16"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("name", DROP_FORMS)
def test_dropout_masks_are_exact(engines, form_switch, name, mode, dtype):
    """No activation, non-zero shift: no reference element is zero in front of the mask (asserted on the CPU), so the output is zero
    exactly where the mask drops -- for the generator's masks (mode 1, rebuilt by tests/rng_host at a non-zero row offset) and for an
    injected mask (mode 2) -- on forms whose epilogues index the elements differently.  The numeric bound holds on the kept ones."""
    eng, dt = engines(dtype), DTYPES[dtype]
    case = next(c for c in FORM_CASES if c["name"] == name)
    xs, wt, raw, _ = operands(case, "base", dtype)
    n, ho, wo, cout = raw.shape
    g = torch.Generator().manual_seed(zlib.crc32(f"drop {name} {mode}".encode()))
    scale, shift = 1.0 + 0.3 * torch.randn(n, cout, generator=g), 0.5 + 0.2 * torch.randn(n, cout, generator=g)
    keep = rng_keep(n, ho, wo, cout) if mode == 1 else (torch.rand(n, ho, wo, cout, generator=g) >= P_DROP).to(torch.uint8)
    want, pre, _ = epilogue_f64(raw, scale, shift, act=0, keep=keep, p=P_DROP)
    assert bool((pre != 0).all())
    for k_, v_ in case["switches"].items():
        form_switch.setenv(k_, v_)
    eng.seed(SEED)
    y = pinned(eng, case["expect"], lambda: eng.op_conv2d_ex(
        xs[0].cuda(), wt, case["s"], case["p"], scale.cuda(), shift.cuda(), act=0, path=case["path"], p=P_DROP,
        mask=keep.cuda() if mode == 2 else None, rng_site=SITE if mode == 1 else None, rng_row_offset=ROW0, rng_forward=FWD))
    exact_mask(y, keep, pre, f"{name} mode {mode}")
    kept = keep != 0
    check16(y.cpu()[kept][None, None, None], want[kept][None, None, None], dtype, f"drop {name} mode {mode}", borders=False)
    check16(y, want, dtype, f"drop {name} mode {mode} (whole)")
    if mode == 1:  # the masks follow the GLOBAL row: the same launch at another offset draws other masks
        assert not torch.equal(rng_keep(n, ho, wo, cout, ROW0 + 1), keep)


# ------------------------------------------------------------------------------------------------ the seam refuses, never truncates
def test_the_seam_refuses_what_the_argument_block_cannot_express(engines):
    eng = engines("bf16")
    x = torch.zeros(2, 8, 8, 64, dtype=torch.bfloat16).cuda()
    wt = torch.zeros(128, 64, 1, 1)
    ok = dict(stride=1, pad=0)
    with pytest.raises(ValueError):
        eng.op_conv2d_ex(x, wt, act=5, **ok)
    with pytest.raises(ValueError):
        eng.op_conv2d_ex(x, wt, p=1.0, mask=torch.ones(2, 8, 8, 128, dtype=torch.uint8).cuda(), **ok)
    with pytest.raises(ValueError):
        eng.op_conv2d_ex(x, wt, coef_div=2, **ok)   # coefficient rows per pair of samples, but no coefficients
    with pytest.raises(ValueError):                # mode 1 draws from the engine's row-key table: 2 max_batch = 32 rows
        eng.op_conv2d_ex(torch.zeros(33, 2, 2, 64, dtype=torch.bfloat16).cuda(), wt, rng_site=0, p=0.1, **ok)
    with pytest.raises(ValueError):
        eng.op_conv2d_ex(x, torch.zeros(128, 64, 9, 9), **ok)   # kernel larger than the padded input
    with pytest.raises(NotImplementedError):
        eng.op_conv2d_ex(x[..., :32].contiguous(), torch.zeros(128, 32, 1, 1), **ok)   # the MFMA path needs 64-channel chunks
