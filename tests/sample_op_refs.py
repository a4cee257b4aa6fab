"""Plain references of the 16-bit sampling kernels between the convs (dyffusion_amd/csrc/unet_kernels.hip, csrc/kernels.hip), the cases
tests/test_gpu_sample_ops.py runs them at through HipEngine.op_sample (dyf_op_sample16), and the bound -- test infrastructure, no GPU.

Every op is a pure torch function of a few lines, NHWC in and out like the seam; it computes in the dtype of its arguments (float64 for
the reference, float32 for the "what does fp32 arithmetic cost" baseline).  The statements tests/train_op_refs.py already has are
reused (its activations, resample matrices, LayerNorm, nearest upsample); what the sampling path adds is stated here: the head, the
stem conv, the commuted upsample epilogue, GroupNorm from conv-epilogue partials, FiLM rows with a stride, the residual.

Inputs are drawn in float64 and rounded to the build's 16-bit type FIRST, so the reference and the kernel see the same numbers.
GroupNorm / LayerNorm inputs carry a per-group offset of about 4 standard deviations and a per-channel scale: the kernels finalise
E[x^2] - mean^2 and must survive that cancellation (a larger offset only makes the 16-bit input grid itself coarse).

The bound (ops with a 16-bit output): with `ref` the float64 result and r16 = round16(ref), rounded to nearest even,
    floor = rms(r16 - ref) / rms(ref)          what rounding ONCE costs
    excess = rms(got - r16) / rms(ref)         what the kernel adds to it
and excess <= floor.  A correct kernel evaluates in fp32 and rounds once: it differs from r16 only where an fp32 error of ~1e-6 carries
a value across a 16-bit rounding boundary, and then by one 16-bit ulp; excess <= floor allows about one element in twelve to do so
(a fraction f of elements off by one ulp gives excess = sqrt(f) ulp, the floor is ulp / sqrt(12)).  No number is tuned to the code
under test.  tests/test_sample_op_refs.py shows that fp32 torch, rounded once, sits inside floor / 2 on every case and that the
`mutant=` versions -- each a mistake a kernel here could make -- do not pass.
"""
import math

import numpy as np
import torch

from tests import rng_host
from tests import train_op_refs as T

TOL_F32 = T.TOL  # rel-RMS of an fp32 output (HEAD) against float64
SEED, ROW_OFFSET, SITE, FORWARD = 20261019, 5, 3, 2  # generator dropout: dyf_seed, global index of batch row 0, dropout site, forward index
DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


# ------------------------------------------------------------------------------------------------------------- rounding, the bound
def round16(t, dt):
    """float64 -> the 16-bit type `dt`, round to nearest even in ONE step (through fp32 a value can round twice: the neighbours of the
    two-step result are tried against the float64 value)."""
    x = t.double()
    r = x.float().to(dt)
    i = r.view(torch.int16).to(torch.int32)
    cands = [r.double()] + [(i + d).clamp(-32768, 32767).to(torch.int16).view(dt).double() for d in (-1, 1)]
    err = torch.stack([torch.nan_to_num((c - x).abs(), nan=math.inf, posinf=math.inf) for c in cands])
    pick = err.argmin(0)  # the first minimum: a true tie keeps the nearest-even result
    return torch.stack(cands).gather(0, pick[None])[0].to(dt)


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def excess_floor(got, ref, dt):
    """(excess, floor) of a 16-bit result `got` against the float64 `ref`."""
    r16 = round16(ref, dt).double()
    den = max(rms(ref), 1e-300)
    return rms(got.double().reshape(ref.shape) - r16) / den, rms(r16 - ref.double()) / den


# ----------------------------------------------------------------------------------------------------------------------- the ops
def _act(v, act):
    return v if act == "none" else T._act(v, act)


def _drop(y, keep, p):
    return y if keep is None else y * keep * (1.0 / (1.0 - p))


def _group_stats(z, groups, mutant=None, part=None):
    """(mean, var) per (sample, group), biased: from the tensor, or from conv-epilogue partials part (nb, slots, C / 8, 2) = (sum, sum of
    squares) per 8-channel octet."""
    nb, h, w, C = z.shape
    cpg = C // groups
    if part is not None:
        pt = part.to(z.dtype)
        if mutant == "slot_dropped":
            pt = pt[:, :-1]
        s = pt.sum(1).reshape(nb, groups, cpg // 8, 2).sum(2)
        mean = s[..., 0] / (h * w * cpg)
        return mean, s[..., 1] / (h * w * cpg) - mean * mean
    zg = z.reshape(nb, h * w, groups, cpg)
    if mutant == "last_pixel":  # the statistics miss the last pixel of the plane
        zg = zg[:, :-1]
    return zg.mean((1, 3)), zg.var((1, 3), unbiased=mutant == "unbiased")


def group_norm(z, gamma, beta, groups, act="none", film=None, film_div=1, residual=None, keep=None, p=0.0, part=None, mutant=None):
    """GroupNorm (biased variance, eps 1e-5) -> FiLM rows (a, c): y * a + c, row = sample // film_div -> activation -> Dropout
    (-> + residual): z (nb,h,w,C).  launch_gn_act (16-bit z, optional partials) and launch_groupnorm (fp32 z)."""
    nb, _, _, C = z.shape
    mean, var = _group_stats(z, groups, mutant, part)
    idx = torch.arange(C) // (C // groups)
    eps = 0.0 if mutant == "no_eps" else 1e-5
    v = (z - mean[:, None, None, idx]) * (var + eps).rsqrt()[:, None, None, idx] * gamma + beta
    if film is not None:
        row = torch.arange(nb) // max(film_div, 1)
        v = v * film[0][row, None, None, :C]
        if mutant != "film_shift":
            v = v + film[1][row, None, None, :C]
    y = _act(v, act)
    if residual is not None and mutant == "residual_before_drop":
        return _drop(y + residual, keep, p)
    y = _drop(y, keep, p)
    return y if residual is None else y + residual


def layernorm_c(x, g, keep=None, p=0.0, mutant=None):
    """unet.LayerNorm over the channels of a pixel + Dropout (train_op_refs.layernorm; two more mutants)."""
    if mutant in (None, "unbiased"):
        return T.layernorm(x, g.reshape(1, -1, 1, 1), keep, p, mutant)
    mean, var = x.mean(-1, keepdim=True), x.var(-1, unbiased=False, keepdim=True)
    if mutant == "tail_pixel":  # the last pixel of the launch normalised by its neighbour's statistics
        f = lambda t: torch.cat([t.reshape(-1, 1)[:-1], t.reshape(-1, 1)[-2:-1]]).reshape(t.shape)
        mean, var = f(mean), f(var)
    y = (x - mean) * (var + (0.0 if mutant == "no_eps" else 1e-5)).rsqrt() * g.reshape(-1)
    return _drop(y, keep, p)


def head(x, w, b, mutant=None):
    """final 1x1 conv: x (nb,h,w,C), w (cout,C), b (cout) -> NCHW (nb,cout,h,w)."""
    if mutant == "last_chunk":  # the last 8-channel chunk never reaches the dot product
        x, w = x[..., :-8], w[:, :-8]
    y = x @ w.T
    return (y if mutant == "no_bias" else y + b).permute(0, 3, 1, 2)


def stem_conv(srcs, w, b, pad, mutant=None):
    """init_conv over the channel concatenation of NCHW sources: taps reach from -pad to k-1-pad, the plane keeps its size -> NHWC."""
    x = torch.cat(srcs, 1).permute(0, 2, 3, 1)
    nb, h, wd, ci = x.shape
    k = w.shape[2]
    xp = torch.zeros(nb, h + k - 1, wd + k - 1, ci, dtype=x.dtype)
    xp[:, pad:pad + h, pad:pad + wd] = x
    y = 0
    for ky in range(k):
        for kx in range(k):
            if mutant == "tap_dropped" and (ky, kx) == (k - 1, k - 1):
                continue
            y = y + xp[:, ky:ky + h, kx:kx + wd] @ w[:, :, ky, kx].T
    return y + b


def _up_matrix(n_in, dtype, mutant=None):
    M = T._resample_matrix(n_in, 2 * n_in, False, dtype)
    if mutant == "border_mirrored" and n_in > 1:  # the clamped tap of the two border outputs taken from the inside instead
        M[0], M[-1] = 0, 0
        M[0, 0], M[0, 1], M[-1, -1], M[-1, -2] = 0.75, 0.25, 0.75, 0.25
    return M


def up2_bilinear(x, x2=None, mutant=None):
    """Upsample(x2, bilinear, align_corners=False) of x or of cat([x, x2]) (train_op_refs.up2_bilinear; two more mutants)."""
    if x2 is not None:
        x = torch.cat([x, x2.roll(8, -1) if mutant == "second_source_shift8" else x2], -1)
    rows = torch.einsum("oh,bhwc->bowc", _up_matrix(x.shape[1], x.dtype, mutant), x)
    return torch.einsum("pw,bowc->bopc", _up_matrix(x.shape[2], x.dtype, mutant), rows)


def up2_epilogue(lo, a, c, coef_div=1, act="none", keep=None, p=0.0, mutant=None):
    """The commuted 1x1 decoder block: drop(act(up2(lo) * a + c)), coefficient row = sample // coef_div."""
    C = lo.shape[-1]
    row = torch.arange(lo.shape[0]) // max(coef_div, 1)
    v = up2_bilinear(lo, mutant=mutant) * a[row, None, None, :C]
    if mutant != "film_shift":
        v = v + c[row, None, None, :C]
    return _drop(_act(v, act), keep, p)


def drop16(x, keep, p):
    return x * keep * (1.0 / (1.0 - p))


# --------------------------------------------------------------------------------------------------------------------- the cases
class Built:
    """One case, drawn for one 16-bit type: `xs` / `params` / `kw` are the arguments of HipEngine.op_sample (CPU tensors), `ref(dtype,
    mutant)` the reference, `kind` how the output is compared ("r16": excess <= floor, "f32": rel-RMS, "exact": bitwise), `form` the
    name the launcher notes in the form log (None: it notes none of `quiet`), `switch` the DYF_* form switches, `gen`: (h, w, c) of the
    output when the keep mask is the engine generator's."""

    def __init__(self, op, xs, params, kw, fn, kind="r16", form=None, quiet=(), switch=None, gen=None, p=0.0, keep=None):
        self.op, self.xs, self.params, self.kw, self.fn, self.kind = op, xs, params, kw, fn, kind
        self.form, self.quiet, self.switch, self.gen, self.p, self.keep = form, quiet, dict(switch or {}), gen, p, keep

    def ref(self, dtype=torch.float64, mutant=None):
        c = lambda t: None if t is None else t.to(dtype)
        return self.fn(c, mutant)


def gen_keep(shape_hwc, nb, p):
    """The keep mask the engine's generator draws (dyf_seed(SEED), forward FORWARD, site SITE, rows ROW_OFFSET ..), rebuilt on the host."""
    rows = [rng_host.row_mask_nhwc(shape_hwc, p, SEED, FORWARD, SITE, ROW_OFFSET + r) for r in range(nb)]
    return torch.from_numpy(np.stack(rows).astype(np.float64))


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 6151 * (int(v) + 17) for i, v in enumerate(key)) % (2 ** 31))


def _rn(g, *shape, scale=1.0):
    return torch.randn(*shape, generator=g, dtype=torch.float64) * scale


def _offset_input(g, nb, hw, C, groups, tiny=False, per_pixel=False):
    """(nb, h, w, C) float64: unit noise + an offset of ~4 sigma per (sample, group) -- per pixel for LayerNorm -- times a per-channel
    scale in [0.5, 1.5]; `tiny`: all of it times 2^-8, where the variance is comparable to eps = 1e-5 (a floating-point grid is as
    fine there)."""
    h, w = T._grid(hw)
    x = _rn(g, nb, h, w, C)
    if per_pixel:
        x = x + 4.0 * torch.sign(_rn(g, nb, h, w, 1)) * (1.0 + 0.1 * _rn(g, nb, h, w, 1))
    else:
        off = 4.0 * torch.sign(_rn(g, nb, groups)) * (1.0 + 0.1 * _rn(g, nb, groups))
        x = x + off[:, None, None, torch.arange(C) // (C // groups)]
    x = x * (0.5 + torch.rand(C, generator=g, dtype=torch.float64))
    return x * 2.0 ** -8 if tiny else x


def _affine(g, C):
    return (1.0 + _rn(g, C, scale=0.3)).float(), _rn(g, C, scale=0.3).float()


def _film_rows(g, rows, C, stride):
    """FiLM rows (rows, stride) fp32: (1 + scale) and shift in the first C columns, junk a kernel must not read behind them."""
    a, c = torch.full((rows, stride), 1e4), torch.full((rows, stride), -1e4)
    a[:, :C], c[:, :C] = (1.0 + _rn(g, rows, C, scale=0.3)).float(), _rn(g, rows, C, scale=0.5).float()
    return a, c


def _partials(x16, slots):
    """What a conv epilogue leaves: per sample, `slots` contiguous pixel ranges x 8-channel octets of (sum, sum of squares), summed in
    float64, stored fp32."""
    nb, h, w, C = x16.shape
    x = x16.double().reshape(nb, h * w, C // 8, 8)
    out = torch.zeros(nb, slots, C // 8, 2, dtype=torch.float64)
    for s, idx in enumerate(np.array_split(np.arange(h * w), slots)):
        out[:, s, :, 0], out[:, s, :, 1] = x[:, idx].sum((1, 3)), x[:, idx].pow(2).sum((1, 3))
    return out.float()


def _mask(g, shape, p):
    return (torch.rand(*shape, generator=g) >= p).to(torch.uint8)


def _drop_kw(g, drop, shape, p, kw):
    """-> (keep float64 or None, gen shape or None); fills op_sample's dropout arguments."""
    if drop == "mask":
        kw.update(mask=_mask(g, shape, p), p=p)
        return kw["mask"].double(), None
    if drop == "gen":
        kw.update(p=p, rng_site=SITE, rng_row_offset=ROW_OFFSET, rng_forward=FORWARD)
        return gen_keep(shape[1:], shape[0], p), tuple(shape[1:])
    return None, None


GN_FORMS = ("gn_stats_kernel+gn_apply", "gn_apply_part_kernel", "gn_finalize_part_kernel+gn_apply")
P_DROP = 0.3


def specs(op):
    """(id, arguments) of every case of `op`: the smallest shapes at which each launcher branch is reached."""
    S = []
    if op == "gn_act":  # (C, hw, nb, groups, extras)
        def gn(cid, C, hw, nb=3, **kw):
            S.append((cid, dict(C=C, hw=hw, nb=nb, **kw)))
        gn("fallback-C32-hw35", 32, 35)                       # 4 channels per group: gn_act_kernel
        gn("fallback-C8-hw1", 8, 1)                           # groups of ONE element
        gn("fallback-C64-hw33-nostats", 64, 33, stats=False)
        gn("fallback-C32-hw35-tiny", 32, 35, tiny=True)
        for hw in (1, 33, 128, 129, 225):                     # register statistics + walk apply: 32 pixel rows / 128 apply pixels per workgroup
            gn(f"walk-C64-hw{hw}", 64, hw)
        gn("walk-C64-hw8281-nb1", 64, 8281, nb=1)             # statistics grid at its cap of 64, 4-way unrolled loop with a remainder
        gn("walk-C64-hw129-tiny", 64, 129, tiny=True)
        gn("walk-C128-hw65", 128, 65)                         # lane-mapping boundaries: 16, 64, 128, 256 chunks
        gn("walk-C512-hw17", 512, 17)
        gn("walk-C1024-hw9", 1024, 9)
        gn("walk-C2048-hw5", 2048, 5)
        gn("atomic-C192-hw37", 192, 37)                       # 24 chunks: LDS-atomic statistics + gn_apply_kernel
        gn("atomic-C192-hw37-tiny", 192, 37, tiny=True)
        gn("apply-C64-hw129-nowalk", 64, 129, switch={"DYF_GN_WALK": "0"})
        gn("part-C64-hw33-slots1", 64, 33, slots=1)
        gn("part-C64-hw33-slots3", 64, 33, slots=3)
        gn("part-C64-hw33-slots3-tiny", 64, 33, slots=3, tiny=True)
        gn("finpart-C64-hw130-slots65", 64, 130, slots=65)    # the smallest slot count past the 1024 threshold
        gn("finpart-C64-hw260-slots130", 64, 260, slots=130)  # the 128-lane slot loop runs twice
        gn("finpart-C512-hw17-slots9", 512, 17, slots=9)
        gn("finpart-C64-hw130-slots65-tiny", 64, 130, slots=65, tiny=True)
        for cid, kw in (("film", dict(film=1)), ("residual", dict(residual=1)), ("noact", dict(act="none")), ("maskdrop", dict(drop="mask")),
                        ("gendrop", dict(drop="gen")), ("all-mask", dict(film=1, residual=1, drop="mask")),
                        ("all-gen", dict(film=1, residual=1, drop="gen")), ("all-gen-noact", dict(film=1, residual=1, drop="gen", act="none"))):
            gn(f"walk-C64-hw129-{cid}", 64, 129, **kw)
        gn("part-C64-hw33-slots3-all-mask", 64, 33, slots=3, film=1, residual=1, drop="mask")
        gn("fallback-C32-hw35-all-gen", 32, 35, film=1, residual=1, drop="gen")
        gn("atomic-C192-hw37-all-mask", 192, 37, film=1, residual=1, drop="mask")
    elif op == "layernorm_c":  # (C, hw, nb, drop)
        S = [(f"vec-C{c}-hw33", dict(C=c, hw=33, nb=3)) for c in (8, 64, 512)]  # 99 pixels: the last workgroup is partial, dead lanes clamped
        S += [("vec-C64-hw1", dict(C=64, hw=1, nb=3)), ("fallback-C24-hw33", dict(C=24, hw=33, nb=3)), ("fallback-C1024-hw9", dict(C=1024, hw=9, nb=3)),
              ("vec-C64-hw33-maskdrop", dict(C=64, hw=33, nb=3, drop="mask")), ("vec-C64-hw33-gendrop", dict(C=64, hw=33, nb=3, drop="gen")),
              ("fallback-C24-hw33-gendrop", dict(C=24, hw=33, nb=3, drop="gen")),
              ("vec-C64-hw33-tiny", dict(C=64, hw=33, nb=3, tiny=True)), ("fallback-C24-hw33-tiny", dict(C=24, hw=33, nb=3, tiny=True))]
    elif op == "head":  # (C, cout, hw, nb)
        S = [("vec-C8-co1", dict(C=8, co=1, hw=35, nb=3)), ("vec-C64-co3-hw225", dict(C=64, co=3, hw=225, nb=3)),  # 675 pixels: the grid-stride loop ends mid-wave
             ("vec-C512-co4", dict(C=512, co=4, hw=35, nb=3)), ("pixel16B-C24-co2", dict(C=24, co=2, hw=35, nb=3)),
             ("generic-C20-co3", dict(C=20, co=3, hw=35, nb=3)), ("generic-C64-co5", dict(C=64, co=5, hw=35, nb=3))]
    elif op == "up2_nearest":
        S = [(f"C{c}-{h}x{w}", dict(C=c, h=h, w=w, nb=3)) for c in (64, 12) for h, w in ((1, 1), (3, 5))]
    elif op == "drop16":
        S = [("5x7x8-mask", dict(drop="mask")), ("5x7x8-gen", dict(drop="gen"))]
    elif op == "stem_conv":  # (dim, k, pad, channels per source, plane)
        def st(cid, dim, k, ch, pad=None, **kw):
            for h, w in ((1, 1), (5, 7)):  # 35 pixels: a partial last 32-pixel group
                S.append((f"{cid}-{h}x{w}", dict(dim=dim, k=k, ch=ch, pad=(k - 1) // 2 if pad is None else pad, h=h, w=w, nb=3, **kw)))
        st("valu-d32-k7-c2", 32, 7, (2,))
        st("valu-d64-k7-c9", 64, 7, (4, 3, 1, 1))             # cin * ts = 36 > 32: four sources
        st("valu-d64-k6-c2", 64, 6, (2,))                     # ts = 3
        st("mfma-d64-k3-c5", 64, 3, (5,), mfma=1)             # ts = 1
        st("mfma-d64-k5-c3", 64, 5, (3,), mfma=1)             # ts = 2
        st("mfma-d64-k7-c2", 64, 7, (2,), mfma=1)             # one source
        st("mfma-d64-k7-c1+1", 64, 7, (1, 1), mfma=1)         # 1 + 1 channels from two sources
        st("mfma-d64-k7-c8", 64, 7, (3, 2, 2, 1), mfma=1)     # the 32-step limit, four sources
        st("valu-d64-k7-c2-nomfma", 64, 7, (2,), switch={"DYF_STEM_MFMA": "0"})
    elif op == "groupnorm_f32":  # (C, groups, hw, nb, extras)
        def gf(cid, C, g, hw, nb=3, **kw):
            S.append((cid, dict(C=C, groups=g, hw=hw, nb=nb, **kw)))
        gf("wave4-C64-hw16", 64, 8, 16, wave=1)
        gf("wave4-C64-hw128", 64, 8, 128, wave=1)             # 256 pieces: the limit of <4>
        gf("wave8-C64-hw129", 64, 8, 129, wave=1)
        gf("wave8-C64-hw256", 64, 8, 256, wave=1)             # 512 pieces: the limit of <8>
        gf("block-C64-hw257", 64, 8, 257)
        gf("block-C24-g4-hw16", 24, 4, 16)                    # 6 channels per group
        gf("block-C64-hw16-nowave", 64, 8, 16, switch={"DYF_GN_WAVE": "0"})
        gf("wave4-C16-g2-hw16", 16, 2, 16, wave=1)            # six (sample, group) waves: the second workgroup is half empty
        gf("wave4-C64-hw16-filmdiv2-nb4", 64, 8, 16, nb=4, film=1, film_div=2, wave=1)
        gf("wave4-C64-hw16-film-relu", 64, 8, 16, film=1, act="relu", wave=1)
        gf("wave8-C64-hw129-film-leaky-maskdrop", 64, 8, 129, film=1, act="leaky", drop="mask", wave=1)
        gf("block-C64-hw257-film-relu-maskdrop", 64, 8, 257, film=1, act="relu", drop="mask")
        gf("wave4-C64-hw16-tiny", 64, 8, 16, tiny=True, wave=1)
        gf("wave8-C64-hw129-tiny", 64, 8, 129, tiny=True, wave=1)
        gf("block-C64-hw257-tiny", 64, 8, 257, tiny=True)
    elif op == "up2_bilinear":  # (c0, c1, h, w)
        S = [(f"quad-{c0}+{c1}-{h}x{w}", dict(c0=c0, c1=c1, h=h, w=w, nb=3, quad=1)) for c0, c1 in ((64, 0), (64, 64)) for h, w in ((2, 2), (3, 5))]
        S += [("vec-64+64-1x4", dict(c0=64, c1=64, h=1, w=4, nb=3)), ("vec-64+64-3x5-noquad", dict(c0=64, c1=64, h=3, w=5, nb=3, switch={"DYF_UP2X_QUAD": "0"})),
              ("scalar-12+4-3x5", dict(c0=12, c1=4, h=3, w=5, nb=3))]
    elif op == "up2_epilogue":  # (C, h, w, extras)
        S = [(f"C{c}-{h}x{w}", dict(C=c, h=h, w=w, nb=3)) for c in (4, 64) for h, w in ((1, 1), (1, 3), (3, 5))]
        S += [("C64-3x5-coefdiv2-nb4", dict(C=64, h=3, w=5, nb=4, coef_div=2)), ("C64-3x5-relu", dict(C=64, h=3, w=5, nb=3, act="relu")),
              ("C4-3x5-leaky", dict(C=4, h=3, w=5, nb=3, act="leaky")), ("C64-3x5-relu-maskdrop", dict(C=64, h=3, w=5, nb=3, act="relu", drop="mask")),
              ("C4-3x5-leaky-maskdrop", dict(C=4, h=3, w=5, nb=3, act="leaky", drop="mask"))]
    return S


OPS = ("gn_act", "layernorm_c", "head", "up2_nearest", "drop16", "stem_conv", "groupnorm_f32", "up2_bilinear", "up2_epilogue")


def build(op, a, dtname):
    """Draw one case for the 16-bit type `dtname` ("bf16" | "fp16")."""
    dt = DTYPES[dtname]
    r16 = lambda t: round16(t, dt)
    if op == "gn_act":
        C, hw, nb, groups = a["C"], a["hw"], a["nb"], a.get("groups", 8)
        g = _gen(1, C, hw, nb, a.get("slots", 0), a.get("tiny", 0))
        x = r16(_offset_input(g, nb, hw, C, groups, a.get("tiny", False)))
        gamma, beta = _affine(g, C)
        act = a.get("act", "silu")
        kw = dict(groups=groups, act=act, stats=a.get("stats", True))
        film = res = part = None
        if a.get("film"):
            film = _film_rows(g, nb, C, 2 * C)
            kw.update(film_a=film[0], film_c=film[1])
        if a.get("residual"):
            res = kw["residual"] = r16(_rn(g, *x.shape))
        if a.get("slots"):
            part = kw["part"] = _partials(x, a["slots"])
        keep, gen = _drop_kw(g, a.get("drop"), x.shape, P_DROP, kw)
        vec = C % 8 == 0 and (C // groups) % 8 == 0
        if part is not None:  # (launch_gn_act: more than 4 KB of partials per sample are finalised once per sample)
            form = GN_FORMS[2] if a["slots"] * (C // 8) * 2 > 1024 and kw["stats"] else GN_FORMS[1]
        else:
            form = GN_FORMS[0] if vec and kw["stats"] else None
        fn = lambda c, m: group_norm(c(x), c(gamma), c(beta), groups, act, None if film is None else (c(film[0]), c(film[1])), 1, c(res), c(keep),
                                     P_DROP, c(part), m)
        return Built(op, [x], [gamma, beta], kw, fn, form=form, quiet=GN_FORMS, switch=a.get("switch"), gen=gen, p=P_DROP, keep=keep)
    if op == "layernorm_c":
        C, hw, nb = a["C"], a["hw"], a["nb"]
        g = _gen(2, C, hw, nb, a.get("tiny", 0))
        x = r16(_offset_input(g, nb, hw, C, 1, a.get("tiny", False), per_pixel=True))
        gain = _affine(g, C)[0]
        kw = {}
        keep, gen = _drop_kw(g, a.get("drop"), x.shape, P_DROP, kw)
        return Built(op, [x], [gain], kw, lambda c, m: layernorm_c(c(x), c(gain), c(keep), P_DROP, m), gen=gen, p=P_DROP, keep=keep)
    if op == "head":
        C, co, hw, nb = a["C"], a["co"], a["hw"], a["nb"]
        g = _gen(3, C, co, hw, nb)
        x = r16(_rn(g, nb, *T._grid(hw), C, scale=1.5))
        w, b = _rn(g, co, C, scale=1.5 / math.sqrt(C)).float(), _rn(g, co, scale=0.5).float()
        return Built(op, [x], [w, b], {}, lambda c, m: head(c(x), c(w), c(b), m), kind="f32")
    if op == "up2_nearest":
        g = _gen(4, a["C"], a["h"], a["w"])
        x = r16(_rn(g, a["nb"], a["h"], a["w"], a["C"], scale=1.5))
        return Built(op, [x], [], {}, lambda c, m: T.up2_nearest(c(x)), kind="exact")
    if op == "drop16":
        # p = 0.5: the survivors' scale 1 / (1 - p) = 2 is exact in every format, so round16(x keep / (1 - p)) has ONE value and the
        # comparison is bitwise without a rounding-boundary caveat; every keep bit and the scale itself are still compared
        g = _gen(5, a["drop"] == "gen")
        x = r16(_rn(g, 3, 5, 7, 8, scale=1.5))
        kw = {}
        keep, gen = _drop_kw(g, a["drop"], x.shape, 0.5, kw)
        return Built(op, [x], [], kw, lambda c, m: drop16(c(x), c(keep), 0.5), kind="exact", gen=gen, p=0.5, keep=keep)
    if op == "stem_conv":
        dim, k, ch, pad, h, w, nb = a["dim"], a["k"], a["ch"], a["pad"], a["h"], a["w"], a["nb"]
        g = _gen(6, dim, k, sum(ch), len(ch), h, w)
        # the sources are fp32 network inputs: the MFMA form carries them as 16-bit hi + lo parts (hi*hi + lo*hi + hi*lo: the product is
        # short of fp32 by ~2^-16 relative in bf16), it does NOT round the operand to one 16-bit value -- so the reference takes them as they are
        srcs = [_rn(g, nb, c, h, w, scale=1.5).float() for c in ch]
        wt, b = _rn(g, dim, sum(ch), k, k, scale=1.5 / math.sqrt(sum(ch) * k * k)).float(), _rn(g, dim, scale=0.5).float()
        return Built(op, srcs, [wt, b], dict(k=k, pad=pad), lambda c, m: stem_conv([c(s) for s in srcs], c(wt), c(b), pad, m),
                     form="stem_mfma_kernel" if a.get("mfma") else None, quiet=("stem_mfma_kernel",), switch=a.get("switch"))
    if op == "groupnorm_f32":
        C, groups, hw, nb = a["C"], a["groups"], a["hw"], a["nb"]
        g = _gen(7, C, groups, hw, nb, a.get("tiny", 0))
        x = _offset_input(g, nb, hw, C, groups, a.get("tiny", False)).float()
        gamma, beta = _affine(g, C)
        act, div = a.get("act", "leaky"), a.get("film_div", 0)
        kw = dict(groups=groups, act=act, film_div=div)
        film = None
        if a.get("film"):
            film = _film_rows(g, -(-nb // div) if div > 1 else nb, C, C + 8)
            kw.update(film_a=film[0], film_c=film[1])
        keep, gen = _drop_kw(g, a.get("drop"), x.shape, P_DROP, kw)
        fn = lambda c, m: group_norm(c(x), c(gamma), c(beta), groups, act, None if film is None else (c(film[0]), c(film[1])), div, None, c(keep),
                                     P_DROP, None, m)
        return Built(op, [x], [gamma, beta], kw, fn, form="groupnorm_wave_kernel" if a.get("wave") else None, quiet=("groupnorm_wave_kernel",),
                     switch=a.get("switch"), gen=gen, p=P_DROP, keep=keep)
    if op == "up2_bilinear":
        c0, c1, h, w, nb = a["c0"], a["c1"], a["h"], a["w"], a["nb"]
        g = _gen(8, c0, c1, h, w)
        x = r16(_rn(g, nb, h, w, c0, scale=1.5))
        x2 = r16(_rn(g, nb, h, w, c1, scale=1.5)) if c1 else None
        return Built(op, [x] + ([x2] if c1 else []), [], {}, lambda c, m: up2_bilinear(c(x), c(x2), m), form="up2x_quad_kernel" if a.get("quad") else None,
                     quiet=("up2x_quad_kernel",), switch=a.get("switch"))
    if op == "up2_epilogue":
        C, h, w, nb, div, act = a["C"], a["h"], a["w"], a["nb"], a.get("coef_div", 0), a.get("act", "none")
        g = _gen(9, C, h, w, nb)
        lo = _rn(g, nb, h, w, C, scale=1.5).float()
        ca, cc = _film_rows(g, -(-nb // div) if div > 1 else nb, C, C + 4)
        kw = dict(film_a=ca, film_c=cc, film_div=div, act=act)
        keep, gen = _drop_kw(g, a.get("drop"), (nb, 2 * h, 2 * w, C), P_DROP, kw)
        return Built(op, [lo], [], kw, lambda c, m: up2_epilogue(c(lo), c(ca), c(cc), div, act, c(keep), P_DROP, m), form="up2x_epilogue_kernel",
                     gen=gen, p=P_DROP, keep=keep)
    raise ValueError(op)


# which (case, mutant) pairs the bound must tell from the reference, per op: at least one case per kernel form for every mutant that
# applies to the op.  INVISIBLE: pairs the bound cannot see at that shape -- listed so that the test says so instead of asserting.
MUTANTS = {
    "gn_act": [(c, m) for c in ("fallback-C32-hw35", "walk-C64-hw33", "walk-C64-hw129", "atomic-C192-hw37", "apply-C64-hw129-nowalk") for m in ("last_pixel", "unbiased")]
    + [(c, "no_eps") for c in ("fallback-C32-hw35-tiny", "walk-C64-hw129-tiny", "atomic-C192-hw37-tiny", "part-C64-hw33-slots3-tiny", "finpart-C64-hw130-slots65-tiny")]
    + [(c, "slot_dropped") for c in ("part-C64-hw33-slots3", "finpart-C64-hw130-slots65", "finpart-C64-hw260-slots130", "finpart-C512-hw17-slots9")]
    + [(c, m) for c in ("walk-C64-hw129-all-mask", "walk-C64-hw129-all-gen", "part-C64-hw33-slots3-all-mask", "fallback-C32-hw35-all-gen", "atomic-C192-hw37-all-mask")
       for m in ("film_shift", "residual_before_drop")],
    "layernorm_c": [(c, m) for c in ("vec-C8-hw33", "vec-C64-hw33", "fallback-C24-hw33") for m in ("unbiased", "tail_pixel")]
    + [("vec-C64-hw33-tiny", "no_eps"), ("fallback-C24-hw33-tiny", "no_eps")],
    "head": [(c, "no_bias") for c in ("vec-C64-co3-hw225", "pixel16B-C24-co2", "generic-C20-co3")] + [(c, "last_chunk") for c in ("vec-C64-co3-hw225", "pixel16B-C24-co2", "generic-C64-co5")],
    "stem_conv": [(c, "tap_dropped") for c in ("valu-d32-k7-c2-5x7", "valu-d64-k6-c2-5x7", "mfma-d64-k3-c5-5x7", "mfma-d64-k5-c3-5x7", "mfma-d64-k7-c8-5x7")],
    "groupnorm_f32": [(c, m) for c in ("wave4-C64-hw16", "block-C24-g4-hw16") for m in ("last_pixel", "unbiased")] + [("wave8-C64-hw129", "last_pixel")]
    + [(c, "no_eps") for c in ("wave4-C64-hw16-tiny", "wave8-C64-hw129-tiny", "block-C64-hw257-tiny")]
    + [(c, "film_shift") for c in ("wave4-C64-hw16-film-relu", "wave8-C64-hw129-film-leaky-maskdrop", "block-C64-hw257-film-relu-maskdrop")],
    "up2_bilinear": [(c, "border_mirrored") for c in ("quad-64+0-2x2", "quad-64+64-3x5", "vec-64+64-1x4", "vec-64+64-3x5-noquad", "scalar-12+4-3x5")]
    + [(c, "second_source_shift8") for c in ("quad-64+64-2x2", "quad-64+64-3x5", "vec-64+64-1x4", "vec-64+64-3x5-noquad")],
    "up2_epilogue": [(c, m) for c in ("C4-1x3", "C64-3x5", "C64-3x5-coefdiv2-nb4") for m in ("border_mirrored", "film_shift")],
}
INVISIBLE = {
    "gn_act": [("walk-C64-hw8281-nb1", "last_pixel"), ("walk-C64-hw8281-nb1", "unbiased"), ("walk-C64-hw129", "no_eps")],
    # (<8> starts at 129 pixels of 8 channels: 1 / (2 * 1032) of rstd is under the bf16 floor at every shape that form takes)
    "groupnorm_f32": [("wave8-C64-hw129", "unbiased"), ("block-C64-hw257", "unbiased"), ("wave4-C64-hw16", "no_eps")],
    "layernorm_c": [("vec-C64-hw33", "no_eps")],
    "up2_epilogue": [("C64-1x1", "border_mirrored")],
}
