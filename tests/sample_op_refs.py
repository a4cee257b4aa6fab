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
        # seed: dyf_seed(SEED) first (generator ops without a dropout); repeat: the op runs that often in a row and every call's outputs
        # are compared; rows: the batch rows the launcher notes its form for
        self.seed, self.repeat, self.rows = gen is not None, 1, xs[0].shape[0] if xs else 0

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


# =================================================================================== the launchers around the networks (csrc/kernels.hip)
# readout, readout tables, the two stems, time MLP and FiLM heads, the sampler's elementwise kernels and the generator's bookkeeping, through
# the same seam.  An op here may return several tensors: Built.kind is then a tuple, one kind per output ("eq": integers, equal).
NET_OPS = ("readout", "stem", "stem16", "time_mlp", "film", "cold_update", "noisy_condition", "rng_begin", "rng_clone")
READOUT_MUTANTS = ("border_mirrored", "border_clamped", "parity_swapped", "not_flipped", "no_bias")
TAU = 0.3


def outputs(v):
    return list(v) if isinstance(v, (tuple, list)) else [v]


def nearest_floor_is_exact(n_in, n_out):
    """bilinear_coord's nearest mode floors (float)dst * ((float)n_in / (float)n_out) in fp32: does that equal floor(dst n_in / n_out) for every dst?"""
    dst = np.arange(n_out)
    f32 = np.floor(dst.astype(np.float32) * (np.float32(n_in) / np.float32(n_out))).astype(np.int64)
    return bool(np.array_equal(np.minimum(f32, n_in - 1), (dst * n_in) // n_out))


def readout_taps(n_in, n_out, nearest, dtype=torch.float64):
    """The readout's stencil along one axis, from the resample matrix alone: output o reads neighbours u of the transposed conv's 2 n_in
    grid with weights M[o, u]; u gathers input i through kernel tap k = u + 1 - 2 i in 0..3, i.e. i = (u + 1) >> 1 (k = 0 or 1) and
    i - 1 (k = 2 or 3).  -> (idx (n_out, 4) long: the input index of tap k, possibly -1 or n_in = outside; wgt (n_out, 4))."""
    M = T._resample_matrix(2 * n_in, n_out, nearest, dtype)
    idx, wgt = torch.full((n_out, 4), -1, dtype=torch.long), torch.zeros(n_out, 4, dtype=dtype)
    for o in range(n_out):
        for u in M[o].nonzero().flatten().tolist():
            for i in ((u + 1) >> 1, ((u + 1) >> 1) - 1):
                k = u + 1 - 2 * i
                idx[o, k], wgt[o, k] = i, wgt[o, k] + M[o, u]
    return idx, wgt


def _tap_gather(idx, wgt, n, mutant):
    """-> (index inside the image, effective weight): a tap outside the image contributes nothing -- or, for the mutants, is mirrored / clamped in."""
    out = (idx < 0) | (idx >= n)
    if mutant == "border_mirrored":
        g = torch.where(idx < 0, -idx, torch.where(idx >= n, 2 * n - 2 - idx, idx)).clamp(0, n - 1)
        return g, wgt
    if mutant == "border_clamped":
        return idx.clamp(0, n - 1), wgt
    return idx.clamp(0, n - 1), wgt * (~out).to(wgt.dtype)


def readout_stencil(x, w, b, oh, ow, nearest, mutant=None):
    """The readout as the kernels evaluate it: 16 (kh, kw) taps per native pixel, each one 64-channel contraction times its bilinear weight."""
    nb, ih, iw, _ = x.shape
    (iy, wy), (ix, wx) = readout_taps(ih, oh, nearest, x.dtype), readout_taps(iw, ow, nearest, x.dtype)
    (gy, wy), (gx, wx) = _tap_gather(iy, wy, ih, mutant), _tap_gather(ix, wx, iw, mutant)
    if mutant == "parity_swapped":
        w = w[:, :, [1, 0, 3, 2]][:, :, :, [1, 0, 3, 2]]
    if mutant == "not_flipped":
        w = w.flip(2, 3)
    xg = x[:, gy][:, :, :, gx]  # (nb, oh, kh, ow, kw, cin)
    y = torch.einsum("nyhxwc,cohw,yh,xw->noyx", xg, w, wy, wx)
    return y if mutant == "no_bias" else y + b[None, :, None, None]


def readout(x, w, b, oh, ow, nearest, mutant=None):
    """ConvTranspose2d(k4, s2, p1) and the final resample: x NHWC (nb, ih, iw, cin), w (cin, cout, 4, 4) -> NCHW (nb, cout, oh, ow)."""
    if mutant is not None:  # ("stencil": the stencil statement itself, nothing edited)
        return readout_stencil(x, w, b, oh, ow, nearest, None if mutant == "stencil" else mutant)
    y = torch.nn.functional.conv_transpose2d(x.permute(0, 3, 1, 2), w, b, stride=2, padding=1)
    return T.resize(y.permute(0, 2, 3, 1), oh, ow, nearest).permute(0, 3, 1, 2)


def readout_columns(iw, ow, nearest):
    """The input columns the reference stencil reads with a non-zero weight -> (sorted stored columns, col_map (iw,) int16: -1 = not stored)."""
    idx, wgt = readout_taps(iw, ow, nearest)
    used = sorted({int(i) for i, g in zip(idx.flatten().tolist(), wgt.flatten().tolist()) if g != 0 and 0 <= i < iw})
    cmap = torch.full((iw,), -1, dtype=torch.int16)
    cmap[used] = torch.arange(len(used), dtype=torch.int16)
    return used, cmap


def stem(srcs, w, b, uh, uw, nearest=False, src_rows=0, nb=None, keep=None, p=0.0, mutant=None):
    """cat of NCHW sources (row r of the output reads source row r % src_rows) -> resample to (uh, uw) -> 1x1 conv -> Dropout: NHWC.
    w = None: the resample alone (the fused stem)."""
    if mutant == "second_source_offset" and len(srcs) > 1:  # the second source's channels start one channel late
        srcs = [srcs[0], srcs[1].roll(1, 1)] + list(srcs[2:])
    x = torch.cat(srcs, 1)
    nb = x.shape[0] if nb is None else nb
    rows = torch.arange(nb) % (src_rows if src_rows > 0 else nb)
    if mutant == "src_rows_ignored":  # row r read as row r: past the rows the sources hold
        x = torch.cat([x, torch.zeros(nb - x.shape[0], *x.shape[1:], dtype=x.dtype)])
        rows = torch.arange(nb)
    y = T.resize(x[rows].permute(0, 2, 3, 1), uh, uw, nearest)
    if w is None:
        return y
    y = y @ w.T
    return _drop(y if mutant == "no_bias" else y + b, keep, p)


def stem16(srcs, uh, uw, nearest=False, src_rows=0, nb=None, mutant=None):
    """The fused stem's tensor: (nb, uh + 2, uw + 2, 16), zero border, channels = the resampled sources, then 1 (slot cin), then zeros."""
    y = stem(srcs, None, None, uh, uw, nearest, src_rows, nb, mutant=mutant)
    cin = y.shape[-1]
    out = torch.zeros(y.shape[0], uh + 2, uw + 2, 16, dtype=y.dtype)
    out[:, 1:-1, 1:-1, :cin] = y
    if mutant != "no_bias_slot":
        out[:, 1:-1, 1:-1, cin] = 1
    return out


def time_mlp(t, w1, b1, w2, b2, learned=None, mutant=None):
    """oracle/nets.py time_embedding, and the SiLU every block's time_mlp starts with: (rows,) -> (rows, 2 dim)."""
    tt = t[:, None]
    sc = (lambda a: torch.cat([a.cos(), a.sin()], -1)) if mutant == "sincos_swapped" else (lambda a: torch.cat([a.sin(), a.cos()], -1))
    if learned is not None:
        e = torch.cat([tt, sc(tt * learned[None, :] * 2 * math.pi)], -1)
    else:
        half = w1.shape[1] // 2
        freqs = torch.exp(torch.arange(half, dtype=t.dtype) * (-math.log(10000.0) / (half if mutant == "half_for_half_minus_1" else half - 1)))
        e = sc(tt * freqs[None, :])
    h = torch.nn.functional.gelu(e @ w1.T + b1, approximate="tanh" if mutant == "tanh_gelu" else "none")
    return torch.nn.functional.silu(h @ w2.T + b2)


def film(silu, wf, bf, norm_a, norm_c, blocks, rows, mutant=None):
    """oracle/nets.py film per block (Linear -> chunk(scale, shift)), folded with the block's norm: a = norm_a (1 + scale),
    c = norm_c (1 + scale) + shift; wf holds, per block, its scale rows then its shift rows.  silu None: scale = shift = 0."""
    A, Cc, off = [], [], 0
    for co in blocks:
        r0 = off if mutant == "blk_off_single" else 2 * off
        if silu is None:
            scale = shift = torch.zeros(rows, co, dtype=norm_a.dtype)
        else:
            ss = silu @ wf[r0:r0 + 2 * co].T + bf[r0:r0 + 2 * co]
            scale, shift = (ss[:, co:], ss[:, :co]) if mutant == "rows_swapped" else (ss[:, :co], ss[:, co:])
        A.append(norm_a[off:off + co] * (1 + scale))
        Cc.append(norm_c[off:off + co] * (1 + scale) + shift)
        off += co
    return torch.cat(A, 1), torch.cat(Cc, 1)


def gen_noise(shape, call, dtype=torch.float64):
    """The field the engine's generator draws at noise call `call` (dyf_seed(SEED), rows ROW_OFFSET ..), rebuilt on the host."""
    n = int(np.prod(shape[1:]))
    npdt = np.float64 if dtype == torch.float64 else np.float32
    return torch.from_numpy(np.stack([rng_host.noise_field(SEED, call, ROW_OFFSET + r, n, npdt) for r in range(shape[0])])).reshape(shape)


def begin_keys(fwd0, row0, rows, per):
    """(row-key table (rows, 2), generator state afterwards) of a forward start over `rows` launch rows, `per` rows per forward."""
    keys = np.array([[int(k) for k in rng_host.row_key(SEED, fwd0 + r // per, row0 + r % per)] for r in range(rows)], dtype=np.uint32)
    state = np.array([SEED & 0xFFFFFFFF, SEED >> 32, fwd0 + -(-rows // per), row0, 0, 0, 0, 0], dtype=np.uint32)
    return torch.from_numpy(keys.view(np.int32)), torch.from_numpy(state.view(np.int32))


RO_GEOM = {"ident": ((2, 3), (4, 6)), "down": ((6, 8), (5, 7)), "up": ((2, 2), (9, 11)), "one": ((1, 1), (3, 3))}
RO_FORMS = {  # switches / tables -> the form launch_readout notes ({co}: the output channels)
    "dma": ({}, True, "readout_dma_kernel"), "nodma": ({"DYF_READOUT_DMA": "0"}, True, "readout_mfma_kernel"), "notab": ({}, False, "readout_mfma_kernel"),
    "regw": ({"DYF_READOUT_MFMA": "0"}, True, "readout_regw_kernel<{co}>"),
    "sliced": ({"DYF_READOUT_MFMA": "0", "DYF_READOUT_REGW": "0"}, True, "readout_sliced_kernel<8>")}
RO_QUIET = ("readout_dma_kernel", "readout_mfma_kernel", "readout_kernel") + tuple(f"readout_regw_kernel<{c}>" for c in (1, 2, 3, 4)) + \
    tuple(f"readout_sliced_kernel<{c}>" for c in (1, 2, 4, 8, 16))
STEM_QUIET = ("stem_kernel", "stem16_kernel", "stem16_rows_kernel")


def net_specs(op):
    S = []
    if op == "readout":
        def ro(cid, geom, form, co, cin=64, nb=3, **kw):
            (ih, iw), (oh, ow) = geom
            sw, tab, name = RO_FORMS[form] if form in RO_FORMS else ({}, True, form)
            S.append((cid, dict(cin=cin, co=co, nb=nb, ih=ih, iw=iw, oh=oh, ow=ow, switch=sw, tables=tab, form=name.format(co=co), **kw)))
        # every form on every geometry, bilinear and nearest; nb = 3: 72 / 105 / 297 / 27 pixels, the ragged last 16-pixel group spans
        # samples (27: an odd count, and half-waves 4..7 of the register-weight form start past the end)
        for gi, (g, geom) in enumerate(RO_GEOM.items()):
            for fi, form in enumerate(RO_FORMS):
                for near in (0, 1):
                    ro(f"{form}-{g}{'-nearest' if near else ''}", geom, form, 1 + (gi + fi + near) % 4, nearest=near)
        for form in RO_FORMS:  # 73 728 pixels: 4608 groups on 4096 waves, groups_per_wave = 2
            ro(f"{form}-big", ((8, 8), (192, 192)), form, 3, nb=2)
        for co in (1, 2, 3, 4):
            ro(f"regw-down-co{co}", RO_GEOM["down"], "regw", co)
        for cin, co in ((8, 8), (16, 5), (32, 8), (128, 3)):
            ro(f"sliced-cin{cin}-co{co}", RO_GEOM["down"], f"readout_sliced_kernel<{cin // 8}>", co, cin=cin)
            ro(f"sliced-cin{cin}-co{co}-up-nearest", RO_GEOM["up"], f"readout_sliced_kernel<{cin // 8}>", co, cin=cin, nearest=1)
        for cin, co in ((12, 3), (24, 8)):
            ro(f"generic-cin{cin}-co{co}", RO_GEOM["down"], "readout_kernel", co, cin=cin)
            ro(f"generic-cin{cin}-co{co}-up", RO_GEOM["up"], "readout_kernel", co, cin=cin)
        for form in ("dma", "notab", "nodma"):  # compact columns: 3 native columns read 8 of 16 decoder columns
            ro(f"{form}-compact", ((6, 16), (5, 3)), form, 3, compact=1)
        ro("dma-compact-nearest", ((6, 16), (5, 3)), "dma", 2, compact=1, nearest=1)
        ro("regw-switch-compact", ((6, 16), (5, 3)), "regw", 3, compact=1, form_override="readout_dma_kernel")  # a compact input stays on the MFMA forms
    elif op == "stem16":
        def s16(cid, ch, hw, uhw, form, nb=2, **kw):
            S.append((cid, dict(ch=ch, h=hw[0], w=hw[1], uh=uhw[0], uw=uhw[1], nb=nb, form=form, **kw)))
        R, K = "stem16_rows_kernel", "stem16_kernel"
        s16("rows-2lane-uw254-c8", (8,), (5, 40), (8, 254), R)                  # the smallest width the rows form takes
        for uh in (7, 8, 9):                                                      # a border-only last block, rows 8-9, rows 8-10
            s16(f"rows-1lane-uw256-c3-uh{uh}", (3,), (5, 40), (uh, 256), R)
            s16(f"rows-2lane-uw256-c9-uh{uh}", (5, 4), (5, 40), (uh, 256), R)
        s16("rows-1lane-uw256-c8", (8,), (5, 40), (8, 256), R)                    # the bias slot in the second half
        s16("rows-2lane-uw256-c15", (15,), (5, 40), (8, 256), R)
        s16("rows-1lane-uw256-c8-2src", (5, 3), (5, 40), (8, 256), R)
        s16("rows-1lane-uw256-c8-3src", (3, 3, 2), (5, 40), (8, 256), R)
        s16("rows-1lane-uw256-c8-4src", (3, 2, 2, 1), (5, 40), (8, 256), R)
        s16("rows-2lane-uw256-c9-4src", (3, 3, 2, 1), (5, 40), (8, 256), R)
        s16("rows-1lane-uw256-c3-nearest", (3,), (5, 40), (8, 256), R, nearest=1)
        s16("rows-2lane-uw256-c9-nearest", (5, 4), (5, 40), (7, 256), R, nearest=1)
        s16("rows-1lane-uw256-c8-srcrows1", (8,), (5, 40), (8, 256), R, src_rows=1)
        s16("rows-2lane-uw254-c8-srcrows1", (5, 3), (5, 40), (9, 254), R, src_rows=1)
        s16("rows-1lane-uw256-c8-fold", (8,), (5, 40), (8, 256), R, nb=4, src_rows=2, fold=1)
        s16("plain-lds-c15-w80", (15,), (5, 80), (8, 256), K)                     # 10 x 80 x 16 floats of rows: past 48 KB
        s16("plain-h12-uh8", (3,), (12, 40), (8, 256), K)                         # downsampled rows: more than ST_ROWS + 2 source rows
        s16("plain-norows-c8", (8,), (5, 40), (8, 256), K, switch={"DYF_STEM16_ROWS": "0"})
        s16("plain-ident-5x7-c3", (3,), (5, 7), (5, 7), K, nb=3)
        s16("plain-up-3x5-c9-4src", (3, 3, 2, 1), (3, 5), (7, 9), K, nb=3)
        s16("plain-down-9x11-c15", (15,), (9, 11), (4, 6), K, nb=3)
        s16("plain-up-3x5-c5-nearest", (4, 1), (3, 5), (6, 15), K, nb=3, nearest=1)
        s16("plain-up-3x5-c8-srcrows1", (8,), (3, 5), (7, 9), K, src_rows=1)
        s16("plain-up-3x5-c3-fold", (3,), (3, 5), (7, 9), K, nb=3, fold=1)
    elif op == "stem":
        def st(cid, dim, ch, hw, uhw, nb=3, **kw):
            S.append((cid, dict(dim=dim, ch=ch, h=hw[0], w=hw[1], uh=uhw[0], uw=uhw[1], nb=nb, **kw)))
        for dim in (8, 12, 64):                                                   # 297 pixels: the second workgroup ends mid-way; 12: scalar stores
            st(f"d{dim}-up-3x5-c5", dim, (3, 2), (3, 5), (9, 11))
        st("d64-ident-5x7-c3", 64, (3,), (5, 7), (5, 7))
        st("d12-down-9x11-c9-4src", 12, (3, 3, 2, 1), (9, 11), (4, 6))
        st("d64-up-3x5-c6-3src-nearest", 64, (3, 2, 1), (3, 5), (6, 15), nearest=1)
        st("d8-up-3x5-c32", 8, (32,), (3, 5), (9, 11))
        st("d64-up-3x5-c5-maskdrop", 64, (3, 2), (3, 5), (9, 11), drop="mask")
        st("d12-up-3x5-c5-gendrop", 12, (3, 2), (3, 5), (9, 11), drop="gen")
        st("d64-up-3x5-c5-gendrop", 64, (3, 2), (3, 5), (9, 11), drop="gen")
        st("d64-up-3x5-c5-srcrows2-nb5", 64, (3, 2), (3, 5), (9, 11), nb=5, src_rows=2)
        st("d12-ident-5x7-c5-srcrows1-nb3", 12, (3, 2), (5, 7), (5, 7), src_rows=1)
    elif op == "time_mlp":
        S = [("sinu-d32", dict(dim=32)), ("sinu-d64", dict(dim=64)), ("learned8-d32", dict(dim=32, lh=8)), ("learned5-d64", dict(dim=64, lh=5))]
    elif op == "film":
        S = [(f"b8+24+64-rows{r}{'-notime' if nt else ''}", dict(blocks=(8, 24, 64), rows=r, notime=nt)) for r in (1, 3) for nt in (0, 1)]
        S.append(("b64-rows3", dict(blocks=(64,), rows=3, notime=0)))
    elif op == "cold_update":
        S = [("3x3x9x11", dict(copy=0)), ("3x3x9x11-copy", dict(copy=1))]         # 891 floats: the fourth workgroup ends mid-way
    elif op == "noisy_condition":
        S = [("3x3x9x11-injected", dict(gen=0)), ("3x3x9x11-generator-2calls", dict(gen=1))]  # rows of 297 floats, global rows 5..7
    elif op == "rng_begin":
        S = [("rows5-per2", dict(rows=5, per=2)), ("rows3", dict(rows=3, per=0)), ("rows8-per4", dict(rows=8, per=4))]
    elif op == "rng_clone":
        S = [("full-rowadd7", dict(counters=0)), ("counters-only", dict(counters=1))]
    return S


def net_build(op, a, dtname):
    dt = DTYPES[dtname]
    r16 = lambda t: round16(t, dt)
    if op == "readout":
        cin, co, nb, ih, iw, oh, ow, near = a["cin"], a["co"], a["nb"], a["ih"], a["iw"], a["oh"], a["ow"], bool(a.get("nearest"))
        g = _gen(20, cin, co, nb, ih, iw, oh, ow)
        # 16-bit activations and 16-bit weights: the fp32-weight forms and the MFMA forms then see the same numbers
        x = r16(_rn(g, nb, ih, iw, cin, scale=1.5))
        w, b = r16(_rn(g, cin, co, 4, 4, scale=1.5 / math.sqrt(4 * cin))).float(), _rn(g, co, scale=0.5).float()
        kw = dict(out_hw=(oh, ow), nearest=near, tables=a["tables"])
        xs, fn = [x], (lambda c, m: readout(c(x), c(w), c(b), oh, ow, near, m))
        if a.get("compact"):
            used, cmap = readout_columns(iw, ow, near)
            kw["col_map"] = cmap
            xs = [x[:, :, used].contiguous()]
            xw = x[:, :, [min(j, len(used) - 1) for j in range(iw)]]  # col_map ignored: decoder column j read at stored column j
            fn = lambda c, m: readout(c(xw if m == "col_map_ignored" else x), c(w), c(b), oh, ow, near, None if m == "col_map_ignored" else m)
        big = nb * oh * ow > 4096
        b_ = Built(op, xs, [w, b], kw, fn, kind="f32", form=a.get("form_override", a["form"]), quiet=RO_QUIET, switch=a["switch"])
        b_.stencil = not big  # (the 16-tap gather of the big case would hold 75 M doubles)
        return b_
    if op in ("stem", "stem16"):
        ch, h, w, uh, uw, nb, near, sr = a["ch"], a["h"], a["w"], a["uh"], a["uw"], a["nb"], bool(a.get("nearest")), a.get("src_rows", 0)
        g = _gen(21 if op == "stem" else 22, sum(ch), len(ch), h, w, uh, uw, nb, sr, a.get("dim", 0))
        srcs = [_rn(g, sr if sr else nb, c, h, w, scale=1.5).float() for c in ch]
        kw = dict(out_hw=(uh, uw), nearest=near, src_rows=sr, nb=nb)
        if op == "stem":
            dim = a["dim"]
            wt, b = _rn(g, dim, sum(ch), scale=1.5 / math.sqrt(sum(ch))).float(), _rn(g, dim, scale=0.5).float()
            keep, gen = _drop_kw(g, a.get("drop"), (nb, uh, uw, dim), P_DROP, kw)
            fn = lambda c, m: stem([c(s) for s in srcs], c(wt), c(b), uh, uw, near, sr, nb, c(keep), P_DROP, m)
            out = Built(op, srcs, [wt, b], kw, fn, form="stem_kernel", quiet=STEM_QUIET, gen=gen, p=P_DROP, keep=keep)
        else:
            fn = lambda c, m: stem16([c(s) for s in srcs], uh, uw, near, sr, nb, m)
            kind = "r16"
            if a.get("fold"):
                kw.update(fold_rng=True, rng_row_offset=ROW_OFFSET, rng_forward=FORWARD)
                keys, state = begin_keys(FORWARD, ROW_OFFSET, nb, sr if sr else nb)
                fn, kind = (lambda c, m: (stem16([c(s) for s in srcs], uh, uw, near, sr, nb, m), keys, state)), ("r16", "eq", "eq")
            out = Built(op, srcs, [], kw, fn, kind=kind, form=a["form"], quiet=STEM_QUIET, switch=a.get("switch"))
            out.seed, out.cin = bool(a.get("fold")), sum(ch)
        out.rows = nb
        return out
    if op == "time_mlp":
        dim, lh = a["dim"], a.get("lh", 0)
        g = _gen(23, dim, lh)
        # the sampler's times: 0, fractions of a step, whole steps up to the horizon of 64
        t = torch.tensor([0.0, 0.25, 1.0 / 3.0, 0.999, 1.0, 7.5, 33.0, 63.9, 64.0], dtype=torch.float64).float()
        nfeat = 2 * lh + 1 if lh else dim
        ps = [_rn(g, 2 * dim, nfeat, scale=1.0 / math.sqrt(nfeat)).float(), _rn(g, 2 * dim, scale=0.3).float(),
              _rn(g, 2 * dim, 2 * dim, scale=1.0 / math.sqrt(2 * dim)).float(), _rn(g, 2 * dim, scale=0.3).float()]
        if lh:
            ps.append(_rn(g, lh, scale=LEARNED_SCALE).float())
        return Built(op, [t], ps, {}, lambda c, m: time_mlp(c(t), *[c(q) for q in ps[:4]], learned=c(ps[4]) if lh else None, mutant=m), kind="f32")
    if op == "film":
        blocks, rows, tdim = a["blocks"], a["rows"], 64
        total = sum(blocks)
        g = _gen(24, total, rows, a["notime"])
        silu = None if a["notime"] else _rn(g, rows, tdim, scale=0.7).float()
        ps = [_rn(g, 2 * total, tdim, scale=1.0 / math.sqrt(tdim)).float(), _rn(g, 2 * total, scale=0.3).float(),
              (1.0 + _rn(g, total, scale=0.3)).float(), _rn(g, total, scale=0.5).float()]
        out = Built(op, [] if silu is None else [silu], ps, dict(blocks=blocks, nb=rows), lambda c, m: film(c(silu), *[c(q) for q in ps], blocks, rows, m),
                    kind=("f32", "f32"))
        out.rows = rows
        return out
    if op == "cold_update":
        g = _gen(25, a["copy"])
        xs = [_rn(g, 3, 3, 9, 11, scale=1.5).float() for _ in range(3)]
        fn = lambda c, m: (c(xs[0]) - c(xs[1]) + c(xs[2]),) * (2 if a["copy"] else 1)
        return Built(op, xs, [], dict(copy=bool(a["copy"])), fn, kind=("f32", "f32") if a["copy"] else ("f32",))
    if op == "noisy_condition":
        g = _gen(26, a["gen"])
        cond, tau = _rn(g, 3, 3, 9, 11, scale=1.5).float(), float(np.float32(TAU))
        mix = lambda c, z: tau * c(cond) + (1.0 - tau) * z
        if not a["gen"]:
            noise = _rn(g, 3, 3, 9, 11).float()
            return Built(op, [cond, noise], [], dict(tau=tau), lambda c, m: mix(c, c(noise)), kind="f32")
        # two calls in a row: the second draws the NEXT field of the stream
        fn = lambda c, m: tuple(mix(c, gen_noise(cond.shape, 0 if m == "same_field_twice" else call, c(cond).dtype)) for call in (0, 1))
        out = Built(op, [cond], [], dict(tau=tau, rng_row_offset=ROW_OFFSET), fn, kind=("f32", "f32"))
        out.seed, out.repeat = True, 2
        return out
    if op == "rng_begin":
        rows, per = a["rows"], a["per"]
        out = Built(op, [], [], dict(nb=rows, src_rows=per, rng_row_offset=ROW_OFFSET, rng_forward=FORWARD),
                    lambda c, m: begin_keys(FORWARD, ROW_OFFSET, rows, per if per else rows), kind=("eq", "eq"))
        out.seed, out.rows = True, rows
        return out
    if op == "rng_clone":
        src, dst = torch.arange(1, 9, dtype=torch.int32) * 1000003, torch.arange(11, 19, dtype=torch.int32)
        want = dst.clone()
        if a["counters"]:
            want[2], want[4] = src[2], src[4]
        else:
            want = src.clone()
            want[3] += 7
        return Built(op, [src], [], dict(dst=dst, rng_row_offset=7, counters_only=bool(a["counters"])), lambda c, m: want, kind="eq")
    raise ValueError(op)


LEARNED_SCALE = 0.05  # learned frequencies: 2 pi t w stays below ~60 rad at t = 64, where an fp32 angle still resolves 4e-6 rad

NET_MUTANTS = {
    "readout": [(c, m) for c in ("dma-down", "nodma-down", "notab-down", "regw-down", "sliced-down", "dma-up-nearest", "sliced-cin32-co8", "generic-cin12-co3",
                                 "dma-compact") for m in READOUT_MUTANTS]
    + [(c, m) for c in ("dma-ident", "regw-up", "dma-one") for m in ("parity_swapped", "not_flipped", "no_bias", "border_clamped")]
    + [(c, "col_map_ignored") for c in ("dma-compact", "notab-compact", "nodma-compact", "dma-compact-nearest")],
    "stem": [(c, m) for c in ("d8-up-3x5-c5", "d12-up-3x5-c5", "d64-up-3x5-c5", "d12-down-9x11-c9-4src") for m in ("second_source_offset", "no_bias")]
    + [(c, "src_rows_ignored") for c in ("d64-up-3x5-c5-srcrows2-nb5", "d12-ident-5x7-c5-srcrows1-nb3")],
    "stem16": [(c, m) for c in ("rows-2lane-uw256-c9-uh8", "rows-1lane-uw256-c8-2src", "rows-2lane-uw256-c9-4src", "plain-up-3x5-c9-4src")
               for m in ("second_source_offset", "no_bias_slot")]
    + [(c, "no_bias_slot") for c in ("rows-1lane-uw256-c3-uh8", "rows-1lane-uw256-c8", "rows-2lane-uw256-c15", "plain-ident-5x7-c3")]
    + [(c, "src_rows_ignored") for c in ("rows-1lane-uw256-c8-srcrows1", "rows-2lane-uw254-c8-srcrows1", "plain-up-3x5-c8-srcrows1")],
    "time_mlp": [(c, m) for c in ("sinu-d32", "sinu-d64") for m in ("tanh_gelu", "sincos_swapped", "half_for_half_minus_1")]
    + [(c, m) for c in ("learned8-d32", "learned5-d64") for m in ("tanh_gelu", "sincos_swapped")],
    "film": [(c, m) for c in ("b8+24+64-rows1", "b8+24+64-rows3") for m in ("rows_swapped", "blk_off_single")] + [("b64-rows3", "rows_swapped")],
    "noisy_condition": [("3x3x9x11-generator-2calls", "same_field_twice")],
}
NET_INVISIBLE = {
    "readout": [("dma-one", "border_mirrored"), ("dma-ident", "border_mirrored")],  # (one input row: its mirror is the clamp; identity: see the test)
    "film": [("b64-rows3", "blk_off_single")],                                      # the first block's offset is 0
}
MUTANTS.update(NET_MUTANTS)
INVISIBLE.update(NET_INVISIBLE)
_specs_between, _build_between = specs, build


def specs(op):  # noqa: F811 -- both halves behind the one name the tests use
    return net_specs(op) if op in NET_OPS else _specs_between(op)


def build(op, a, dtname):  # noqa: F811
    return net_build(op, a, dtname) if op in NET_OPS else _build_between(op, a, dtname)


OPS = OPS + NET_OPS
