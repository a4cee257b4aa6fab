"""The plain reference of a 3x3 conv with the GroupNorm fused into its epilogue (dyffusion_amd/csrc/gn_fused.h; the second ladder of
csrc/conv_dispatch.hip, choose_gn_fused), the cases tests/test_gpu_conv_gn_fused.py runs through HipEngine.op_conv_gn (dyf_op_conv_gn),
and mutants -- test infrastructure, no GPU.  The bound, the rounding and the GroupNorm statement are tests/sample_op_refs.py's.

The chain, a pure torch function in the dtype of its arguments:
    conv3x3(cat(sources)) + bias -> GroupNorm (biased variance, eps 1e-5) -> FiLM row sample // coef_div -> SiLU -> keep / (1 - p)
    -> + residual
Inputs are drawn in float64 and rounded to the build's 16-bit type first; the weights are rounded to that type as well (the weight
upload stores them in it).  The conv output has about unit variance; the bias carries an offset of about 4 of those standard deviations
per group and a spread per channel inside the group: the kernels finalise E[y^2] - mean^2 from fp32 partial sums and must survive the
cancellation, and a statistics mistake (a pixel count, a slot, a slab credited to the wrong sample) moves the output by far more than a
16-bit ulp.

The mutants are mistakes one of the four kernels could make.  The ones about statistics are stated on what the kernels exchange: partial
(sum, sum of squares) per slot and 8-channel octet, with the slot geometry of each form (slot_geometry) -- sample_op_refs.group_norm
takes such partials in place of a statistics pass.
"""
import math

import torch
import torch.nn.functional as F

from tests import sample_op_refs as S

DTYPES = S.DTYPES
P_DROP = S.P_DROP

GN16 = "conv_gn16_kernel+gn_fused"
HALO5 = "conv_up_halo_kernel<5>+gn_fused"
BM128 = "conv_igemm2_kernel<2,bm128>+gn_fused"
BM256 = "conv_igemm2_kernel<2>+gn_fused"
SH3 = "conv_igemm2_kernel+sh3"
# form -> (the form-log notes of a launch, the DYF_* switches that bring a small problem to the form)
_IG = {"DYF_GN16": 0, "DYF_HALO5": 0, "DYF_IGEMM2_MIN_TILES": 1}
FORMS = {
    "gn16": ({GN16}, {"DYF_GN16_MIN_TILES": 1, "DYF_GN16_ANY_PLANE": 1}),
    "halo5": ({HALO5}, {"DYF_GN16": 0, "DYF_HALO5_MIN_TILES": 1}),
    "bm128": ({BM128, BM256}, _IG),  # (launch_conv_igemm2 notes the kernel, then the 128-pixel tile form)
    "bm256": ({BM256}, dict(_IG, DYF_IGEMM2_BM128_BELOW=0)),
    # what the halo5 switches leave to the implicit-GEMM form (cover rule, unequal sources): its own tile threshold lowered as well
    "halo5>bm128": ({BM128, BM256}, {"DYF_GN16": 0, "DYF_HALO5_MIN_TILES": 1, "DYF_IGEMM2_MIN_TILES": 1}),
    "prod>bm128": ({BM128, BM256}, {}),  # the production thresholds
}


def kernel_of(form):
    return form.split(">")[-1]


# ------------------------------------------------------------------------------------------------------------- slot geometry
def slot_geometry(form, h, w):
    """How a form cuts a sample's pixels into statistics slots: ("tile", th, tw, sy, sx) = th x tw tiles in raster order, each cut
    into sy x sx slots (conv_gn16: one slot per 16 x 16 tile; conv_up_halo<5>: 16 x 32 tiles, one slot per wave = 8 x 16 quadrant;
    conv_igemm2 on 2-D tiles: two half-tile slabs) or ("slab", R) = R-row slabs of the FLATTENED (n * plane) pixel axis."""
    k = kernel_of(form)
    if k == "gn16":
        return ("tile", 16, 16, 1, 1)
    if k == "halo5":
        return ("tile", 16, 32, 2, 2)
    th = 16 if k == "bm256" else 8
    if w % 16 == 0 and h % th == 0:
        return ("tile", th, 16, 2, 1)
    return ("slab", 8 * th)


def slots_of(form, h, w):
    """Slots per sample (conv_gn16_slots, conv_halo5_gn_slots, conv_igemm2_gn_slots[_bm128]); 0 = the form does not serve the plane."""
    g = slot_geometry(form, h, w)
    if g[0] == "tile":
        return -(-h // g[1]) * -(-w // g[2]) * g[3] * g[4]
    return 0 if h * w < g[1] else -(-(h * w) // g[1]) + 1


def _slot_owner(geom, n, h, w, straddle_first=False):
    """-> (owner sample, slot inside the owner's slots) per (sample, pixel), and the slot count."""
    plane = h * w
    if geom[0] == "tile":
        _, th, tw, sy, sx = geom
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        tile = (ys // th) * -(-w // tw) + xs // tw
        sub = ((ys % th) // (th // sy)) * sx + (xs % tw) // (tw // sx)
        slot = (tile * (sy * sx) + sub).reshape(1, plane).expand(n, plane)
        return torch.arange(n)[:, None].expand(n, plane), slot, -(-h // th) * -(-w // tw) * sy * sx
    R = geom[1]
    slab = torch.arange(n * plane).reshape(n, plane) // R
    owner = torch.arange(n)[:, None].expand(n, plane)
    if straddle_first:  # a slab's pixels all go to the sample its first row lies in
        owner = (slab * R) // plane
    return owner, slab - (owner * plane) // R, -(-plane // R) + 1


def _partials(z, owner, slot, nslots):
    """(n, nslots, C / 8, 2): (sum, sum of squares) per owner sample, slot and 8-channel octet."""
    n, h, w, C = z.shape
    zz = z.reshape(n * h * w, C // 8, 8)
    idx = (owner * nslots + slot).reshape(-1)
    s1 = torch.zeros(n * nslots, C // 8, dtype=z.dtype).index_add_(0, idx, zz.sum(-1))
    s2 = torch.zeros(n * nslots, C // 8, dtype=z.dtype).index_add_(0, idx, zz.pow(2).sum(-1))
    return torch.stack([s1, s2], -1).reshape(n, nslots, C // 8, 2)


# ----------------------------------------------------------------------------------------------------------------------- the op
MUTANTS = ("stats_no_bias", "tile_pixels", "slot_dropped", "straddle_first", "cpg64", "film_per_sample", "bias_not_in_c", "unbiased",
           "residual_before_drop")


def conv3x3(xs, wt):
    """3x3 / stride 1 / pad 1 conv of the channel concatenation of NHWC sources -> NHWC."""
    x = torch.cat(list(xs), 3).permute(0, 3, 1, 2)
    return F.conv2d(x, wt, None, 1, 1).permute(0, 2, 3, 1).contiguous()


def conv_gn(xs, wt, bias, gamma, beta, groups, film=None, coef_div=1, residual=None, keep=None, p=0.0, mutant=None, geom=None, acc=None):
    """The fused chain.  `acc`: the conv of (xs, wt) if the caller already has it.  mutant "partials": the same statement with the
    statistics taken from per-slot partials of `geom` (nothing edited); the statistics mutants need `geom` too."""
    acc = conv3x3(xs, wt) if acc is None else acc
    z = acc + bias
    n, h, w, C = z.shape
    gn = lambda t, **kw: S.group_norm(t, gamma, beta, groups, "silu", kw.pop("film", film), kw.pop("div", coef_div), residual, keep, p, **kw)
    if mutant in (None, "unbiased", "residual_before_drop"):
        return gn(z, mutant=mutant)
    if mutant == "film_per_sample":  # row = sample (the rows that exist: ceil(n / coef_div))
        row = torch.arange(n).clamp(max=film[0].shape[0] - 1)
        return gn(z, film=(film[0][row], film[1][row]), div=1)
    owner, slot, ns = _slot_owner(geom, n, h, w, mutant == "straddle_first")
    part = _partials(acc if mutant == "stats_no_bias" else z, owner, slot, ns)
    if mutant == "slot_dropped":  # the last slot a sample's pixels reach never arrives
        part = part.clone()
        part[torch.arange(n), _slot_owner(geom, n, h, w)[1].max(1).values] = 0
    if mutant == "tile_pixels":  # the mean over the pixels the tiles (slabs) cover instead of the plane's
        counted = -(-h // geom[1]) * geom[1] * -(-w // geom[2]) * geom[2] if geom[0] == "tile" else -(-(h * w) // geom[1]) * geom[1]
        part = part * (h * w / counted)
    if mutant == "cpg64":  # the statistics of the whole 64-channel block for every group inside it
        # (every octet gets an eighth of its block's sums: a group of cpg channels then adds up to cpg / 64 of them, over count h w cpg)
        part = (part.reshape(n, ns, C // 64, 8, 2).sum(3, keepdim=True) / 8).expand(n, ns, C // 64, 8, 2).reshape(n, ns, C // 8, 2)
    return gn(acc if mutant == "bias_not_in_c" else z, part=part)


# --------------------------------------------------------------------------------------------------------------------- the cases
FEATURES = ("film", "coefdiv", "residual", "gendrop", "nsel", "maxslots", "all")


def _case(form, h, w, c0, c1, cout, groups, n=3, feature=None):
    cid = f"{form}-{h}x{w}-{c0}+{c1}>{cout}-g{groups}" + (f"-n{n}" if n != 3 else "") + (f"-{feature}" if feature else "")
    return dict(id=cid, form=form, h=h, w=w, c0=c0, c1=c1, cout=cout, groups=groups, n=n, feature=feature)


def _form_cases():
    c = []
    for h, w in ((16, 16), (20, 36), (12, 8), (33, 17)):  # one tile | ragged both ways, 6 slots | less than a tile | one-pixel strips
        c += [_case("gn16", h, w, 64, 0, 64, g) for g in (8, 4, 1)] + [_case("gn16", h, w, 128, 0, 128, g) for g in (16, 8, 2)]
        c += [_case("gn16", h, w, 128, 64, 64, 8), _case("gn16", h, w, 64, 64, 128, 8)]
    c += [_case("gn16", 15, 15, 256, 0, 256, 8), _case("gn16", 15, 15, 256, 0, 256, 4), _case("gn16", 15, 15, 256, 128, 256, 8)]  # the frag64 copy
    for h, w in ((16, 32), (30, 30)):  # one tile, 4 slots | 2 ragged tiles
        c += [_case("halo5", h, w, 64, 0, 64, 8), _case("halo5", h, w, 64, 0, 64, 1), _case("halo5", h, w, 128, 0, 128, 8),
              _case("halo5", h, w, 64, 64, 128, 8)]
    # 20 x 40 covers 39 % of its four 16 x 32 tiles (the rule asks 60 %), 128 + 64 has c1 != c0: left to the implicit-GEMM form
    c += [_case("halo5>bm128", 20, 40, 128, 0, 128, 8), _case("halo5>bm128", 30, 30, 128, 64, 128, 8)]
    for f in ("bm128", "bm256"):
        c += [_case(f, 16, 32, 128, 0, 128, 8), _case(f, 16, 32, 256, 128, 256, 32)]                        # 2-D tiles
        c += [_case(f, 15, 15, 128, 0, 128, 8), _case(f, 15, 15, 128, 0, 128, 2), _case(f, 15, 15, 256, 0, 256, 8),  # slabs straddle samples
              _case(f, 15, 15, 256, 128, 128, 16), _case(f, 15, 15, 256, 128, 256, 4)]
        c += [_case(f, 12, 12, 256, 0, 128, 16, n=5), _case(f, 12, 12, 128, 0, 256, 8, n=5)]
    c += [_case("bm128", 8, 8, 128, 0, 128, 8), _case("bm128", 8, 8, 256, 128, 256, 8)]
    # 1600 pixels are above DYF_GN16_C256_MAX_PLANE: the 256-channel copy of conv_gn16 leaves the plane to the implicit-GEMM form
    c += [_case("prod>bm128", 40, 40, 256, 0, 256, 8)]
    return c


FEATURE_BASE = {"gn16": (20, 36, 64, 0, 64), "halo5": (30, 30, 64, 0, 64), "bm128": (15, 15, 128, 0, 128), "bm256": (15, 15, 128, 0, 128)}
FORM_CASES = _form_cases()
FEATURE_CASES = [_case(f, *FEATURE_BASE[f], 8, feature=ft) for f in FEATURE_BASE for ft in FEATURES]
CASES = FORM_CASES + FEATURE_CASES
BY_ID = {c["id"]: c for c in CASES}
# planes no fused form of the ladder serves under the form's switches: fused = 0 (conv_igemm2_gn_slots: a slab would touch three samples)
UNSERVED = [_case("bm256", 8, 8, 128, 0, 128, 8), _case("bm256", 9, 7, 128, 0, 128, 8), _case("bm128", 9, 7, 128, 0, 128, 8)]


def _draw(key, *shape, scale=1.0):
    return S._rn(S._gen(*key), *shape, scale=scale)


_cache = {}


class Built:
    """One case drawn for one 16-bit type: the arguments of HipEngine.op_conv_gn as CPU tensors and `ref(dtype, mutant)`.  The sources,
    the weights and their conv are shared by every case of the same (n, plane, channels): the conv is computed once per dtype."""

    def __init__(self, case, dtname):
        self.case, self.dtname, dt = case, dtname, DTYPES[dtname]
        n, h, w, c0, c1, cout, groups = (case[k] for k in ("n", "h", "w", "c0", "c1", "cout", "groups"))
        ft = case["feature"]
        self.key = (n, h, w, c0, c1, cout, dtname == "fp16")
        if self.key not in _cache:
            g = S._gen(41, *self.key)
            xs = [S.round16(S._rn(g, n, h, w, c), dt) for c in (c0, c1) if c]
            wt = S._rn(g, cout, c0 + c1, 3, 3, scale=1.0 / math.sqrt(9 * (c0 + c1))).float()
            _cache[self.key] = dict(xs=xs, wt=wt, acc={})
        self.xs, self.wt = _cache[self.key]["xs"], _cache[self.key]["wt"]
        g = S._gen(43, *self.key, groups, FEATURES.index(ft) if ft else 99)
        off = 4.0 * torch.sign(S._rn(g, groups)) * (1.0 + 0.1 * S._rn(g, groups))
        self.bias = (off[torch.arange(cout) // (cout // groups)] + S._rn(g, cout, scale=0.5)).float()
        self.gamma, self.beta = S._affine(g, cout)
        self.geom = slot_geometry(case["form"], h, w)
        self.slots = slots_of(case["form"], h, w)
        self.coef_div = 2 if ft in ("coefdiv", "all") else 0
        self.film = self.residual = self.keep = None
        if ft in ("film", "coefdiv", "all"):  # stride > cout: junk behind the row that a kernel must not read
            self.film = S._film_rows(g, -(-n // self.coef_div) if self.coef_div else n, cout, cout + 8)
        if ft in ("residual", "all"):
            self.residual = S.round16(S._rn(g, n, h, w, cout), dt)
        self.gen = ft in ("gendrop", "all")
        if self.gen:
            self.keep = S.gen_keep((h, w, cout), n, P_DROP)
        self.n_sel = n + 4 if ft in ("nsel", "all") else 0
        self.max_slots = self.slots + 3 if ft in ("maxslots", "all") else self.slots

    def acc(self, dtype):
        a = _cache[self.key]["acc"]
        if dtype not in a:
            a[dtype] = conv3x3([t.to(dtype) for t in self.xs], self.wt.to(DTYPES[self.dtname]).to(dtype))
        return a[dtype]

    def ref(self, dtype=torch.float64, mutant=None, keep="own", residual="own"):
        c = lambda t: None if t is None else t.to(dtype)
        keep = self.keep if isinstance(keep, str) else keep
        residual = self.residual if isinstance(residual, str) else residual
        return conv_gn(None, None, c(self.bias), c(self.gamma), c(self.beta), self.case["groups"],
                       None if self.film is None else (c(self.film[0]), c(self.film[1])), max(self.coef_div, 1), c(residual), c(keep),
                       P_DROP if keep is not None else 0.0, mutant, self.geom, self.acc(dtype))


def two_step_excess(b):
    """What the UN-fused chain costs against the fused reference when nothing but the arithmetic is ideal: y = conv + bias rounded to 16
    bit, then GroupNorm .. SiLU of THAT tensor in float64 with the exact statistics of the unrounded y, rounded once -> its excess.  (The
    offset of 4 standard deviations makes y's 16-bit grid coarser than the normalised output's, so this is several floors.)"""
    dt = DTYPES[b.dtname]
    z = b.acc(torch.float64) + b.bias.double()
    n, h, w, _ = z.shape
    owner, slot, ns = _slot_owner(("tile", h, w, 1, 1), n, h, w)
    two = S.group_norm(S.round16(z, dt).double(), b.gamma.double(), b.beta.double(), b.case["groups"], "silu", part=_partials(z, owner, slot, ns))
    return S.excess_floor(S.round16(two, dt), b.ref(), dt)[0]


_built = {}


def build(case, dtname):
    k = (case["id"], dtname)
    if k not in _built:
        _built[k] = Built(case, dtname)
    return _built[k]


# which (case, mutant) pairs the bound must tell from the reference: for every mutant one case on every kernel form it applies to.
# INVISIBLE: pairs the bound cannot see, or where the mutant IS the reference -- listed so that the host test says so instead of asserting.
def _ids(*cases):
    return [c["id"] for c in cases]


_RAGGED = _ids(_case("gn16", 20, 36, 64, 0, 64, 8), _case("halo5", 30, 30, 64, 0, 64, 8), _case("bm128", 15, 15, 128, 0, 128, 8),
               _case("bm256", 15, 15, 128, 0, 128, 8))
_ALL = _ids(*[_case(f, *FEATURE_BASE[f], 8, feature="all") for f in FEATURE_BASE])
VISIBLE = {
    "stats_no_bias": _RAGGED,
    "tile_pixels": _RAGGED,
    "slot_dropped": _RAGGED + _ids(_case("gn16", 16, 16, 64, 0, 64, 8), _case("gn16", 15, 15, 256, 0, 256, 8), _case("halo5", 16, 32, 64, 0, 64, 8),
                                   _case("bm128", 16, 32, 128, 0, 128, 8), _case("bm256", 16, 32, 128, 0, 128, 8)),
    "straddle_first": _ids(_case("bm128", 15, 15, 128, 0, 128, 8), _case("bm256", 15, 15, 128, 0, 128, 8), _case("bm128", 12, 12, 256, 0, 128, 16, n=5),
                           _case("bm256", 12, 12, 256, 0, 128, 16, n=5)),
    "cpg64": _RAGGED + _ids(_case("gn16", 15, 15, 256, 0, 256, 8), _case("bm128", 15, 15, 256, 128, 128, 16)),
    "film_per_sample": _ALL + _ids(*[_case(f, *FEATURE_BASE[f], 8, feature="coefdiv") for f in FEATURE_BASE]),
    "bias_not_in_c": _RAGGED,
    # (the smallest group of each form: 1 / (2 count) of 1 / std has to reach the 16-bit floor)
    "unbiased": _ids(_case("gn16", 12, 8, 64, 0, 64, 8), _case("halo5", 16, 32, 64, 0, 64, 8), _case("bm128", 8, 8, 128, 0, 128, 8),
                     _case("bm256", 12, 12, 256, 0, 128, 16, n=5)),
    "residual_before_drop": _ALL,
}
INVISIBLE = {
    # one group per 64-channel block: "64 channels per group assumed" is then the truth
    "cpg64": _ids(_case("gn16", 20, 36, 64, 0, 64, 1), _case("bm256", 15, 15, 128, 0, 128, 2)),
    # planes the tiles cover exactly, and slab-aligned samples: nothing is ragged, nothing straddles
    "tile_pixels": _ids(_case("gn16", 16, 16, 64, 0, 64, 8), _case("halo5", 16, 32, 64, 0, 64, 8)),
    "straddle_first": _ids(_case("bm128", 16, 32, 128, 0, 128, 8), _case("bm256", 16, 32, 128, 0, 128, 8), _case("bm128", 8, 8, 128, 0, 128, 8)),
}


# ... in the bf16 build only: a group of conv_up_halo<5> holds at least 16 x 32 pixels x 8 channels, one of the 256-pixel implicit-GEMM
# form at least 128 x 8 (1152 on the smallest plane here): 1 / (2 count) of 1 / std stays under the bf16 floor (fp16 sees both)
INVISIBLE_BF16 = {"unbiased": _ids(_case("halo5", 16, 32, 64, 0, 64, 8), _case("bm256", 12, 12, 256, 0, 128, 16, n=5))}


# ------------------------------------------------------------------------------------------------ the statistics entry (want = "stats")
# the un-fused conv_up_halo_kernel<5> with its statistics epilogue, on the operands of the fused halo5 cases of the same shape
STATS_CASES = [_case("halo5", h, w, c, 0, c, 8) for h, w in ((16, 32), (30, 30)) for c in (64, 128)]
STATS_FORM, STATS_SWITCH = "conv_up_halo_kernel<5>", {"DYF_HALO5_MIN_TILES": 1}
STATS_P = 128 * 8  # elements one slot adds per octet: a wave's 128 pixels x 8 channels


def stats_bound(absc, bias, K):
    """Forward bound of the fp32 (sum, sum of squares) of y = conv + bias per (sample, octet), slots added exactly: every y is an fp32 sum
    of K products plus the bias (relative error (K + 1) u of T = conv(|x|, |w|) + |bias|), a slot adds P of them ((P - 1) u more), three
    more roundings in the wave reduction: |err| <= (K + P + 4) u sum(T) -- the f32_bound argument of tests/test_gpu_conv_forms.py.  The
    squares carry y's error twice: the same expression with 2 K, over sum(T^2).  -> (n, C / 8, 2)."""
    T = absc + bias.double().abs()
    n, h, w, C = T.shape
    T8 = T.reshape(n, h * w, C // 8, 8)
    u = 2.0 ** -24
    return torch.stack([(K + STATS_P + 4) * u * T8.sum((1, 3)), (2 * K + STATS_P + 4) * u * T8.pow(2).sum((1, 3))], -1)
