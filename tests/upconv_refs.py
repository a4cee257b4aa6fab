"""The plain reference of the fused Upsample(x2, bilinear, align_corners=False) + Conv2d(3x3, pad 1) convs (dec3 .. dec5 of unet_simple:
csrc/conv.hip conv_igemm_kernel<.., UP>, csrc/conv_up_halo.hip, csrc/conv_halo_rows.hip), the cases tests/test_gpu_upconv_forms.py runs
through HipEngine.op_upconv2d_ex (dyf_op_upconv2d_ex), and mutants -- test infrastructure, no GPU.  The bound and the rounding are
tests/sample_op_refs.py's: excess <= floor.

Model A is the OPERAND model the kernels' header documents (csrc/conv.hip, "PHASE DECOMPOSITION"), derived here from the float64
resample matrix alone.  Along one axis, output o = 2 i + p (phase p) of a 3-tap conv over the upsampled axis reads upsampled positions
o + k - 1; in the interior each of them is a fixed mix of the low-res samples i - 1, i, i + 1, which gives E[p][a][k], the coefficient of
kernel tap k in stencil tap a.  Replicate-clamping i + a reproduces the matrix at the edges for every upsampled position INSIDE the
image; the conv's zero padding (position -1 or 2 n) is what the clamp cannot express, and the difference "true operator minus clamped
stencil" is one coefficient on the edge sample of the first / last output: the correction E[p][3][k].  The 2-D operator is the product
(stencil_y + correction_y) (stencil_x + correction_x): nine stencil taps, three row-correction taps (first / last output row), three
column-correction taps and one corner tap (inclusion / exclusion) -- 16 taps per phase, each a float64 combination of the 3x3 kernel,
each rounded to the build's 16-bit type as the operand is defined (v.float().to(dt)).  Everything else is float64: sources concatenated
on channels, affine row n // coef_div, activation, keep / (1 - p); a sparse case gathers the needed columns.

Model B is F.interpolate(bilinear) in float64 followed by F.conv2d(pad 1), no rounding of any weight.  A with unrounded taps equals B
(tests/test_upconv_refs.py): that identity is what validates A without the engine.

The mutants are mistakes these kernels could make; REGIONS is where the bound is evaluated (a whole-tensor bound cannot see the ring).
"""
import math

import torch
import torch.nn.functional as F

from tests import sample_op_refs as S

DTYPES = S.DTYPES
P_DROP = S.P_DROP
REGIONS = ("interior", "row0", "rowL", "col0", "colL", "corners")
RING = ("row0", "rowL", "col0", "colL", "corners")
NS_IW, NS_OW = 256, 42  # the NS geometry: dec5's output is 256 columns wide, the readout resamples its 512 to 42 native columns


# ------------------------------------------------------------------------------------------------------------- the operand model
def phase_factors(dtype=torch.float64):
    """E (2, 4, 3): E[p][a + 1][k] for the stencil taps a = -1, 0, +1 and E[p][3][k], the border correction, from the resample matrix."""
    n, i = 8, 3
    M = S._up_matrix(n, dtype)  # (2 n, n)
    E = torch.zeros(2, 4, 3, dtype=dtype)
    for p in range(2):
        for k in range(3):
            u = 2 * i + p + k - 1
            for a in (-1, 0, 1):
                E[p, a + 1, k] = M[u, i + a]
            assert float(M[u].sum() - E[p, :3, k].sum()) == 0.0  # nothing outside the three taps
    clamp = lambda v: min(max(v, 0), n - 1)
    for o in range(2 * n):  # true operator minus the clamped stencil, per kernel tap
        ii, p = o // 2, o % 2
        for k in range(3):
            u = o + k - 1
            d = M[u].clone() if 0 <= u < 2 * n else torch.zeros(n, dtype=dtype)
            for a in (-1, 0, 1):
                d[clamp(ii + a)] -= E[p, a + 1, k]
            edge = 0 if p == 0 else n - 1
            if o in (0, 2 * n - 1):
                E[p, 3, k] = d[edge]
                d[edge] = 0
            assert float(d.abs().max()) == 0.0, (o, k)  # the correction lives on the edge sample of the first / last output only
    return E


def taps(wt, dt=None):
    """(2, 2, cout, cin, 4, 4) float64: per phase (py, px) the tap weights [a + 1 or 3 = correction][b + 1 or 3]; dt: each rounded to it."""
    E = phase_factors()
    W = torch.einsum("pak,qbl,oikl->pqoiab", E, E, wt.double())
    return W if dt is None else W.float().to(dt).double()


def upconv_acc(xs, W, mutant=None):
    """Model A in the dtype of its arguments: NHWC sources (n, h, w, c), W from taps() -> (n, 2h, 2w, cout)."""
    if mutant == "src_swapped":
        xs = xs[::-1]
    if mutant == "skip_offset0" and len(xs) > 1:  # the skip's K chunks read at channel offset 0 of the concatenation: the first source again
        xs = [xs[0], xs[0][..., :xs[1].shape[3]]]
    x = torch.cat(list(xs), 3).permute(0, 3, 1, 2)
    n, _, h, w = x.shape
    cout = W.shape[2]
    mode = {"edge_zero": "constant", "edge_mirrored": "reflect"}.get(mutant, "replicate")
    xp = F.pad(x, (1, 1, 1, 1), mode=mode)
    if mutant == "halo_next_sample":  # the halo row under the last low-res row: the next sample's first row
        xp = xp.clone()
        xp[:, :, h + 1] = xp.roll(-1, 0)[:, :, 1]
    out = x.new_zeros(n, 2 * h, 2 * w, cout)
    for py in range(2):
        for px in range(2):
            Wp = W[px, py] if mutant == "phase_swapped" else W[py, px]
            y = F.conv2d(xp, Wp[:, :, :3, :3])
            r, c = (0 if py == 0 else h - 1), (0 if px == 0 else w - 1)
            if mutant != ("row_first_dropped", "row_last_dropped")[py]:
                y[:, :, r, :] += F.conv2d(xp[:, :, r + 1:r + 2, :], Wp[:, :, 3:4, :3])[:, :, 0, :]
            if mutant != ("col_first_dropped", "col_last_dropped")[px]:
                y[:, :, :, c] += F.conv2d(xp[:, :, :, c + 1:c + 2], Wp[:, :, :3, 3:4])[:, :, :, 0]
            if mutant != "corner_dropped":
                y[:, :, r, c] += (-1.0 if mutant == "corner_sign" else 1.0) * (x[:, :, r, c] @ Wp[:, :, 3, 3].T)
            out[:, py::2, px::2] = y.permute(0, 2, 3, 1)
    return out


def model_b(xs, wt, align_corners=False):
    """F.interpolate(x2, bilinear) then F.conv2d(pad 1) -> NHWC."""
    x = torch.cat(list(xs), 3).permute(0, 3, 1, 2)
    up = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=align_corners)
    return F.conv2d(up, wt.to(x.dtype), None, 1, 1).permute(0, 2, 3, 1).contiguous()


def _act(v, act):
    if act == 1:
        return v.clamp_min(0.0)
    if act == 2:
        return torch.where(v > 0, v, 0.2 * v)
    if act == 3:
        return v * torch.sigmoid(v)
    assert act == 0
    return v


def epilogue(acc, scale, shift, coef_div=0, act=0, keep=None, p=0.0, mutant=None):
    """tests/test_gpu_conv_forms.py epilogue_f64's chain in the dtype of its arguments: affine row n // coef_div -> act -> keep / (1 - p)."""
    n = acc.shape[0]
    rows = torch.arange(n) // coef_div if coef_div > 1 else torch.arange(n)
    if mutant == "coef_per_sample":  # (the rows that exist: ceil(n / coef_div))
        rows = torch.arange(n).clamp(max=scale.shape[0] - 1)
    v = acc * scale[rows][:, None, None, :] + shift[rows][:, None, None, :]
    if keep is None:
        return _act(v, act)
    if mutant == "drop_before_act":
        return _act(v * keep * (1.0 / (1.0 - p)), act)
    return _act(v, act) * keep * (1.0 / (1.0 - p))


def seam_columns(w, tile):
    """Low-res columns j that start a `tile`-column tile inside the plane."""
    return list(range(tile, w, tile))


def regions(ho, wo, cols=None):
    """name -> boolean mask (ho, stored columns): `cols` = the dense column of every stored column (None: all).  Empty regions are left out."""
    cols = torch.arange(wo) if cols is None else torch.as_tensor(cols)
    ys = torch.arange(ho)[:, None].expand(ho, len(cols))
    xs = cols[None, :].expand(ho, len(cols))
    top, bot, left, right = ys == 0, ys == ho - 1, xs == 0, xs == wo - 1
    m = {"interior": ~(top | bot | left | right), "row0": top, "rowL": bot, "col0": left, "colL": right, "corners": (top | bot) & (left | right)}
    return {k: v for k, v in m.items() if bool(v.any())}


# --------------------------------------------------------------------------------------------------------------------- the cases
def ns_needed():
    """The output columns of dec5 the NS readout reads (sample_op_refs.readout_columns) -> bool (256,)."""
    used, _ = S.readout_columns(NS_IW, NS_OW, False)
    m = torch.zeros(NS_IW, dtype=torch.bool)
    m[used] = True
    return m


def needed_of(kind, wo):
    """ns: the NS set (it stores neither column 0 nor column 255); edges / edges16: the NS set and columns 0, 1, 254, 255; ragged: the NS set without three of its odd columns (nvalid0 != nvalid1); declined: fifteen columns in every
    sixteen (128 entries in the even list: neither tiling saves anything, the planners decline)."""
    if kind is None:
        return None
    if kind == "declined":
        return torch.arange(wo) % 16 != 15
    assert wo == NS_IW
    m = ns_needed()
    if kind in ("edges", "edges16"):  # ... with the first and the last two columns: the sparse forms' own left / right border and corners
        if kind == "edges16":  # two columns fewer per phase: 52 entries again, 13 per 16-slot tile, which then fit the 40-column halo
            for px in (0, 1):
                own = [int(c) for c in m.nonzero().flatten() if int(c) % 2 == px]
                m[[own[25], own[26]]] = False
        m[[0, 1, wo - 2, wo - 1]] = True
    if kind == "ragged":
        odd = [int(c) for c in m.nonzero().flatten() if int(c) % 2 == 1]
        m[[odd[3], odd[20], odd[41]]] = False
    return m


# form -> (the form-log notes of a launch: conv_* and up_border*, the DYF_* switches that bring a small problem to the form, needed kind)
SPLIT, RING4 = "up_border_split_kernel", "up_border_ring4_kernel"
IG128, IG256 = "conv_igemm_kernel<128,128,UP>", "conv_igemm_kernel<256,64,UP>"
HALO0, HALO1, ROWS0, ROWS1 = "conv_up_halo_kernel<0>", "conv_up_halo_kernel<1>", "conv_halo_rows_kernel<0>", "conv_halo_rows_kernel<1>"
_ROWS4 = {"DYF_HALO_MIN_PLANE": 8, "DYF_ROWS_TR": 4, "DYF_HALO_SPLITK": 0}
FORMS = {
    "igemm128": ({IG128}, {"DYF_UP_HALO": 0}, None),
    "igemm256": ({IG256}, {"DYF_UP_HALO": 0}, None),
    "halo0": ({HALO0, SPLIT}, {"DYF_HALO_MIN_PLANE": 8}, None),  # (w % 32 != 0 keeps the rows form away)
    "halo0-norows": ({HALO0, SPLIT}, {"DYF_HALO_MIN_PLANE": 8, "DYF_HALO_ROWS": 0}, None),
    "halo0-xcd": ({HALO0, SPLIT}, {"DYF_HALO_MIN_PLANE": 8, "DYF_HALO_ROWS": 0, "DYF_HALO_TN_XCD": 1}, None),
    "rows0": ({ROWS0, SPLIT}, _ROWS4, None),
    "rows0+tr2": ({ROWS0 + "+tr2", SPLIT}, {"DYF_HALO_MIN_PLANE": 8, "DYF_ROWS_TR": 2}, None),
    "rows0+tr1": ({ROWS0 + "+tr1", SPLIT}, {"DYF_HALO_MIN_PLANE": 8, "DYF_ROWS_TR": 1}, None),
    "rows0+splitk2": ({ROWS0 + "+splitk", SPLIT}, {"DYF_HALO_MIN_PLANE": 8, "DYF_ROWS_TR": 4, "DYF_HALO_SPLITK_FORCE": 2}, None),
    "rows0+splitk4": ({ROWS0 + "+splitk", SPLIT}, {"DYF_HALO_MIN_PLANE": 8, "DYF_ROWS_TR": 4, "DYF_HALO_SPLITK_FORCE": 4}, None),
    # the border ring's other two kernels (up_border_kernel notes nothing: no up_border* note next to a halo form IS its pin)
    "border8": ({ROWS0}, dict(_ROWS4, DYF_UP_BORDER_SPLIT_ROWS=0), None),
    "border8-nsel80": ({ROWS0}, {}, None),  # 32 x 64, n_sel = 80: 1280 four-row tiles (no short tiles), one K chunk (no split)
    "ring4": ({ROWS0, RING4}, dict(_ROWS4, DYF_UP_BORDER_SPLIT_ROWS=0, DYF_UP_BORDER_RING4=1), None),
    "mixed": ({ROWS1, SPLIT}, {}, "ns"),
    "mixed-2grids": ({ROWS1, SPLIT}, {"DYF_SPARSE_MIXED_ONE_GRID": 0}, "ns"),
    "uniform32": ({ROWS1, SPLIT}, {"DYF_SPARSE_MIXED": 0}, "ns"),
    "halo1": ({HALO1, SPLIT}, {"DYF_HALO_ROWS": 0}, "ns"),
    "ragged": ({ROWS1, SPLIT}, {}, "ragged"),
    "edges": ({ROWS1, SPLIT}, {}, "edges"),
    "edges-halo1": ({HALO1, SPLIT}, {"DYF_HALO_ROWS": 0}, "edges16"),
    "declined": ({ROWS0, SPLIT}, {"DYF_ROWS_TR": 4, "DYF_HALO_SPLITK": 0}, "declined"),
}
# the plan a sparse row is there for (dyf_upconv_sparse): 52 entries per phase = 3 x 16 + 4, two uniform tiles of 32, four of 16
PLANS = {
    "mixed": dict(planned=1, mix=[0, 3, 1], ntiles=4, npad=52, nvalid0=52, nvalid1=52, wo_store=104),
    "mixed-2grids": dict(planned=1, mix=[0, 3, 1], ntiles=4, npad=52, nvalid0=52, nvalid1=52, wo_store=104),
    "uniform32": dict(planned=1, mix=[0, 0, 0], ntiles=2, npad=64, nvalid0=52, nvalid1=52, wo_store=104),
    "halo1": dict(planned=1, mix=[0, 0, 0], ntiles=4, npad=64, nvalid0=52, nvalid1=52, wo_store=104),
    "ragged": dict(planned=1, mix=[0, 0, 0], ntiles=2, npad=64, nvalid0=52, nvalid1=49, wo_store=101),  # (the mixed planner declines: a 16-entry tile of the shorter list does not fit)
    "edges": dict(planned=1, nvalid0=54, nvalid1=54, wo_store=108), "edges-halo1": dict(planned=1, mix=[0, 0, 0], ntiles=4, npad=64, nvalid0=52, nvalid1=52, wo_store=104),
    "declined": dict(planned=0),
}
# the dense launch a sparse rows plan is compared with bit for bit on the stored columns (see test_gpu_upconv_forms.py)
DENSE_OF = {"mixed": "rows0", "mixed-2grids": "rows0", "uniform32": "rows0", "ragged": "rows0", "edges": "rows0", "halo1": "halo0-norows",
            "edges-halo1": "halo0-norows"}
KERNEL_OF = {"halo0-norows": "halo0", "halo0-xcd": "halo0", "border8": "up_border_kernel", "border8-nsel80": "up_border_kernel", "ring4": "up_border_ring4",
             "mixed-2grids": "mixed", "edges-halo1": "halo1"}

FEATURES = ("base", "src2", "coefdiv", "act0", "act1", "act2", "act3", "mask2", "rng1", "nsel")


def _case(form, h, w, c0, cout, n=3, feature="base", c1=None, n_sel=0):
    c1 = (c0 if feature == "src2" else 0) if c1 is None else c1
    cid = f"{form}-{h}x{w}-{c0}+{c1}>{cout}-n{n}-{feature}"
    return dict(id=cid, form=form, h=h, w=w, c0=c0, c1=c1, cout=cout, n=n, feature=feature, n_sel=n_sel, needed=FORMS[form][2])


# (conv_mfma_supported, which the network forward asks too: cout % 128 == 0 tiles the low-res plane by 8 rows, cout 64 by 16 -- the 8- and
# 24-row planes run with 128 output channels)
# form row -> (h, w, c0 of the base / per source of the src2 column, cout, n).  Planes: 8 x 32 (every tile touches the top and the bottom),
# 16 x 32, 24 x 48 (w % 32 != 0: conv_up_halo_kernel<0>, with an interior tile), 32 x 64, 32 x 128 (the NS lists need 128 low-res columns)
ROWS = {
    "igemm128": (8, 32, 192, 64, 128, 3), "igemm256": (16, 32, 64, 64, 64, 3),
    "halo0": (24, 48, 64, 64, 128, 3), "halo0-xcd": (8, 32, 64, 64, 128, 3),
    "rows0": (8, 32, 64, 128, 128, 3), "rows0+tr2": (16, 32, 64, 64, 64, 3), "rows0+tr1": (16, 32, 64, 64, 128, 3),
    "rows0+splitk2": (16, 32, 128, 64, 64, 3), "rows0+splitk4": (8, 32, 256, 128, 128, 3),
    "border8": (16, 32, 64, 64, 64, 9), "ring4": (16, 32, 64, 64, 64, 9),
    "mixed": (32, 128, 64, 64, 64, 3), "mixed-2grids": (32, 128, 64, 64, 64, 3), "uniform32": (32, 128, 64, 64, 64, 3),
    "halo1": (32, 128, 64, 64, 64, 3),
}


def _matrix():
    c = []
    for form, (h, w, c0, c2, cout, n) in ROWS.items():
        for ft in FEATURES:
            c.append(_case(form, h, w, c2 if ft == "src2" else c0, cout, n, ft, n_sel=n + 5 if ft == "nsel" else 0))
    return c


MATRIX = _matrix()
EXTRA = [
    _case("border8-nsel80", 32, 64, 64, 64, 9, n_sel=80),  # the 80-row benchmark's ring kernel without a switch
    _case("halo0-norows", 32, 128, 64, 64, 3),            # the dense launch conv_up_halo_kernel<1> is compared with
    _case("rows0", 32, 128, 64, 64, 3),                   # ... and the one the rows plans are compared with
    _case("rows0", 32, 64, 64, 64, 3),                    # an interior 4 x 32 tile
    _case("ragged", 32, 128, 64, 64, 3), _case("ragged", 32, 128, 64, 64, 3, "mask2"),
    _case("edges", 32, 128, 64, 64, 3), _case("edges", 32, 128, 64, 64, 3, "rng1"), _case("edges-halo1", 32, 128, 64, 64, 3),
    _case("declined", 32, 128, 64, 64, 3),
]
# unequal sources: the halo forms turn 128 + 64 away (c1 == c0 or 0), the ladder falls to the implicit-GEMM form WITHOUT a switch
FALLS = [_case("igemm128", 32, 32, 128, 128, 3, c1=64), _case("igemm256", 32, 32, 128, 64, 3, c1=64)]
CASES = MATRIX + EXTRA + FALLS
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)


_cache = {}


class Built:
    """One case drawn for one 16-bit type: the arguments of HipEngine.op_upconv2d_ex as CPU tensors and `ref(dtype, mutant)`.  Sources,
    weights and their model-A accumulator are shared by every case of the same (n, plane, channels): computed once per dtype."""

    def __init__(self, case, dtname):
        self.case, self.dtname, self.dt = case, dtname, DTYPES[dtname]
        n, h, w, c0, c1, cout = (case[k] for k in ("n", "h", "w", "c0", "c1", "cout"))
        ft = case["feature"]
        self.key = (n, h, w, c0, c1, cout, dtname == "fp16")
        if self.key not in _cache:
            g = S._gen(51, *self.key)
            xs = [S.round16(S._rn(g, n, h, w, c), self.dt) for c in (c0, c1) if c]
            wt = S._rn(g, cout, c0 + c1, 3, 3, scale=1.0 / math.sqrt(9 * (c0 + c1))).float()
            _cache[self.key] = dict(xs=xs, wt=wt, acc={})
        self.xs, self.wt = _cache[self.key]["xs"], _cache[self.key]["wt"]
        g = S._gen(57, *self.key, FEATURES.index(ft))
        self.coef_div = 2 if ft == "coefdiv" else 0
        rows = -(-n // self.coef_div) if self.coef_div else n
        self.scale = (1.0 + S._rn(g, rows, cout, scale=0.3)).float()
        # (a dropout case: shift 0.5 keeps every element away from zero in front of the mask, see exact_mask)
        self.shift = ((0.5 if ft in ("mask2", "rng1") else 0.0) + S._rn(g, rows, cout, scale=0.2)).float()
        self.act = {"act0": 0, "act1": 1, "act2": 2, "act3": 3, "base": 1, "mask2": 3, "rng1": 3}.get(ft, 2)
        self.keep = self.mask = None
        self.gen = ft == "rng1"
        if ft == "mask2":
            self.mask = S._mask(g, (n, 2 * h, 2 * w, cout), P_DROP)
            self.keep = self.mask.double()
        elif self.gen:
            self.keep = S.gen_keep((2 * h, 2 * w, cout), n, P_DROP)
        self.needed = needed_of(case["needed"], 2 * w)
        self.cols = None if self.needed is None or case["form"] == "declined" else self.needed.nonzero().flatten()

    def acc(self, dtype, mutant=None):
        a = _cache[self.key]["acc"]
        if (dtype, mutant) not in a:
            if mutant == "align_corners":
                v = model_b([t.to(dtype) for t in self.xs], self.wt.to(self.dt).to(dtype), align_corners=True)
            elif mutant in ("seam16", "seam32"):  # the b = -1 tap of the first column of a tile read from the tile's own side
                w = self.case["w"]
                js = seam_columns(w, 16 if mutant == "seam16" else 32)
                xs2 = [t.clone() for t in self.xs]
                for t in xs2:
                    for j in js:
                        t[:, :, j - 1] = t[:, :, j + 1]
                v = self.acc(dtype).clone()
                v2 = upconv_acc([t.to(dtype) for t in xs2], taps(self.wt, self.dt).to(dtype))
                for j in js:
                    v[:, :, 2 * j:2 * j + 2] = v2[:, :, 2 * j:2 * j + 2]
            else:
                v = upconv_acc([t.to(dtype) for t in self.xs], taps(self.wt, self.dt).to(dtype), mutant)
            if mutant is not None:
                return v
            a[(dtype, mutant)] = v
        return a[(dtype, mutant)]

    def excess(self, got, only=None):
        """region -> (excess, floor) of a 16-bit result in the seam's layout against ref(), per region (`only`: these regions); the
        reference and its one-step rounding are computed once per case."""
        if not hasattr(self, "_r16"):
            ref = self.ref()
            self._ref, self._r16 = ref, S.round16(ref, self.dt).double()
            self._masks = regions(ref.shape[1], 2 * self.case["w"], self.cols)
        out = {}
        for name, m in self._masks.items():
            if only is None or name in only:
                ref, r16 = self._ref[:, m], self._r16[:, m]
                den = max(S.rms(ref), 1e-300)
                out[name] = (S.rms(got[:, m].double() - r16) / den, S.rms(r16 - ref) / den)
        return out

    def gather(self, t):
        return t if self.cols is None else t[:, :, self.cols]

    def ref(self, dtype=torch.float64, mutant=None, keep="own", dense=False):
        """The result as the seam returns it (compact for a sparse case unless `dense`)."""
        c = lambda t: None if t is None else t.to(dtype)
        keep = self.keep if isinstance(keep, str) else keep
        acc = self.acc(dtype, mutant if mutant in ACC_MUTANTS else None)
        compact = self.cols is not None and not dense
        if compact:  # (the epilogue is elementwise in the columns: gather first)
            acc = self.gather(acc)
            if keep is not None:
                n, ho, ws, cout = acc.shape
                # drop_compact_pos: the mask / generator index (oy * wo_store + c) * cout + co of the sample instead of the dense one
                keep = keep.reshape(n, -1)[:, :ho * ws * cout].reshape(n, ho, ws, cout) if mutant == "drop_compact_pos" else self.gather(keep)
        out = epilogue(acc, c(self.scale), c(self.shift), self.coef_div, self.act, c(keep), P_DROP if keep is not None else 0.0, mutant)
        if compact and mutant == "slot_shifted":  # one list slot stored one compact column to the right (its own column keeps what the buffer held)
            s = out.shape[2] // 2
            out = out.clone()
            out[:, :, s + 1] = out[:, :, s]
            out[:, :, s] = 0
        return out  # (pad_slot_stored: see INVISIBLE -- the mutant IS the reference)


ACC_MUTANTS = ("row_first_dropped", "row_last_dropped", "col_first_dropped", "col_last_dropped", "corner_dropped", "corner_sign", "edge_zero",
               "edge_mirrored", "phase_swapped", "align_corners", "src_swapped", "skip_offset0", "halo_next_sample", "seam16", "seam32")
MUTANTS = ACC_MUTANTS + ("coef_per_sample", "slot_shifted", "pad_slot_stored", "drop_before_act", "drop_compact_pos")

_built = {}


def build(case, dtname):
    k = (case["id"], dtname)
    if k not in _built:
        _built[k] = Built(case, dtname)
    return _built[k]


# ------------------------------------------------------------------------------------------- which mutant must be seen where
ALL = REGIONS


def applies(mutant, case):
    """The regions of `case` on which `mutant` changes the operation (empty: it does not apply to the case)."""
    two, sparse, ft = case["c1"] > 0, case["needed"] in ("ns", "ragged", "edges", "edges16"), case["feature"]
    if mutant in ("row_first_dropped",):
        return ("row0", "corners")
    if mutant in ("row_last_dropped", "halo_next_sample"):
        return ("rowL", "corners")
    if mutant == "col_first_dropped":
        return ("col0", "corners")
    if mutant == "col_last_dropped":
        return ("colL", "corners")
    if mutant in ("corner_dropped", "corner_sign"):
        return ("corners",)
    if mutant in ("edge_zero", "edge_mirrored"):
        return RING
    if mutant in ("phase_swapped", "align_corners"):
        return ALL
    if mutant in ("src_swapped", "skip_offset0"):
        return ALL if two else ()
    if mutant == "coef_per_sample":
        return ALL if ft == "coefdiv" else ()
    if mutant in ("seam16", "seam32"):  # (a sparse case sees a seam only where it stores one of the seam column's two outputs)
        js = seam_columns(case["w"], 16 if mutant == "seam16" else 32)
        if sparse:
            need = needed_of(case["needed"], 2 * case["w"])
            js = [j for j in js if bool(need[2 * j]) or bool(need[2 * j + 1])]
        return ("interior", "row0", "rowL") if js else ()
    if mutant in ("slot_shifted", "pad_slot_stored"):
        return ("interior", "row0", "rowL") if sparse else ()
    if mutant == "drop_before_act":
        return ALL if ft in ("mask2", "rng1") else ()
    if mutant == "drop_compact_pos":
        return ALL if sparse and ft in ("mask2", "rng1") else ()
    raise KeyError(mutant)


# Mutants the bound cannot see, with the reason -- the host test says so (and checks the reason) instead of asserting.
INVISIBLE = {
    # plan_up_sparse_columns[_mixed]: a padded slot repeats its list's last column AND carries that column's compact index, so storing
    # it writes the same value to the same place: the mutant is the reference on every sparse case, whatever the plan
    "pad_slot_stored": "a padded slot carries the compact index of the column it repeats",
}
