"""References, cases and bounds of the SimpleConvNet SAMPLING path (dyffusion_amd/csrc/simple_conv_net.hip: sc_forward, sc_f32_forward,
one conv_direct_kernel launch per block) for tests/test_scn_sample_refs.py (CPU) and tests/test_gpu_scn_sample_ops.py -- test
infrastructure, no GPU.

E64, the exact reference: tests/scn_train_refs.py::forward in float64, eval-mode BatchNorm, erf GELU, the keep masks handed in.

M(dtype), the rounding model: the same network with the engine's rounding points, read off sc_load_weights / sc_forward /
conv_direct_kernel:
    cat[inputs, condition] -> 16 bit                         (pack_inputs_kernel)
    conv weights -> 16 bit                                   (pack_conv)
    a = gamma / sqrt(var + 1e-5), c = beta + (conv bias - mean) a   in double, stored fp32 (sc_load_weights)
    A = a (1 + scale), C = c (1 + scale) + shift             fp32 rows of compute_coefs, row = batch row, slice = block
    v = conv * A + C -> erf GELU -> keep ? v / (1 - p) : 0 -> + block input (cin == dim) -> 16 bit, ONCE per block
    head: fp32 weights on the 16-bit activations, fp32 out
evaluated in float64 (M64, what the 16-bit checks compare with) and in float32 (M32, "what does fp32 arithmetic cost").  With the
rounding switched off M is E64 (tested).  `mutant=` turns M into one of the mistakes this path could make (MUTANTS).

Bounds, all from the references alone:
    16-bit forward:  floor = rel_rms(M64, E64), what the 16-bit storage itself costs; rel_rms(engine, M64) <= floor.  A kernel that
                     computes in fp32 and rounds once per block leaves M64 only where an fp32 error crosses a 16-bit rounding boundary.
    fp32 / bf16x3:   rel_rms(engine, E64) <= 1e-5 (tests/train_op_refs.TOL).
    one block (op_conv2d_ex, path 0): tests/sample_op_refs.excess_floor, excess <= floor.

Measured on the CPU (tests/test_scn_sample_refs.py prints them; worst over the dropout modes of a case; "mutant" = the smallest ratio
mutant / floor over the (mutant, case) pairs of MUTANTS aimed at that case and type, "-" = none aimed there), and on an MI355X
(tests/test_gpu_scn_sample_ops.py, "engine" = worst rel_rms(engine, M64) / floor over the dropout modes and both generator forwards):

    case            bf16 floor (min..max)  M32/floor  mutant  engine  |  fp16 floor (min..max)  M32/floor  mutant  engine
    golden-shape    2.56e-03..2.73e-03  0.000      2.7  0.000  |  3.21e-04..3.37e-04  0.148     19.6  0.148
    wide            3.08e-03..3.34e-03  0.038    148.3  0.039  |  3.78e-04..3.88e-04  0.422     16.2  0.379
    tall            3.15e-03..3.48e-03  0.213     11.2  0.213  |  3.94e-04..4.38e-04  0.321     11.8  0.220
    flat            1.60e-03..1.94e-03  0.000     80.9  0.000  |  1.43e-04..2.11e-04  0.001    745.7  0.001
    tiny-k15        2.72e-03..3.44e-03  0.000     10.2  0.000  |  3.73e-04..4.31e-04  0.000     70.8  0.000
    res0-64         2.09e-03..2.23e-03  0.000      3.5  0.000  |  2.40e-04..2.95e-04  0.006     31.9  0.009
    no-time         3.15e-03..3.15e-03  0.000    133.6  0.000  |  3.64e-04..3.64e-04  0.064      9.3  0.000
    one-row-batch   1.95e-03..2.30e-03  0.000      3.4  0.000  |  2.61e-04..2.90e-04  0.000     22.9  0.000
    fp32 torch against E64 (bound 1e-5): worst 3.39e-07 over the cases and modes.  Engine at precision 32 / 48 (GPU): worst 4.54e-07.
    block cases, excess / floor: fp32 torch rounded once (CPU) at most 0.258; conv_direct_kernel (GPU) at most 0.258.
    fp32 6 x 10 generator-dropout rollout against the oracle on host-rebuilt masks (bound 1e-4): 2.22e-07.
    The engine's ratios equal M32's almost everywhere: where it leaves M64 at all, it is the fp32 summation order.

One mutant is invisible to the whole forward: a block that rounds its output BEFORE the residual add sits at 0.9 .. 1.6 floors there (a
second rounding of the same size as the first).  It is held by a block case of its own, whose residual cancels 15/16 of the activation
(BLOCK_CASES, "cancel"): 16.6 floors.  tanh GELU (<= 4.7e-4 absolute) is aimed at the fp32 bound alone (9 .. 25 bounds), BatchNorm eps 1e-3
at the bf16 floor only where the case has a variance near 0.05 in a channel that matters (2.7, 3.4 floors), at the fp16 and fp32 bounds
everywhere.

The res0-64 case enters block 0 with 60 + 4 = 64 channels: the engine's 32-channel limit is the U-Nets' stem's and does not apply to
this backbone (dyf_engine_create).
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import init as oinit
from tests import rng_host
from tests import scn_train_refs as S
from tests import train_op_refs as T
from tests.helpers import rel_rms
from tests.sample_op_refs import DTYPES, excess_floor, round16  # noqa: F401  (re-exported for the two test files)

TOL = T.TOL  # rel-RMS of an fp32 forward against E64
SEED, ROW_OFFSET = 20261021, 5  # generator dropout: dyf_seed, dyf_set_row_offset
GAIN = 0.8
MODES = ("off", "mask", "gen")  # dropout off, injected masks, the engine generator's masks (forward 0; "gen1": forward 1)


# ------------------------------------------------------------------------------------------------------------------- the cases
def _case(cid, dim, n_in, n_cond, n_out, ks, h, w, nb, p=0.1, time_emb=True, max_batch=None):
    return dict(id=cid, dim=dim, n_in=n_in, n_cond=n_cond, n_out=n_out, ks=list(ks), h=h, w=w, nb=nb, p=p, time_emb=time_emb,
                max_batch=max_batch or nb)


CASES = [
    _case("golden-shape", 8, 8, 1, 4, (9, 7, 5, 3), 10, 10, 2),     # today's shape
    _case("wide", 64, 8, 1, 4, (9, 7, 5, 3), 10, 10, 3),            # BASELINE configs[0]
    _case("tall", 24, 4, 1, 4, (1, 5, 3, 7, 9, 3), 12, 7, 3, p=0.5),  # H != W, six blocks, dim % 8 != 0
    _case("flat", 8, 4, 1, 2, (9, 3), 1, 7, 2),                     # one row, kernel above the grid
    _case("tiny-k15", 8, 8, 0, 4, (3, 15), 3, 5, 3),                # first-block residual, no condition, k = 15
    _case("res0-64", 64, 60, 4, 3, (5,), 7, 3, 2),                  # one block, residual from the packed input
    _case("no-time", 8, 3, 1, 3, (5, 3), 5, 9, 3, p=0.0, time_emb=False),  # film_kernel without a time embedding; no dropout sites
    _case("one-row-batch", 8, 8, 1, 4, (7, 3), 10, 10, 1, max_batch=5),    # nb = 1 on an engine built for 5
]
CASE = {c["id"]: c for c in CASES}


def modes_of(case):
    return MODES if case["p"] > 0 else ("off",)


def model_cfg(case):
    return dict(dim=case["dim"], kernel_sizes=case["ks"], with_time_emb=case["time_emb"], dropout=case["p"], residual=True)


def _seed_of(case):
    return 7000 + 13 * CASES.index(case)


_built = {}


def build(cid):
    """-> dict(P, x, c, t, keeps): fp32 parameters (oracle.init.seeded_state at gain 0.8, the BatchNorm statistics / affine and the conv
    bias redrawn away from (0, 1): var log-uniform in [0.05, 1.5] with gamma ~ sqrt(var), so A stays O(1) while every term of the fold
    matters), inputs, one time value per row, injected NHWC uint8 keep masks per block."""
    if cid in _built:
        return _built[cid]
    case = CASE[cid]
    dim, nb, h, w = case["dim"], case["nb"], case["h"], case["w"]
    shapes = oinit.simple_conv_net_param_shapes(dim, case["n_in"] + case["n_cond"], case["n_out"], case["ks"], case["time_emb"])
    P = oinit.seeded_state(shapes, seed=_seed_of(case), gain=GAIN)
    g = torch.Generator().manual_seed(_seed_of(case) + 1)
    for i in range(len(case["ks"])):
        pre = f"convs.{i}"
        var = torch.exp(torch.empty(dim).uniform_(math.log(0.05), math.log(1.5), generator=g))
        P[f"{pre}.norm.running_var"] = var
        P[f"{pre}.norm.running_mean"] = 0.5 * torch.randn(dim, generator=g)
        P[f"{pre}.norm.weight"] = var.sqrt() * (1.0 + 0.3 * torch.randn(dim, generator=g))
        P[f"{pre}.norm.bias"] = 0.3 * torch.randn(dim, generator=g)
        P[f"{pre}.conv.bias"] = 0.5 * torch.randn(dim, generator=g)
    x = torch.randn(nb, case["n_in"], h, w, generator=g)
    c = torch.rand(nb, case["n_cond"], h, w, generator=g) if case["n_cond"] else None
    t = (torch.arange(nb, dtype=torch.float32) * 1.75 + 0.5 * torch.rand(nb, generator=g)) if case["time_emb"] else None
    keeps = [(torch.rand(nb, h, w, dim, generator=g) >= case["p"]).to(torch.uint8) for _ in case["ks"]] if case["p"] > 0 else None
    _built[cid] = dict(P=P, x=x, c=c, t=t, keeps=keeps)
    return _built[cid]


def gen_keeps(case, forward=0, mutant=None):
    """The generator's masks of one forward, rebuilt on the host: site i = block i, global row = ROW_OFFSET + r."""
    site = 1 if mutant == "gen_next_site" else 0
    row0 = 0 if mutant == "gen_local_row" else ROW_OFFSET
    fwd = 0 if mutant == "gen_forward0" else forward
    shape = (case["h"], case["w"], case["dim"])
    return [torch.from_numpy(np.stack([rng_host.row_mask_nhwc(shape, case["p"], SEED, fwd, i + site, row0 + r) for r in range(case["nb"])])
                             .astype(np.uint8)) for i in range(len(case["ks"]))]


def keeps_of(cid, mode, mutant=None):
    case = CASE[cid]
    if mode == "off" or case["p"] <= 0:
        return None
    if mode == "mask":
        return build(cid)["keeps"]
    return gen_keeps(case, 1 if mode == "gen1" else 0, mutant)


# ------------------------------------------------------------------------------------------------------------------- references
def exact(cid, mode="off", dtype=torch.float64, gelu=S.gelu_erf):
    """E64 (dtype float64) / fp32 torch (float32): tests/scn_train_refs.forward on the case."""
    b, case = build(cid), CASE[cid]
    keeps = keeps_of(cid, mode)
    drop = None if keeps is None else S.MaskList([k.permute(0, 3, 1, 2) for k in keeps])
    with torch.no_grad():
        return S.forward(S.to_dtype(b["P"], dtype), model_cfg(case), b["x"], b["t"], b["c"], dropout=drop, gelu=gelu)


def conv_block(x, w, A, C, pad, keep=None, scale=1.0, res=None, gelu=S.gelu_erf):
    """One block in front of its rounding, NCHW in the dtype of x: conv(x, w) * A + C -> GELU -> keep * scale -> + res.  A, C: (rows, cout)."""
    v = F.conv2d(x, w, None, padding=pad) * A[:, :, None, None] + C[:, :, None, None]
    v = gelu(v)
    if keep is not None:
        v = torch.where(keep != 0, v * scale, torch.zeros_like(v))
    return v if res is None else v + res


def model(P, cfg, x, t, c, dt=None, dtype=torch.float64, keeps=None, mutant=None):
    """M: dt = a 16-bit torch dtype (None: no rounding at all = the exact network), dtype = the arithmetic.  keeps: NHWC uint8 per block."""
    q = (lambda v: round16(v, dt).to(dtype)) if dt is not None else (lambda v: v)
    f32 = (lambda v: v.float().to(dtype)) if dt is not None else (lambda v: v.to(dtype))  # the fp32 storage of the coefficient tables
    Pd = S.to_dtype(P, dtype)
    dim, p = cfg["dim"], float(cfg.get("dropout", 0.0))
    srcs = [x.to(dtype)] + ([] if c is None else [c.to(dtype)])
    xx = q(torch.cat(srcs[::-1] if mutant == "cat_order" else srcs, 1))
    nb, _, H, W = xx.shape
    silu = F.silu(S.time_embedding(Pd, t, dim)) if cfg.get("with_time_emb", False) else None
    scale = 1.0 / (1.0 - p) if dt is None else float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))  # DropSpec::scale is fp32
    if mutant == "drop_scale" and p > 0:
        scale = 1.0 / p
    coefs = []
    for i in range(len(cfg["kernel_sizes"])):
        pre = f"convs.{i}"
        g64 = lambda k: P[f"{pre}.{k}"].double()
        a = g64("norm.weight") / torch.sqrt(g64("norm.running_var") + (1e-3 if mutant == "bn_eps" else 1e-5))
        cb = torch.zeros_like(a) if mutant == "no_conv_bias" else g64("conv.bias")
        cc = g64("norm.bias") + (cb - g64("norm.running_mean")) * a
        a, cc = f32(a), f32(cc)
        if silu is not None:
            ss = silu @ Pd[f"{pre}.time_mlp.1.weight"].T + Pd[f"{pre}.time_mlp.1.bias"]
            sc, sh = (ss[:, dim:], ss[:, :dim]) if mutant == "film_swapped" else (ss[:, :dim], ss[:, dim:])
            A, C = a * (1 + sc), cc * (1 + sc) + sh
        else:
            A, C = a[None].expand(nb, dim), cc[None].expand(nb, dim)
        if mutant == "coef_row0":
            A, C = A[:1].expand(nb, dim), C[:1].expand(nb, dim)
        coefs.append((f32(A), f32(C)))
    for i, k in enumerate(cfg["kernel_sizes"]):
        A, C = coefs[i - 1] if (mutant == "coef_prev_block" and i > 0) else coefs[i]
        w = q(Pd[f"convs.{i}.conv.weight"])
        pad = (k - 1) // 2
        keep = None
        if keeps is not None and p > 0:
            keep = keeps[i].reshape(nb, dim, H, W) if mutant == "mask_nchw" else keeps[i].permute(0, 3, 1, 2)
        res = xx if (xx.shape[1] == dim and not (mutant == "no_res0" and i == 0)) else None
        xin = xx
        if mutant == "hw_swapped":  # every NHWC buffer walked as (W, H): pixel index -> (index / H, index % H)
            walk = lambda v, a, b: None if v is None else v.permute(0, 2, 3, 1).reshape(nb, a, b, -1).permute(0, 3, 1, 2)
            xin, keep, res = walk(xx, W, H), walk(keep, W, H), walk(res, W, H)
        if mutant == "pad_short" and k > 1:  # pad k // 2 - 1: every tap reads one pixel further down / right
            xin, pad = F.pad(xin, (pad - 1, pad + 1, pad - 1, pad + 1)), 0
        late = mutant in ("drop_after_residual", "residual_after_rounding")
        v = conv_block(xin, w, A, C, pad, None if mutant == "drop_after_residual" else keep, scale, None if late else res,
                       S.gelu_tanh if mutant == "tanh_gelu" else S.gelu_erf)
        if mutant == "hw_swapped":
            v = walk(v, H, W)
        if mutant == "drop_after_residual":
            v = v if res is None else v + res
            if keep is not None:
                v = torch.where(keep != 0, v * scale, torch.zeros_like(v))
        if mutant == "residual_after_rounding" and res is not None:
            v = q(v) + res
        xx = q(v)
    return F.conv2d(xx, Pd["head.weight"], Pd["head.bias"])


def rounded(cid, dtname, mode="off", dtype=torch.float64, mutant=None):
    """M64 / M32 of a case: dtname "bf16" | "fp16" | None (no rounding)."""
    b, case = build(cid), CASE[cid]
    gen_mut = mutant if mutant in ("gen_next_site", "gen_local_row", "gen_forward0") else None
    with torch.no_grad():
        return model(b["P"], model_cfg(case), b["x"], b["t"], b["c"], None if dtname is None else DTYPES[dtname], dtype,
                     keeps_of(cid, mode, gen_mut), None if gen_mut else mutant)


_refs = {}


def refs(cid, dtname, mode):
    """(E64, M64, floor) of a case for a 16-bit type, E64 alone for dtname None; computed once, shared, never written to."""
    if (cid, None, mode) not in _refs:
        _refs[(cid, None, mode)] = exact(cid, mode)
    e = _refs[(cid, None, mode)]
    if dtname is None:
        return e
    if (cid, dtname, mode) not in _refs:
        m = rounded(cid, dtname, mode)
        _refs[(cid, dtname, mode)] = (e, m, rel_rms(m, e))
    return _refs[(cid, dtname, mode)]


# which (mutant -> [(case, mode, kind)]) pairs must miss the bound by a factor of 2 or more; kind = the bound the mutant is aimed at:
# "bf16" / "fp16": rel_rms(mutant M64, M64) against the floor of that type; "f32": rel_rms(mutant exact, E64) against TOL.
_W = lambda *cases, mode="off", kinds=("bf16", "fp16", "f32"): [(c, mode, k) for c in cases for k in kinds]
MUTANTS = {
    "hw_swapped": _W("tall", "flat", "tiny-k15", "res0-64", "no-time"),
    "pad_short": _W("golden-shape", "flat", "tiny-k15", "res0-64"),
    "no_res0": _W("tiny-k15", "res0-64"),
    "residual_after_rounding": [("k3-8to8-5x7-n2-cancel", "off", "block")],  # (a block case: see BLOCK_CASES)
    "coef_row0": _W("golden-shape", "tall", "tiny-k15", "res0-64"),
    "coef_prev_block": _W("golden-shape", "tall", "no-time"),
    "film_swapped": _W("golden-shape", "res0-64"),
    "no_conv_bias": _W("golden-shape", "no-time", "res0-64"),
    # (1e-3 against var >= 0.05: 1.1 .. 3.4 bf16 floors, 8 .. 23 fp16 floors, 190 .. 630 fp32 bounds over the cases)
    "bn_eps": _W("golden-shape", "one-row-batch") + _W("wide", "no-time", "tall", kinds=("fp16", "f32")),
    "tanh_gelu": _W("golden-shape", "tall", "res0-64", kinds=("f32",)),
    "drop_after_residual": _W("tall", "res0-64", "tiny-k15", mode="mask") + _W("tall", mode="gen"),
    "drop_scale": _W("golden-shape", "res0-64", mode="mask") + _W("wide", mode="gen"),
    "mask_nchw": _W("golden-shape", "tall", "flat", mode="mask"),
    "gen_next_site": _W("golden-shape", "tall", "res0-64", mode="gen"),
    "gen_local_row": _W("wide", "flat", "one-row-batch", mode="gen"),
    "gen_forward0": _W("tiny-k15", "tall", mode="gen1"),
    "cat_order": _W("golden-shape", "flat", "res0-64"),
}


def mutant_ratio(name, cid, mode, kind):
    """how far the mutant sits from the reference of its bound, in units of that bound ("block": the worse of the two 16-bit types)"""
    if kind == "block":
        out = []
        for dtname in DTYPES:
            b = block_build(next(bc for bc in BLOCK_CASES if block_id(bc) == cid), dtname)
            excess, floor = excess_floor(round16(b["ref"](mutant=name), b["dt"]), b["ref"](), b["dt"])
            out.append(excess / floor)
        return min(out)
    if kind == "f32":
        return rel_rms(rounded(cid, None, mode, mutant=name), refs(cid, None, mode)) / TOL
    _, m, floor = refs(cid, kind, mode)
    return rel_rms(rounded(cid, kind, mode, mutant=name), m) / floor


# ----------------------------------------------------------------------------------------------------- one block through the conv seam
#              k  cin cout  h   w  n  mask   residual
BLOCK_CASES = [(1, 9, 8, 3, 5, 3, True, None), (5, 64, 64, 1, 7, 2, False, "input"), (9, 9, 64, 10, 10, 2, True, None),
               (9, 64, 64, 12, 7, 2, False, "input"), (15, 8, 8, 3, 5, 3, True, "input"),
               # a residual that cancels 15/16 of the activation: the sum is 16 times finer than its terms, so a block that rounds
               # its output BEFORE the residual add (the one mutant the whole forward cannot tell from M, 0.9 .. 1.6 floors) shows here
               (3, 8, 8, 5, 7, 2, False, "cancel")]
BLOCK_P = 0.1


def block_id(bc):
    return "k{}-{}to{}-{}x{}-n{}{}{}".format(*bc[:6], "-mask" if bc[6] else "", "-cancel" if bc[7] == "cancel" else "")


def block_build(bc, dtname):
    """-> dict: 16-bit NHWC x, fp32 weight (cout, cin, k, k), fp32 rows A, C (n, cout) that differ per row, the 16-bit residual (the
    block input where cin == cout), an injected NHWC uint8 keep mask on the marked cases, and ref(dtype, mutant) = the block in front
    of its rounding, NHWC."""
    k, cin, cout, h, w, n, masked, resid = bc
    dt = DTYPES[dtname]
    g = torch.Generator().manual_seed(9000 + 31 * BLOCK_CASES.index(bc) + (dtname == "fp16"))
    x = round16(torch.randn(n, h, w, cin, generator=g, dtype=torch.float64), dt)
    wt = torch.randn(cout, cin, k, k, generator=g) * (1.2 / math.sqrt(cin * min(k, h + 2) * min(k, w + 2)))
    A, C = 1.0 + 0.3 * torch.randn(n, cout, generator=g), 0.5 * torch.randn(n, cout, generator=g)
    keep = (torch.rand(n, h, w, cout, generator=g) >= BLOCK_P).to(torch.uint8) if masked else None
    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(BLOCK_P)))
    nchw = lambda v, dtype: None if v is None else v.to(dtype).permute(0, 3, 1, 2)

    def body(dtype, res):
        y = conv_block(nchw(x, dtype), round16(wt, dt).to(dtype), A.to(dtype), C.to(dtype), (k - 1) // 2, nchw(keep, dtype), scale, nchw(res, dtype))
        return y.permute(0, 2, 3, 1).contiguous()
    res = x if resid == "input" else round16(-0.9375 * body(torch.float64, None), dt) if resid == "cancel" else None

    def ref(dtype=torch.float64, mutant=None):
        if mutant == "residual_after_rounding":
            return round16(body(dtype, None), dt).to(dtype) + res.to(dtype)
        return body(dtype, res)
    return dict(x=x, w=wt, A=A, C=C, keep=keep, res=res, pad=(k - 1) // 2, ref=ref, dt=dt)
