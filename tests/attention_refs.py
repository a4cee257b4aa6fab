"""Float64 references, operand-rounding models, the per-element bound, the case lists and the mutants for the 16-bit Attention core
(csrc/unet_kernels.hip: attention_kernel, flash_attention2_kernel, flash_attention4_kernel behind launch_attention) -- test
infrastructure, no GPU.  tests/test_attention_refs.py checks this file on the CPU, tests/test_gpu_attention_core.py the kernels.

Operand model per kernel family, on the 16-bit input bits as given (qkv (nb, N, 384): q | k | v, 4 heads of 32 channels each):

  flash   (both flash kernels)  q' = round16(fp32(q) * fp32(32^-1/2 * log2 e)) as the Q fragments are built (unet_kernels.hip:1779,
          1795 / 2088, 2108: pack_el16x2 rounds to nearest even), scores q' . k, p = 2^(s - max), l = sum p BEFORE dropout,
          want = scale * (keep * p) @ v / l.
  plain   (attention_kernel)    no rounding of q: scores fp32(q * 32^-1/2) . k (unet_kernels.hip:1569, 1573), natural exponent, P stays fp32.

Bound per output element (HU: half ulp of the output type, HU_P: of the P operand of the second MFMA, 0 for the plain kernel):

    |got - want| <= HU |want| + HU_P AP + F A  [+ 2^-24 U in fp16, flash only]
    A = scale sum_j keep_j p_j |v_j| / l,   U = scale sum_j |v_j| / l

  * got = fl16(o (1 + e)) with o the kernel's fp32 value: the output rounding is HU |want| (to first order);
  * every kept p_j enters the second MFMA as p_j (1 + d_j), |d_j| <= HU_P: the numerator moves by at most HU_P scale sum keep p |v| / l
    = HU_P A.  AP = A wherever the normaliser is summed from the fp32 probabilities (flash_attention2_kernel, every dropout kernel);
  * where the kernel differs from the description above: the DROPOUT-FREE flash_attention4_kernel sums the ROUNDED probabilities on the
    matrix pipe (fa4_rowsum, unet_kernels.hip:1914-1934, called at 1971-1972 and 2012-2013), so numerator and normaliser carry the same
    d_j: got = sum p (1 + d) v / sum p (1 + d), which differs from want by sum p d (v - want) / l -- at most HU_P AP with
    AP = sum_j p_j |v_j - want| / l.  (A constant V column is returned exactly; AP <= A + |want|.)  Nothing else about that kernel
    differs; its dropout instantiations sum the fp32 probabilities (1974-1977);
  * fp16 only: a P below 2^-14 is subnormal, its rounding error absolute (2^-25 at most, on a P scale where the kernel's maximum is at
    least the reference's 1 -- the lazy maximum m never exceeds the true one by more than the first sub-tile's): 2^-24 U covers it and
    the subnormal OUTPUT; the plain kernel keeps P in fp32, so there only the output's own subnormal spacing appears: the first term
    is max(HU |want|, 2^-25) in fp16;
  * F is the fp32 slack: score accumulation, hardware exp2 / exp, the sums.  F_CPU = (N + 64) 2^-24 is what the fp32 torch model is
    held to on the CPU; F_GPU is measured per family on the kernels and fixed here.
"""
import functools

import numpy as np
import torch

from tests import rng_host as R

HEADS, DH = 4, 32
C_PLAIN = np.float32(0.17677669529663687)
C_FLASH = np.float32(np.float32(0.17677669529663687) * np.float32(1.4426950408889634))  # the fp32 product the compiler folds
HU = {"bf16": 2.0 ** -8, "fp16": 2.0 ** -11}
TDTYPE = {"bf16": torch.bfloat16, "fp16": torch.float16}


def family_of(form):
    return "plain" if form.startswith("attention_kernel") else "flash2" if form.startswith("flash_attention2") else "flash4"


def f_cpu(N):
    return (N + 64) * 2.0 ** -24


# fp32 slack of the kernels, measured on an MI355X: four times the worst (|got - want| - HU |want| - HU_P AP) / A
# over every case of this file and every form, rounded up to a power of two.  The worst was attention_kernel's 6.7e-6 (fp16; bf16 4.6e-6);
# on the flash kernels the derived terms alone held on every element (worst value below zero)
F_GPU = dict.fromkeys(("plain", "flash2", "flash4"), 2.0 ** -15)


def round16(x, dtype):
    return x.to(TDTYPE[dtype]).to(x.dtype)


def _split(qkv16):
    nb, N, _ = qkv16.shape
    x = qkv16.float().view(nb, N, 3, HEADS, DH).permute(2, 0, 3, 1, 4)  # (3, nb, h, N, d)
    return x[0], x[1], x[2]


def _merge(o):  # (nb, h, N, d) -> (nb, N, h * 32 + d): "b h (x y) d -> b (h d) x y"
    nb, _, N, _ = o.shape
    return o.permute(0, 2, 1, 3).reshape(nb, N, HEADS * DH)


def reference(qkv16, dtype, form, keep=None, scale=1.0, mutant=None):
    """float64.  qkv16 (nb, N, 384) in the 16-bit type; keep (nb, 4, N, N) bool / uint8 or None; scale of the survivors.
    -> dict(want, A, AP, U), each (nb, N, 128) float64.  `mutant`: one of REFERENCE_MUTANTS."""
    fam = family_of(form)
    q, k, v = _split(qkv16)
    nb, _, N, _ = q.shape
    if mutant == "row_reads_previous_v":
        v = torch.roll(v, 1, 0)
    if fam == "plain":
        qs = (q * float(C_PLAIN) if mutant != "no_score_scale" else q).double()
    else:
        c = float(C_FLASH) if mutant != "no_score_scale" else float(np.float32(1.4426950408889634))
        qs = round16(q * c, dtype).double()
    s = qs @ k.double().transpose(-1, -2)
    mx = s.max(-1, keepdim=True).values
    p = torch.exp(s - mx) if fam == "plain" else torch.exp2(s - mx)
    kp = p if keep is None else p * keep.to(torch.float64)
    l = p.sum(-1, keepdim=True)
    if mutant == "normaliser_after_dropout":
        l = kp.sum(-1, keepdim=True)
    if mutant == "padded_keys_in_normaliser":  # the zero rows that fill the last 64-key tile score 0
        pad0 = torch.exp(-mx) if fam == "plain" else torch.exp2(-mx)
        l = l + ((-N) % 64) * pad0
    vd = v.double()
    want = scale * (kp @ vd) / l
    A = scale * (kp @ vd.abs()) / l
    U = scale * vd.abs().sum(-2, keepdim=True) / l
    AP = A
    if fam == "flash4" and keep is None:  # normaliser of the rounded probabilities: see the module docstring
        AP = torch.empty_like(A)
        for d in range(DH):
            AP[..., d] = (p * (vd[..., None, :, d] - want[..., :, None, d]).abs()).sum(-1) / l[..., 0]
    if mutant == "heads_swapped":
        want = want[:, [1, 0, 3, 2]]
    return dict(want=_merge(want), A=_merge(A), AP=_merge(AP), U=_merge(U.expand_as(A)))


def model_fp32(qkv16, dtype, form, keep=None, scale=1.0):
    """The same model in fp32 torch, P and the output rounded once each where the kernel rounds them -> (nb, N, 128) fp32 holding
    16-bit values."""
    fam = family_of(form)
    q, k, v = _split(qkv16)
    if fam == "plain":
        s = (q * float(C_PLAIN)) @ k.transpose(-1, -2)
        p = torch.exp(s - s.max(-1, keepdim=True).values)
        l = p.sum(-1, keepdim=True)
        kp = p if keep is None else p * keep.float()
        return _merge(round16((kp @ v) * (np.float32(scale) / l), dtype))
    s = round16(q * float(C_FLASH), dtype) @ k.transpose(-1, -2)
    p = torch.exp2(s - s.max(-1, keepdim=True).values)
    p16 = round16(p if keep is None else p * keep.float(), dtype)
    l = (p16 if fam == "flash4" and keep is None else p).sum(-1, keepdim=True)
    return _merge(round16((p16 @ v) * (np.float32(scale) / l), dtype))


def bound(ref, dtype, form, F):
    fam = family_of(form)
    hu = HU[dtype]
    first = hu * ref["want"].abs()
    if dtype == "fp16":
        first = first.clamp_min(2.0 ** -25)
    b = first + F * ref["A"]
    if fam != "plain":
        b = b + hu * ref["AP"]
        if dtype == "fp16":
            b = b + 2.0 ** -24 * ref["U"]
    return b


def worst_ratio(got, ref, dtype, form, F):
    """largest |got - want| / bound over the elements"""
    return float(((got.double() - ref["want"]).abs() / bound(ref, dtype, form, F)).max())


def fp32_excess(got, ref, dtype, form):
    """largest (|got - want| - HU |want| - HU_P AP [- 2^-24 U]) / A: what F has to cover (<= 0: the derived terms alone hold)"""
    rest = (got.double() - ref["want"]).abs() - bound(ref, dtype, form, 0.0)
    a = ref["A"]
    ok = a > 0
    return float((rest[ok] / a[ok]).max()) if bool(ok.any()) else 0.0


# ------------------------------------------------------------------------------------------------ inputs
SCORE_RANGES = ("small", "spread", "low", "high")  # tests/test_gpu_fp16.py test_attention_core_sequence_lengths_and_score_ranges


def core_inputs(nb, N, case, dtype, seed=0):
    """(nb, N, 384) in the 16-bit type.  Every row comes from its own draws, and row r carries the offset 0.25 (r + 1) in V, so a wrong
    row stride or a wrong (row, head) map cannot return the right numbers.  Score ranges: `small` |scores| of a few units (the lazy
    maximum of the fourth form stays 0), `spread` +-90 in the log2 domain, `low` / `high` every score near -+165; `randn`: small."""
    g = torch.Generator().manual_seed(1000 * N + 10 * nb + len(case) + seed)
    x = torch.randn(nb, N, 384, generator=g)
    if case == "spread":
        x[:, :, :256] *= 4.0
    elif case in ("low", "high"):
        x[:, :, :128] = 4.5 + 0.1 * x[:, :, :128]
        x[:, :, 128:256] = (-4.5 if case == "low" else 4.5) + 0.1 * x[:, :, 128:256]
    else:
        assert case in ("small", "randn"), case
    x[:, :, 256:] += 0.25 * (torch.arange(nb, dtype=torch.float32)[:, None, None] + 1.0)
    return x.to(TDTYPE[dtype])


PLAIN, FA2, FA4_4, FA4_8 = "attention_kernel", "flash_attention2_kernel<QB=1>", "flash_attention4_kernel<NW=4>", "flash_attention4_kernel<NW=8>"
# (form, {switch: value}, N)
CORE_FORMS = [(PLAIN, {"DYF_FLASH_ATTN": "0"}, n) for n in (1, 63, 65, 130)] + \
             [(FA2, {"DYF_FLASH_ATTN": "2"}, n) for n in (1, 31, 33, 64, 100, 128, 132, 225)] + \
             [(FA4_4, {}, n) for n in (31, 64, 100, 200, 384, 511)] + [(FA4_4, {"DYF_FLASH_NW": "4"}, 640)] + \
             [(FA4_8, {}, n) for n in (512, 577, 768)]
CORE_ROWS = [(3, c) for c in SCORE_RANGES] + [(2, "spread"), (4, "spread")]
# quad dropout: the form a launch with engine dropout takes at N tokens
QUAD_FORMS = [(PLAIN, {"DYF_FLASH_ATTN": "0"}, n) for n in (1, 33, 65)] + \
             [(FA2, {"DYF_FLASH_ATTN": "2"}, n) for n in (2, 31, 33, 130, 225)] + \
             [(FA2, {"DYF_FLASH_ATTN": "2"}, n) for n in (132, 192)] + [(FA2, {"DYF_FLASH_ATTN": "2"}, 640)] + \
             [(FA4_4, {}, n) for n in (128, 384)] + [(FA4_8, {}, n) for n in (512, 768)]
QUAD_SCORE_FORMS = [c for c in QUAD_FORMS if c[2] > 2]
QUAD_ROWS = [(3, 5, 0.7), (2, 0, 0.1)]  # (nb, row offset, p)
QUAD_SCORES = ("randn", "spread")
MASK_FORMS = [(FA2, {"DYF_FLASH_ATTN": "2"}, n) for n in (31, 132, 225)] + [(PLAIN, {"DYF_FLASH_ATTN": "0"}, n) for n in (33, 65)]
MASK_P, MASK_NB = 0.3, 3


def case_id(form, switch, N):
    return form.replace("_kernel", "").replace("<", "-").replace(">", "").replace("=", "") + ("-nw4" if switch.get("DYF_FLASH_NW") else "") + f"-N{N}"


def quad_seed(N):
    return 20261021 + N


def bernoulli_mask(nb, N, p, seed):
    """(nb, 4, N, N) uint8, every row its own draws"""
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(nb, HEADS, N, N, generator=g) >= p).to(torch.uint8)


# ------------------------------------------------------------------------------------------------ the quad stream and its mutants
QUAD_MUTANTS = ("no_head_fold", "element_hNi", "bytes_from_the_top")


def quad_keep_row(N, p, seed, fwd, site, grow, mutant=None):
    """tests/rng_host.py attn_quad_keep restated with the switches of QUAD_MUTANTS (mutant None: equal to it, checked on the CPU)."""
    k = R.keep_threshold8(p)
    r0, r1 = R.row_key(seed, fwd, grow)
    s0, s1 = R.layer_salt(site)
    k0, k1 = r0 ^ s0, (r1 + s1) & R.M32
    u = np.uint64
    ij = np.arange(N, dtype=np.uint64)[:, None] * u(N) + np.arange(N, dtype=np.uint64)[None, :]
    keep = np.empty((HEADS, N, N), dtype=bool)
    for h in range(HEADS):
        kh = k0 if mutant == "no_head_fold" else R.fmix32((k0 + u(h + 1) * u(0x9E3779B9)) & R.M32)
        e = ((ij + u(h) * u(N) * u(N)) if mutant == "element_hNi" else ij) & R.M32
        byte = (u(3) - (e & u(3))) if mutant == "bytes_from_the_top" else (e & u(3))
        keep[h] = ((R.pair_word(e >> u(2), kh, k1) >> (u(8) * byte)) & u(0xFF)) < u(k)
    return keep


@functools.lru_cache(maxsize=64)
def quad_keep(nb, N, p, seed, grow, mutant=None):
    """(keep (nb, 4, N, N) bool tensor, scale) of a launch of nb rows at row offset `grow`: forward 0, site 0 (dyf_op_attention_dropout)"""
    rows = [R.attn_quad_keep(N, p, seed, 0, 0, grow + r)[0] if mutant is None else quad_keep_row(N, p, seed, 0, 0, grow + r, mutant)
            for r in range(nb)]
    return torch.from_numpy(np.stack(rows)), 256.0 / R.keep_threshold8(p)


REFERENCE_MUTANTS = ("normaliser_after_dropout", "row_reads_previous_v", "no_score_scale", "padded_keys_in_normaliser", "heads_swapped")
