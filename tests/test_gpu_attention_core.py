"""-m gpu: the 16-bit Attention core (csrc/unet_kernels.hip launch_attention), kernel form by kernel form, per output element against
the float64 reference and bound of tests/attention_refs.py -- and the masks of its default ("quad") probability dropout bit for bit
against tests/rng_host.py attn_quad_keep.

  (a) dropout-free: attention_kernel, flash_attention2_kernel<FA_DROP_OFF>, flash_attention4_kernel<FA_DROP_OFF, 4 / 8>; three rows
      with four score ranges, and two / four rows (8 / 16 (row, head) pairs: the XCD block remap of the flash kernels is taken);
  (b) quad masks recovered from the outputs, zero differing bits allowed, on every dropout instantiation and both mask paths of
      flash_attention2_kernel<FA_DROP_QUAD>; survivor values;
  (c) quad dropout on real scores against the reference on host-rebuilt masks;
  (d) injected masks (DropSpec mode 2) through dyf_op_attention_mask.

Every test pins the kernel form with form_switch and reads the form it got back from the form log.  The fp32 slack F of the bound is
tests/attention_refs.py F_GPU; every test prints what it needed of it, and the module prints the worst per form at the end."""
import numpy as np
import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from tests import attention_refs as AR
from tests.gpu_common import DEV

pytestmark = pytest.mark.gpu
DTYPES = ["fp16", "bf16"]
WORST = {}  # (form, dtype) -> [largest fp32 excess / A, largest |err| / bound]


@pytest.fixture(scope="module")
def engines():
    cfg = D.resnet_net_config(in_channels=2, cond_channels=0, out_channels=1, dim=64, dim_mults=(1, 2))
    made = {}

    def get(dtype):
        if dtype not in made:
            made[dtype] = D.HipEngine(cfg, cfg, 16, 16, max_batch=2, use_graph=False, dtype=dtype)
            assert made[dtype].attention_dropout == "fast"
        return made[dtype]

    yield get
    for e in made.values():
        e.close()
    for (form, dtype), (ex, ratio) in sorted(WORST.items()):
        note = f"2^{np.log2(ex):.1f}" if ex > 0 else "the derived terms alone hold"
        print(f"\n[attention core] {form} {dtype}: worst fp32 excess / A = {ex:.3e} ({note}), worst |err| / bound = {ratio:.3f}", end="")


def _launch(eng, form_switch, form, switch, nb, fn, launches=1):
    """run fn() under the pinned form; the form log must hold exactly `launches` launches of `form` with nb rows"""
    for k, v in switch.items():
        form_switch.setenv(k, v)
    eng.form_log(True)
    try:
        out = fn()
        log = eng.form_log_read()
    finally:
        eng.form_log(False)
    assert list(log) == [form] and log[form] == {nb: launches}, log
    return out


def _check(got, ref, dtype, form, what):
    got = got.float().cpu()
    assert bool(torch.isfinite(got).all()), what
    ex, ratio = AR.fp32_excess(got, ref, dtype, form), AR.worst_ratio(got, ref, dtype, form, AR.F_GPU[AR.family_of(form)])
    w = WORST.setdefault((form, dtype), [-1.0, 0.0])
    w[0], w[1] = max(w[0], ex), max(w[1], ratio)
    print(f"{form} {dtype} {what}: fp32 excess / A = {ex:.3e}, worst |err| / bound = {ratio:.3f}")
    assert ratio <= 1.0, (what, ratio)


# ------------------------------------------------------------------------------------------------ (a) dropout-free core
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("nb,case", AR.CORE_ROWS, ids=[f"nb{nb}-{c}" for nb, c in AR.CORE_ROWS])
@pytest.mark.parametrize("form,switch,N", AR.CORE_FORMS, ids=[AR.case_id(*c) for c in AR.CORE_FORMS])
def test_dropout_free_core_per_element(engines, form_switch, form, switch, N, nb, case, dtype):
    eng = engines(dtype)
    qkv = AR.core_inputs(nb, N, case, dtype)
    got = _launch(eng, form_switch, form, switch, nb, lambda: eng.op_attention(qkv.to(DEV)))
    _check(got, AR.reference(qkv, dtype, form), dtype, form, f"N={N} nb={nb} {case}")


# ------------------------------------------------------------------------------------------------ (b) quad masks, bit for bit
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,switch,N", AR.QUAD_FORMS, ids=[AR.case_id(*c) for c in AR.QUAD_FORMS])
def test_quad_masks_equal_the_host_restatement_bit_for_bit(engines, form_switch, form, switch, N, dtype):
    """q = k = 0 makes every probability 1 / N; V one-hot over a block of 32 keys makes out[i, h * 32 + c] = keep(i, j0 + c) * scale / N:
    one launch per key block (the generator re-seeded before each, so every launch draws forward 0) recovers the engine's whole keep
    tensor (nb, 4, N, N).  nb = 3 rows at row offset 5.  Survivors are (1 / N) * 256 / k to half an ulp of the output type -- which at
    p = 0.7 is not 1 / (1 - p): 256 / 76 = 3.368 against 3.333, 1 % apart."""
    eng = engines(dtype)
    nb, grow, seed, hu = 3, 5, AR.quad_seed(N), AR.HU[dtype]
    eng.set_row_offset(grow)
    try:
        for p in (0.1, 0.7):
            def run():
                keep, vals = torch.zeros(nb, 4, N, N, dtype=torch.bool), []
                for j0 in range(0, N, 32):
                    w = min(32, N - j0)
                    qkv = torch.zeros(nb, N, 384, dtype=eng.torch_dtype)
                    for h in range(4):
                        qkv[:, torch.arange(j0, j0 + w), 256 + h * 32 + torch.arange(w)] = 1.0
                    eng.seed(seed)
                    out = eng.op_attention(qkv.to(DEV), p_drop=p).float().cpu().reshape(nb, N, 4, 32)[..., :w]  # (nb, i, h, c)
                    keep[:, :, :, j0:j0 + w] = (out != 0).permute(0, 2, 1, 3)
                    vals.append(out[out != 0])
                return keep, torch.cat(vals).double()
            keep, vals = _launch(eng, form_switch, form, switch, nb, run, launches=(N + 31) // 32)
            want, scale = AR.quad_keep(nb, N, p, seed, grow)
            wrong = int((keep != want).sum())
            print(f"{form} {dtype} N={N} p={p}: kept {float(keep.float().mean()):.4f}, bits differing from the host restatement: {wrong}")
            assert wrong == 0
            expect = (1.0 / N) * scale
            worst = float(((vals - expect).abs() / expect).max()) if vals.numel() else 0.0
            print(f"    survivors: worst relative distance from (1/N) * 256 / k = {worst:.3e} (half ulp {hu:.3e})")
            assert worst <= hu + 1e-6  # (1e-6: the fp32 arithmetic before the output is rounded)
            if p == 0.7:  # ... and this tells 256 / k from 1 / (1 - p): the two are more than two such intervals apart
                assert abs(1.0 / (1.0 - p) - scale) / scale > 2 * (hu + 1e-6)
                if vals.numel():
                    assert float(((vals - (1.0 / N) / (1.0 - p)).abs() / expect).min()) > hu + 1e-6
    finally:
        eng.set_row_offset(0)


# ------------------------------------------------------------------------------------------------ (c) quad dropout, real scores
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("score", AR.QUAD_SCORES)
@pytest.mark.parametrize("nb,grow,p", AR.QUAD_ROWS, ids=[f"nb{nb}-row{g}-p{p}" for nb, g, p in AR.QUAD_ROWS])
@pytest.mark.parametrize("form,switch,N", AR.QUAD_SCORE_FORMS, ids=[AR.case_id(*c) for c in AR.QUAD_SCORE_FORMS])
def test_quad_dropout_on_real_scores_per_element(engines, form_switch, form, switch, N, nb, grow, p, score, dtype):
    eng = engines(dtype)
    qkv = AR.core_inputs(nb, N, score, dtype)
    keep, scale = AR.quad_keep(nb, N, p, AR.quad_seed(N), grow)
    eng.set_row_offset(grow)
    eng.seed(AR.quad_seed(N))
    try:
        got = _launch(eng, form_switch, form, switch, nb, lambda: eng.op_attention(qkv.to(DEV), p_drop=p))
    finally:
        eng.set_row_offset(0)
    _check(got, AR.reference(qkv, dtype, form, keep, scale), dtype, form, f"N={N} nb={nb} row {grow} p={p} {score}")


# ------------------------------------------------------------------------------------------------ (d) injected masks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form,switch,N", AR.MASK_FORMS, ids=[AR.case_id(*c) for c in AR.MASK_FORMS])
def test_injected_masks_per_element(engines, form_switch, form, switch, N, dtype):
    """Every row its own Bernoulli mask at p = 0.3; then a mask of all ones, which returns 1 / 0.7 times the dropout-free output: both
    are the 16-bit roundings of fp32 values that agree to the fp32 slack, so they differ by at most the sum of their two bounds."""
    eng = engines(dtype)
    nb, p, scale = AR.MASK_NB, AR.MASK_P, 1.0 / (1.0 - AR.MASK_P)
    qkv = AR.core_inputs(nb, N, "randn", dtype)
    keep = AR.bernoulli_mask(nb, N, p, N)
    assert not torch.equal(keep[0], keep[1]) and not torch.equal(keep[1], keep[2])
    got = _launch(eng, form_switch, form, switch, nb, lambda: eng.op_attention(qkv.to(DEV), p_drop=p, mask=keep.to(DEV)))
    _check(got, AR.reference(qkv, dtype, form, keep, scale), dtype, form, f"N={N} injected Bernoulli masks")
    ones = torch.ones_like(keep)
    got1 = _launch(eng, form_switch, form, switch, nb, lambda: eng.op_attention(qkv.to(DEV), p_drop=p, mask=ones.to(DEV)))
    ref1 = AR.reference(qkv, dtype, form, ones, scale)
    _check(got1, ref1, dtype, form, f"N={N} mask of ones")
    free = _launch(eng, form_switch, form, switch, nb, lambda: eng.op_attention(qkv.to(DEV))).double().cpu()
    F = AR.F_GPU[AR.family_of(form)]
    r = float(((got1.double().cpu() - scale * free).abs() / (2.0 * AR.bound(ref1, dtype, form, F))).max())
    print(f"{form} {dtype} N={N}: mask of ones against the dropout-free output / 0.7: {r:.3f} of the two bounds")
    assert r <= 1.0


@pytest.mark.parametrize("dtype", DTYPES)
def test_masks_take_the_second_form_and_the_seam_refuses_what_it_cannot_express(engines, form_switch, dtype):
    eng = engines(dtype)
    nb, N, p = 2, 128, AR.MASK_P
    qkv = AR.core_inputs(nb, N, "randn", dtype)
    keep = AR.bernoulli_mask(nb, N, p, 7)
    # the fourth form does not take masks: N = 128 runs flash_attention4_kernel<NW=4> without a mask and with engine dropout
    got = _launch(eng, form_switch, AR.FA2, {"DYF_FLASH_ATTN": "4"}, nb, lambda: eng.op_attention(qkv.to(DEV), p_drop=p, mask=keep.to(DEV)))
    _check(got, AR.reference(qkv, dtype, AR.FA2, keep, 1.0 / (1.0 - p)), dtype, AR.FA2, f"N={N} injected masks under DYF_FLASH_ATTN=4")
    _launch(eng, form_switch, AR.FA4_4, {"DYF_FLASH_ATTN": "4"}, nb, lambda: eng.op_attention(qkv.to(DEV), p_drop=p))
    lib, x, m = eng._lib, qkv.to(DEV), keep.to(DEV)
    y = torch.empty(nb, N, 128, dtype=eng.torch_dtype, device=DEV)
    eng.form_log(True)
    try:
        assert lib.dyf_op_attention_mask(eng._h, x.data_ptr(), nb, N, p, None, y.data_ptr(), None) == L.DYF_ERR_INVALID_ARGUMENT
        for bad_p in (0.0, 1.0, -0.1):
            assert lib.dyf_op_attention_mask(eng._h, x.data_ptr(), nb, N, bad_p, m.data_ptr(), y.data_ptr(), None) == L.DYF_ERR_INVALID_ARGUMENT
        assert lib.dyf_op_attention_mask(eng._h, x.data_ptr(), 0, N, p, m.data_ptr(), y.data_ptr(), None) == L.DYF_ERR_INVALID_ARGUMENT
        # 4 rows x 4 heads x 16384^2 bytes: refused before anything is launched (the pointers are never read)
        assert lib.dyf_op_attention_mask(eng._h, x.data_ptr(), 4, 16384, p, m.data_ptr(), y.data_ptr(), None) == L.DYF_ERR_UNSUPPORTED
        assert eng.form_log_read() == {}  # nothing was launched
    finally:
        eng.form_log(False)
