"""-m gpu: the fused-stem launcher at channel pitch 8 and writing only the DISTINCT rows of a paired launch (StemArgs::out_pitch,
StemArgs::distinct_only; HipEngine.op_sample "stem16" with pitch=8 / pair_once=True), one launch at a time against float64 torch:
reference tests/sample_op_refs.stem16 sliced to 8 channels (no bias slot at pitch 8) and to the distinct rows, bound that file's
`excess <= floor`.

Geometries: the two where the row-block form's branches change (tests/sample_op_refs.py net_specs) -- sources 5 x 40 -> 8 x 256 (one
lane per pixel, a wave stores whole 1 KB runs) and 5 x 40 -> 9 x 254 (the general path, a second row block).  Channels: 8 from one
and from two sources (the interpolator: every channel used) and 5 from two (the forecaster: three pad channels).  nb = 4 output rows
over src_rows in {0, 2}, pair_once on and off, the row-block form and the per-pixel form (DYF_STEM16_ROWS=0), bf16 and fp16, pitch 8 and
-- for the distinct rows -- 16.  Asserted: the bound, the zero border, zero pad channels, the bias slot (1 at pitch 16, absent at 8),
that with pair_once exactly src_rows rows are written and equal the first src_rows rows of the full output bit for bit, and the noted
form with the rows of the forward (nb, not the rows written).
"""
import pytest
import torch

import dyffusion_amd as D
from tests import sample_op_refs as S
from tests.gpu_common import DEV

pytestmark = pytest.mark.gpu
NB = 4
GEOMS = {"1lane-8x256": ((5, 40), (8, 256)), "general-9x254": ((5, 40), (9, 254))}
CHANNELS = {"c8": (8,), "c5+3": (5, 3), "c3+2": (3, 2)}


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def eng(request):
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False, dtype=request.param)
    yield e
    e.close()


def sources(ch, hw, rows):
    g = S._gen(77, sum(ch), len(ch), hw[0], hw[1], rows)
    return [S._rn(g, rows, c, hw[0], hw[1], scale=1.5).float() for c in ch]


def reference(srcs, uhw, src_rows, pitch, mutant=None):
    """float64 (NB, uh + 2, uw + 2, pitch): at pitch 8 the first 8 channels of the 16-channel tensor without its bias slot."""
    if pitch == 16:
        return S.stem16(srcs, uhw[0], uhw[1], False, src_rows, NB, mutant)
    if mutant is None:
        return S.stem16(srcs, uhw[0], uhw[1], False, src_rows, NB, "no_bias_slot")[..., :8]
    assert mutant == "src_rows_ignored"  # (S.stem16 takes one mutant: the bias slot of the mutant is cleared here)
    out = S.stem16(srcs, uhw[0], uhw[1], False, src_rows, NB, mutant)
    out[..., sum(s.shape[1] for s in srcs)] = 0
    return out[..., :8]


def launch(eng, srcs, uhw, src_rows, pair_once, pitch):
    eng.form_log(True)
    try:
        y = eng.op_sample("stem16", [s.to(DEV) for s in srcs], out_hw=uhw, nb=NB, src_rows=src_rows, pair_once=pair_once, pitch=pitch)
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    return y.cpu(), forms


@pytest.mark.parametrize("pitch", [8, 16])
@pytest.mark.parametrize("per_pixel", [0, 1], ids=["rows", "per-pixel"])
@pytest.mark.parametrize("src_rows", [0, 2])
@pytest.mark.parametrize("ch", list(CHANNELS))
@pytest.mark.parametrize("geom", list(GEOMS))
def test_stem16_pitch_and_distinct_rows(eng, form_switch, geom, ch, src_rows, per_pixel, pitch):
    hw, uhw = GEOMS[geom]
    ch = CHANNELS[ch]
    if per_pixel:
        form_switch.setenv("DYF_STEM16_ROWS", "0")
    form = "stem16_kernel" if per_pixel else "stem16_rows_kernel"
    srcs = sources(ch, hw, src_rows if src_rows else NB)
    cin = sum(ch)
    ref = reference([s.double() for s in srcs], uhw, src_rows, pitch)
    full, forms = launch(eng, srcs, uhw, src_rows, False, pitch)
    assert tuple(full.shape) == (NB, uhw[0] + 2, uhw[1] + 2, pitch) and forms[form] == {NB: 1}, forms
    outs = [("full", full, ref)]
    if src_rows:
        once, forms = launch(eng, srcs, uhw, src_rows, True, pitch)
        assert forms[form] == {NB: 1}, forms                                   # the rows of the forward the launch serves
        assert tuple(once.shape) == (src_rows, uhw[0] + 2, uhw[1] + 2, pitch)  # exactly the distinct rows
        assert torch.equal(once.view(torch.int16), full[:src_rows].view(torch.int16))
        outs.append(("distinct rows", once, ref[:src_rows]))
    else:
        with pytest.raises(ValueError):
            eng.op_sample("stem16", [s.to(DEV) for s in srcs], out_hw=uhw, nb=NB, pair_once=True, pitch=pitch)
    if pitch == 8:  # ... and the 8 channels are the first 8 of the 16-channel tensor, bit for bit, but for its bias slot
        wide, _ = launch(eng, srcs, uhw, src_rows, False, 16)
        keep = [c for c in range(8) if c != cin]
        assert torch.equal(full[..., keep].view(torch.int16), wide[..., keep].view(torch.int16))
    for tag, got, want in outs:
        assert bool(torch.isfinite(got.float()).all())
        excess, floor = S.excess_floor(got, want, eng.torch_dtype)
        print(f"stem16 pitch {pitch} {geom} ch {ch} src_rows {src_rows} {form} {tag}: excess {excess:.3e}, floor {floor:.3e}")
        assert excess <= floor
        g = got.float()
        border = torch.cat([g[:, 0].flatten(), g[:, -1].flatten(), g[:, :, 0].flatten(), g[:, :, -1].flatten()])
        assert float(border.abs().max()) == 0.0
        pad0 = cin if pitch == 8 else cin + 1                                  # pad channels (behind the bias slot at pitch 16)
        if pad0 < pitch:
            assert float(g[..., pad0:].abs().max()) == 0.0
        if pitch == 16:
            assert bool((g[:, 1:-1, 1:-1, cin] == 1).all())


def test_pitch_8_takes_at_most_8_channels(eng):
    with pytest.raises(ValueError):
        eng.op_sample("stem16", [torch.zeros(2, 9, 5, 40, device=DEV)], out_hw=(8, 256), pitch=8)
    with pytest.raises(ValueError):
        eng.op_sample("stem16", [torch.zeros(2, 8, 5, 40, device=DEV)], out_hw=(8, 256), pitch=12)
