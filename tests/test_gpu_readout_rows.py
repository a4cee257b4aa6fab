"""-m gpu: the two bodies of the readout's DMA form (csrc/kernels.hip) compute the same words.

readout_dma_kernel gathers 16 taps per output pixel (the gather body); readout_dma_rows_kernel stages every decoder row once per band
of output rows, contracts each decoder pixel once per kernel row and blends from LDS (the rows body, the default where its LDS plan
fits: stored rows of up to 128 columns).  Same MFMA per dot product, same fmaf chain in the same tap order: the outputs are compared
as int32 words, so a last bit, a signed zero or a NaN payload counts.  Every case goes through the op seam (HipEngine.op_sample
"readout") with the tap tables; DYF_READOUT_ROWS = 1 | 0 picks the body, and each run asserts the marker its body notes
(readout_dma_kernel+rows / +gather) beside the form's own single note.  What the streaming order rests on:
tests/test_readout_rows_premise.py.
"""
import pytest
import torch

import dyffusion_amd as D
from tests import sample_op_refs as S
from tests.gpu_common import DEV, build_dyffusion, seeded_pair

pytestmark = pytest.mark.gpu

NB = 3
# id -> ((ih, iw), (oh, ow)), compact, nearest, cout, body under the default.  With NB = 3 a band is 8 output rows (fewer when ow > 128).
CASES = {
    "compact-8cols": (((6, 16), (5, 3)), 1, 0, 3, "rows"),        # 8 stored columns: less than one 16-pixel group
    "compact-ns-like": (((32, 32), (27, 5)), 1, 0, 1, "rows"),    # the NS-like 2.3x / 6x reduction; 4 bands, the last of 3 rows
    "dense-ragged-group": (((40, 24), (33, 9)), 0, 0, 2, "rows"),  # 24 columns: a ragged second group; 5 bands
    "up-6x": (((8, 8), (48, 48)), 0, 0, 4, "rows"),               # many output rows per decoder row; 384 pixels per band
    "one-pixel": (((1, 1), (3, 3)), 0, 0, 3, "rows"),             # every tap at a border
    "ow70": (((6, 40), (5, 70)), 0, 0, 2, "rows"),                # ow > 64: a row of the band spans two waves
    "compact-nearest": (((32, 32), (27, 5)), 1, 1, 4, "rows"),    # nearest: taps of weight 0 with valid offsets
    "dense-nearest": (((6, 16), (5, 3)), 0, 1, 1, "rows"),
    "three-bands": (((20, 12), (21, 7)), 0, 0, 3, "rows"),        # bands of 8, 8 and 5 rows
    "widest-128": (((2, 128), (3, 20)), 0, 0, 2, "rows"),         # the widest stored row of the rows body's LDS plan (80 KB)
    "wider-129": (((2, 129), (3, 20)), 0, 0, 3, "gather"),        # one wider: the gather body under the default too
}


@pytest.fixture(scope="module", params=["bf16", "fp16"])
def eng(request):
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False, dtype=request.param)
    yield e
    e.close()


def inputs(eng, geom, compact, nearest, co):
    (ih, iw), (oh, ow) = geom
    g = torch.Generator().manual_seed(1000 * ih + 10 * ow + co)
    x = (1.5 * torch.randn(NB, ih, iw, 64, generator=g)).to(eng.torch_dtype)
    w = (1.5 / 16 * torch.randn(64, co, 4, 4, generator=g)).to(eng.torch_dtype).float()
    b = 0.5 * torch.randn(co, generator=g)
    kw = dict(out_hw=(oh, ow), nearest=bool(nearest))
    if compact:
        used, cmap = S.readout_columns(iw, ow, bool(nearest))
        x, kw["col_map"] = x[:, :, used].contiguous(), cmap.to(DEV)
    return x, [w, b], kw


def run_body(eng, form_switch, rows, x, params, kw):
    """-> (output words int32 on the host, the forms noted)"""
    form_switch.setenv("DYF_READOUT_ROWS", "1" if rows else "0")
    eng.form_log(True)
    try:
        y = eng.op_sample("readout", [x.to(DEV)], params, **kw)
        forms = eng.form_log_read()
    finally:
        eng.form_log(False)
    assert y.dtype == torch.float32
    return y.cpu().view(torch.int32), forms


def both_bodies(eng, form_switch, x, params, kw, default_body, tag):
    got, forms = run_body(eng, form_switch, True, x, params, kw)
    want, forms0 = run_body(eng, form_switch, False, x, params, kw)
    nb = x.shape[0]
    for f, body in ((forms, default_body), (forms0, "gather")):
        other = "gather" if body == "rows" else "rows"
        assert f.get("readout_dma_kernel") == {nb: 1} and f.get(f"readout_dma_kernel+{body}") == {nb: 1}, (tag, f)
        assert f"readout_dma_kernel+{other}" not in f and "readout_mfma_kernel" not in f, (tag, f)
    diff = int((got != want).sum())
    print(f"readout bodies {tag}: {diff} of {want.numel()} words differ ({default_body} vs gather)")
    assert torch.equal(got, want), tag
    return got


@pytest.mark.parametrize("cid", list(CASES))
def test_rows_body_is_bitwise_the_gather_body(eng, cid, form_switch):
    geom, compact, nearest, co, body = CASES[cid]
    x, params, kw = inputs(eng, geom, compact, nearest, co)
    got = both_bodies(eng, form_switch, x, params, kw, body, f"{cid}-{eng.dtype}")
    assert bool(torch.isfinite(got.view(torch.float32)).all())


@pytest.mark.parametrize("cid", ["compact-ns-like", "compact-nearest"])
def test_non_finite_pixels_reach_the_same_outputs_through_every_tap(eng, cid, form_switch):
    """One stored pixel +inf, one NaN (and a single NaN channel): a tap with valid offsets is blended whatever its weight --
    0 * inf is NaN in both bodies -- and the payloads agree."""
    geom, compact, nearest, co, body = CASES[cid]
    x, params, kw = inputs(eng, geom, compact, nearest, co)
    x[1, 10, 3, :] = float("inf")
    x[2, 20, 1, :] = float("nan")
    x[0, 31, x.shape[2] - 1, 5] = float("nan")
    got = both_bodies(eng, form_switch, x, params, kw, body, f"{cid}-nonfinite-{eng.dtype}").view(torch.float32)
    bad = ~torch.isfinite(got)
    assert bool(bad[1].any()) and bool(bad[2].any()) and bool(bad[0].any()) and not bool(bad.all())


def test_rollout_fields_are_bitwise_the_same_under_both_bodies(form_switch):
    """The 23x11 @ 64^2, h = 4 pair of tests/test_gpu_sampler.py with 3 rows, a captured graph and MC dropout on: the fields of the
    two bodies are equal word for word, and the replay of the graph equals the call that captured it."""
    hp = dict(timesteps=4, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only",
              sampling_type="cold", refine_intermediate_predictions=True, enable_interpolator_dropout=True,
              num_input_channels=3)
    mk = dict(dim=64, upsample_dims=[64, 64], outer_sample_mode="bilinear", with_time_emb=True, dropout=0.15)
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(2)
    x0, c = torch.randn(NB, 3, 23, 11, generator=g).to(DEV), torch.rand(NB, 2, 23, 11, generator=g).to(DEV)
    fields = {}
    for rows in (1, 0):
        form_switch.setenv("DYF_READOUT_ROWS", str(rows))
        m = build_dyffusion(PF, PI, mk, 3, 2, hp, max_batch=NB, use_graph=True)
        m.seed(77)
        m._ensure_engine((23, 11), NB)
        m._engine.form_log(True)
        try:
            first = m.sample(x0, static_condition=c)
            forms = m._engine.form_log_read()
        finally:
            m._engine.form_log(False)
        body, other = ("rows", "gather") if rows else ("gather", "rows")
        assert f"readout_dma_kernel+{body}" in forms and f"readout_dma_kernel+{other}" not in forms, forms
        assert forms[f"readout_dma_kernel+{body}"] == forms["readout_dma_kernel"], forms
        m.seed(77)
        again = m.sample(x0, static_condition=c)
        assert all(torch.equal(first[k].view(torch.int32), again[k].view(torch.int32)) for k in first), rows
        fields[rows] = {k: v.cpu().view(torch.int32) for k, v in first.items()}
        m._engine.close()
    assert sorted(fields[0]) == sorted(fields[1]) and len(fields[1]) > 0
    for k in fields[1]:
        assert torch.equal(fields[1][k], fields[0][k]), k
