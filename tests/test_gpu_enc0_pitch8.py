"""-m gpu: the encoder entry of the 16-bit sampling path on the 8-channel stem, and paired launches on the distinct stem rows.

(1) enc0 on the 8-channel stem (csrc/conv_enc0_stem.hip, P8: 8 pixel k-steps and a ninth that carries init_conv's bias as the 0/1
"tap inside the image" indicator): NB = 8 at 256 x 256 -- the smallest batch the persistent kernel takes -- forecaster (5 input
channels) and interpolator (8), one forward each, MC dropout off and drawn by the engine (masks rebuilt on the host,
tests/rng_host.EngineDropout).  The enc0 block output of rows 0 and 7 against the oracle's `enc0` tap under the rule of
test_gpu_bench_forms.test_nb160_forward_block_outputs_match_the_oracle_taps, rel-RMS <= 1.25 x the oracle's own bf16 storage model
+ 2e-4, evaluated SEPARATELY on the border ring (oy or ox in {0, 127}: where the bias indicator is not all ones) and on the interior.

(2) A PAIRED interpolator launch (2 nb rows over nb distinct inputs: csrc/engine.hip interp2 and the batched refinement) with the
stem written once per distinct row and enc0 run once per distinct tile (StemArgs::distinct_only, ConvArgs::src0_rows): the K pass is
shared, every copy keeps its own FiLM row, dropout row key and output tile, so the launch must give BIT FOR BIT what
DYF_STEM_PAIR_ONCE=0 -- every row of the stem tensor written and read -- gives.  A 3-timestep cold-sampling rollout with MC dropout at
NB = 8 has paired launches of 16 rows (both interpolations of a step, and the two refinement forwards, which are the rollout's last
launch: its enc0 output is what read_block_output sees afterwards).  A 4-row call on the same engine has 2048 distinct row segments
per launch and stays on the full 16-channel stem tensor: bitwise equal with both switches at their old and at their new values.
"""
import pytest
import torch

from oracle import nets
from tests import rng_host as R
from tests.gpu_common import DEV, build_dyffusion, cached, mirror_from_params, seeded_pair
from tests.helpers import rel_rms

pytestmark = pytest.mark.gpu
NB = 8
MK = dict(dim=64, upsample_dims=[256, 256], outer_sample_mode="bilinear", with_time_emb=True, dropout=0.15)
HP = dict(timesteps=3, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only", sampling_type="cold",
          refine_intermediate_predictions=True, enable_interpolator_dropout=True)
SEED = 20261020


def _inputs(nb):
    g = torch.Generator().manual_seed(808)
    return torch.randn(nb, 3, 23, 11, generator=g), torch.rand(nb, 2, 23, 11, generator=g)


def _rollout(form_switch, pair_once, use_graph, nb, pitch):
    """-> (fields, enc0 output of the last interpolator launch over 2 nb rows, form log) of one rollout on a fresh engine for NB rows."""
    form_switch.setenv("DYF_STEM_PAIR_ONCE", pair_once)
    form_switch.setenv("DYF_STEM_PITCH", pitch)
    PF, PI = seeded_pair(64, 3, 2)
    x0, c = _inputs(nb)
    m = build_dyffusion(PF, PI, MK, 3, 2, HP, max_batch=NB, use_graph=use_graph)
    m.seed(SEED)
    m._ensure_engine((23, 11), NB)
    eng = m._engine
    eng.form_log(True)
    out = {k: v.clone() for k, v in m.sample(x0.to(DEV), static_condition=c.to(DEV)).items()}
    forms = eng.form_log_read()
    eng.form_log(False)
    if use_graph:  # the replay of the captured rollout draws the next forwards' masks: only that it runs and stays finite
        again = m.sample(x0.to(DEV), static_condition=c.to(DEV))
        assert all(bool(torch.isfinite(v).all()) for v in again.values())
    enc0 = eng.read_block_output(1, 0, 2 * nb).cpu()
    eng.close()
    return {k: v.cpu() for k, v in out.items()}, enc0, forms


@pytest.fixture(scope="module")
def full_stem():
    """The rollouts with every stem row written (DYF_STEM_PAIR_ONCE=0), computed once: {(use_graph, nb, pitch): (fields, enc0, forms)}."""
    return {}


def _reference(full_stem, form_switch, use_graph, nb, pitch):
    if (use_graph, nb, pitch) not in full_stem:
        full_stem[(use_graph, nb, pitch)] = _rollout(form_switch, 0, use_graph, nb, pitch)
    return full_stem[(use_graph, nb, pitch)]


@pytest.mark.parametrize("pitch", [16, 8])  # (at equal pitch: the two pitches sum enc0 in different orders)
@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_paired_launch_on_the_distinct_stem_rows_is_bitwise_the_full_stem_launch(full_stem, form_switch, use_graph, pitch):
    want, want_enc0, forms0 = _reference(full_stem, form_switch, use_graph, NB, pitch)
    got, got_enc0, forms1 = _rollout(form_switch, 1, use_graph, NB, pitch)
    print("forms, pair once:", {k: sorted(v) for k, v in forms1.items() if "stem" in k})
    for forms in (forms0, forms1):  # the same forms, noted with the rows of the forward they serve
        assert 2 * NB in forms["stem16_rows_kernel"] and NB in forms["stem16_rows_kernel"], forms.get("stem16_rows_kernel")
        assert 2 * NB in forms["conv_enc0_stem_kernel"] and NB in forms["conv_enc0_stem_kernel"], forms.get("conv_enc0_stem_kernel")
    assert forms0 == forms1
    assert sorted(got) == sorted(want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()), k
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got_enc0, want_enc0)
    # the two halves of the launch really had FiLM rows and dropout masks of their own
    assert not torch.equal(got_enc0[:NB], got_enc0[NB:])
    diff = (got_enc0[:NB] != got_enc0[NB:]).float().mean()
    print(f"enc0 of the last paired launch: {float(diff):.3f} of the elements differ between the halves")
    assert float(diff) > 0.5


def test_a_four_row_call_on_the_same_engine_keeps_the_full_stem_tensor(form_switch):
    want, want_enc0, forms0 = _rollout(form_switch, 0, False, 4, pitch=16)  # both switches at their old values
    got, got_enc0, forms1 = _rollout(form_switch, 1, False, 4, pitch=8)
    assert forms0 == forms1
    assert "conv_enc0_stem_kernel" in forms1 and set(forms1["conv_enc0_stem_kernel"]) == {8}, forms1.get("conv_enc0_stem_kernel")
    for k in want:
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got_enc0, want_enc0)


# ------------------------------------------------------------------------------------------------ (1) enc0 on the 8-channel stem
FWD_SEED = 20261021
ROWS = [0, NB - 1]


def _net_case(which):
    """(parameters, inputs (NB, 3 | 6, 23, 11), condition (NB, 2, ...), times) of the forecaster (5 channels) / interpolator (8)."""
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(909 + (which == "interpolator"))
    n_in = 3 if which == "forecaster" else 6
    x, c = torch.randn(NB, n_in, 23, 11, generator=g), torch.rand(NB, 2, 23, 11, generator=g)
    t = torch.arange(NB, dtype=torch.float32) % 3 + 1
    return (PF if which == "forecaster" else PI), n_in, x, c, t


def _oracle_enc0(which, dropout):
    """enc0 taps of rows ROWS: (fp32 oracle, its bf16 storage model), each (2, 128, 128, 128); with `dropout` on the engine's masks of
    forward 0, global rows ROWS."""
    def run():
        P, _, x, c, t = _net_case(which)
        out = {}
        for name, fwd in (("f32", nets.unet_simple_forward), ("b16", nets.unet_simple_forward_bf16_model)):
            rows = []
            for r in ROWS:
                drop = None
                if dropout:
                    drop = R.EngineDropout(FWD_SEED, MK["dim"], 256, 256, row_offset=r)
                    drop.begin_forward()
                taps = {}
                with torch.no_grad():
                    fwd(P, MK, x[r:r + 1], t[r:r + 1], c[r:r + 1], dropout=drop, taps=taps)
                rows.append(taps["enc0"][0])
            out[name] = torch.stack(rows)
        return out
    return cached(f"enc0_pitch8_{which}_{'drop' if dropout else 'eval'}", run)


@pytest.mark.parametrize("dropout", [False, True], ids=["eval", "engine-dropout"])
@pytest.mark.parametrize("which", ["forecaster", "interpolator"])
def test_enc0_on_the_8_channel_stem_matches_the_oracle_tap(form_switch, which, dropout):
    form_switch.setenv("DYF_STEM_PITCH", 8)
    P, n_in, x, c, t = _net_case(which)
    net = mirror_from_params(P, MK, n_in, 2, 3)
    net._own_engine(NB, (23, 11))
    eng = net._engine
    eng.seed(FWD_SEED)
    eng.form_log(True)
    with net.inference_dropout_scope(dropout):
        y = net(x.to(DEV), time=t.to(DEV), condition=c.to(DEV))
    forms = eng.form_log_read()
    eng.form_log(False)
    assert bool(torch.isfinite(y).all())
    assert forms.get("conv_enc0_stem_kernel") == {NB: 1} and forms.get("stem16_rows_kernel") == {NB: 1}, forms
    got = eng.read_block_output(0, 0, NB)[ROWS].cpu()
    want = _oracle_enc0(which, dropout)
    ring = torch.zeros(128, 128, dtype=torch.bool)
    ring[0], ring[-1], ring[:, 0], ring[:, -1] = True, True, True, True
    for j, r in enumerate(ROWS):
        for tag, sel in (("border ring", ring), ("interior", ~ring)):
            e_eng = rel_rms(got[j][:, sel], want["f32"][j][:, sel])
            e_model = rel_rms(want["b16"][j][:, sel], want["f32"][j][:, sel])
            print(f"enc0 on the 8-channel stem, {which}, dropout {dropout}, row {r}, {tag}: engine {e_eng:.3e}  bf16 model {e_model:.3e}")
            assert e_eng <= 1.25 * e_model + 2e-4, (which, dropout, r, tag)
