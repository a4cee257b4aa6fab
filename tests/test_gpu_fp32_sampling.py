"""-m gpu: fp32 sampling (`dtype="fp32"`, dyf_set_sample_precision(32)) of all three backbones.

Tolerance (stated): rel-RMS <= 1e-4 per field over the full rollout against the reference's goldens / the fp32 oracle.
The fp32 forward kernels are held to 1e-5 per forward (tests/test_gpu_training.py), the oracle to <= 5e-6 against the goldens on the
CPU (tests/test_oracle_*.py), so the reference side sits an order of magnitude inside the bound.  Every test prints its worst value.
"""
import gc
import json

import pytest
import torch

import dyffusion_amd as D
from oracle import nets, sampler
from tests import rng_host as R
from tests.gpu_common import DEV, build_dyffusion, mirror_from_params, nhwc_masks, oracle_rollout, seeded_pair
from tests.helpers import load_npz, rel_rms, split_state
from tests.test_gpu_sampler import NAMES

pytestmark = pytest.mark.gpu
TOL32 = 1e-4
TOL_BF16, TOL_FP16 = 2.5e-2, 1e-2  # tests/test_gpu_sampler.TOL, tests/test_gpu_fp16.py

HP4 = dict(timesteps=4, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only",
           sampling_type="cold", refine_intermediate_predictions=True, enable_interpolator_dropout=False, num_input_channels=3)
MK64 = dict(dim=64, upsample_dims=[64, 64], outer_sample_mode="bilinear", with_time_emb=True, dropout=0.15)


@pytest.mark.parametrize("name", NAMES)
def test_fp32_rollout_matches_reference_golden(name):
    """Every G4 fixture of tests/test_gpu_sampler.py through an fp32 engine: injected masks (sample_dropout), injected noise
    (sample_datanoise) and the logged intermediates (sample_log_*) included."""
    z = load_npz(name + ".npz")
    hp = json.loads(str(z["hp"]))
    PF, PI = split_state(z, "F"), split_state(z, "I")
    N, B = hp["num_predictions"], hp["B"]
    x0 = torch.from_numpy(z["x0"]).repeat(N, 1, 1, 1)
    c = torch.from_numpy(z["c"]).repeat(N, 1, 1, 1)
    m = build_dyffusion(PF, PI, hp["model"], 4, 1, hp, max_batch=N * B, dtype="fp32")
    masks = noise = None
    if hp.get("enable_interpolator_dropout"):
        src = nets.DropoutSeeded(hp["dropout_seed"], record=True)
        oracle_rollout(PF, PI, hp["model"], hp, x0, c, drop=src)
        masks = nhwc_masks(src.masks)
    if hp["forward_conditioning"] == "data+noise":
        gen = torch.Generator().manual_seed(hp["noise_seed"])
        draws = []

        def nf(t):
            draws.append(torch.randn(t.shape, generator=gen))
            return draws[-1]

        oracle_rollout(PF, PI, hp["model"], hp, x0, c, noise_fn=nf)
        noise = torch.stack(draws, 0).to(DEV)
    _, got, _ = m.sample_loop(x0.to(DEV), static_condition=c.to(DEV), _masks=masks, _noise=noise)
    assert m._engine.dtype == "fp32" and m._engine.sample_precision == 32
    want = {k[len("out::"):]: v for k, v in z.items() if k.startswith("out::")}
    assert sorted(got) == sorted(want)
    worst = max(rel_rms(got[k].cpu().reshape(w.shape), w) for k, w in want.items())
    print(name, "fp32 worst rel-rms", worst)
    assert worst <= TOL32


def test_fp32_matrix_core_sizes_graph_equals_eager_and_is_repeatable():
    """dim 64 on a 64 x 64 inner grid: the convolutions run on the fp32 matrix cores (split-K partial sums reduced in a fixed order).
    Captured rollout == eager launch, bit for bit; two replays are bit-identical; the fields meet the fp32 tolerance."""
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(2)
    x0, c = torch.randn(3, 3, 23, 11, generator=g).to(DEV), torch.rand(3, 2, 23, 11, generator=g).to(DEV)
    a = build_dyffusion(PF, PI, MK64, 3, 2, HP4, max_batch=3, use_graph=True, dtype="fp32")
    b = build_dyffusion(PF, PI, MK64, 3, 2, HP4, max_batch=3, use_graph=False, dtype="float32")
    ya1 = {k: v.clone() for k, v in a.sample(x0, static_condition=c).items()}
    ya2 = {k: v.clone() for k, v in a.sample(x0, static_condition=c).items()}
    yb = b.sample(x0, static_condition=c)
    assert a._engine.forward_counts() == (4, 8)
    for k in yb:
        assert torch.equal(ya1[k], yb[k]) and torch.equal(ya2[k], yb[k]), k
    want = oracle_rollout(PF, PI, MK64, HP4, x0.cpu(), c.cpu())
    assert sorted(want) == sorted(ya1)
    worst = max(rel_rms(ya1[k].cpu(), want[k]) for k in want)
    print("fp32 dim64 h=4 rollout worst rel-rms", worst)
    assert worst <= TOL32


def _oracle_rollout_with_engine_masks(PF, PI, mk, hp, x0, c, seed, row_offset=0, first_forward=0):
    uh, uw = mk["upsample_dims"]
    drop = R.EngineDropout(seed, mk["dim"], uh, uw, row_offset=row_offset, first_forward=first_forward)

    def i_fn(x, t, cond):
        drop.begin_forward()
        return nets.unet_simple_forward(PI, mk, x, t, cond, dropout=drop)

    with torch.no_grad():
        out = sampler.sample_loop(lambda x, t, cond: nets.unet_simple_forward(PF, mk, x, t, cond), i_fn, x0, c, hp)
    return out, drop.fwd + 1


@pytest.mark.parametrize("hp_extra", [dict(), dict(additional_interpolation_steps=2, timesteps=5, use_cold_sampling_for_last_step=True)],
                         ids=["h4", "h5k2_coldlast"])
def test_fp32_rng_mode_rollout_equals_oracle_with_host_reproduced_masks(hp_extra):
    """Engine generator, captured graph, two consecutive sample() calls: the oracle on the host-rebuilt masks of forward counters
    [0, n_i) and [n_i, 2 n_i) -- the un-paired forward order -- to the fp32 tolerance."""
    hp = dict(HP4, enable_interpolator_dropout=True, **hp_extra)
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(21)
    nb = 3
    x0, c = torch.randn(nb, 3, 23, 11, generator=g), torch.rand(nb, 2, 23, 11, generator=g)
    m = build_dyffusion(PF, PI, MK64, 3, 2, hp, max_batch=nb, use_graph=True, dtype="fp32")
    seed = 987654321
    m.seed(seed)
    got1 = {k: v.cpu() for k, v in m.sample(x0.to(DEV), static_condition=c.to(DEV)).items()}
    got2 = {k: v.cpu() for k, v in m.sample(x0.to(DEV), static_condition=c.to(DEV)).items()}  # graph replay
    want1, nfwd = _oracle_rollout_with_engine_masks(PF, PI, MK64, hp, x0, c, seed)
    want2, _ = _oracle_rollout_with_engine_masks(PF, PI, MK64, hp, x0, c, seed, first_forward=nfwd)
    n_f, n_i = m._engine.forward_counts()
    assert nfwd == n_i
    for tag, got, want in (("first call", got1, want1), ("graph replay", got2, want2)):
        assert sorted(got) == sorted(want)
        worst = max(rel_rms(got[k], want[k]) for k in want)
        print(f"fp32 rng-mode rollout ({tag}) worst rel-rms vs oracle on host-rebuilt masks: {worst:.3e}")
        assert worst <= TOL32
    assert min(rel_rms(got1[k], got2[k]) for k in got1) > 5e-2


def test_same_seed_draws_the_same_masks_at_every_precision():
    """bf16, fp16 and fp32 engines with one seed: the 16-bit rollouts sit within their own storage tolerance of the fp32 one (a wrong
    mask anywhere moves a field by > 5e-2) and are not bit-equal to it; the fp32 stream is a function of the global row."""
    hp = dict(HP4, enable_interpolator_dropout=True)
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(22)
    nb = 4
    x0, c = torch.randn(nb, 3, 23, 11, generator=g).to(DEV), torch.rand(nb, 2, 23, 11, generator=g).to(DEV)

    def run(dtype, rows=slice(0, nb), offset=0):
        m = build_dyffusion(PF, PI, MK64, 3, 2, hp, max_batch=nb, dtype=dtype)
        m.seed(42)
        m.set_row_offset(offset)
        return {k: v.clone() for k, v in m.sample(x0[rows], static_condition=c[rows]).items()}

    y32 = run("fp32")
    for dtype, tol in (("bf16", TOL_BF16), ("fp16", TOL_FP16)):
        y16 = run(dtype)
        worst = max(rel_rms(y16[k].cpu(), y32[k].cpu()) for k in y32)
        print(f"{dtype} vs fp32, same seed: worst rel-rms {worst:.3e}")
        assert worst <= tol
        assert not any(torch.equal(y16[k], y32[k]) for k in y32)
    lo, hi = run("fp32", rows=slice(0, 2)), run("fp32", rows=slice(2, 4), offset=2)
    worst = max(max(rel_rms(lo[k].cpu(), y32[k][:2].cpu()), rel_rms(hi[k].cpu(), y32[k][2:].cpu())) for k in y32)
    print(f"fp32 rows [0:2] + [2:4] at row offset 2 vs the 4-row batch: worst rel-rms {worst:.3e}")
    assert worst <= TOL32


def test_fp32_net_forward_with_engine_rng_and_injected_masks():
    """The per-network seam on an fp32 engine (`net.engine_dtype = "fp32"`): eval, engine generator with a row offset, and the SAME
    masks injected as uint8 tensors, each against the oracle."""
    from oracle import init as oinit
    P = oinit.seeded_state(oinit.unet_simple_param_shapes(64, 5, 3), seed=36)
    g = torch.Generator().manual_seed(10)
    x, c, t = torch.randn(2, 3, 23, 11, generator=g), torch.rand(2, 2, 23, 11, generator=g), torch.tensor([2.0, 3.0])
    net = mirror_from_params(P, MK64, 3, 2, 3)
    net.engine_dtype = "fp32"
    y_eval = net(x.to(DEV), time=t.to(DEV), condition=c.to(DEV)).cpu()
    assert net._engine.dtype == "fp32"
    with torch.no_grad():
        e0 = rel_rms(y_eval, nets.unet_simple_forward(P, MK64, x, t, c))
    seed = 1234567890123
    with net.inference_dropout_scope(True):
        net._engine.seed(seed)
        net._engine.set_row_offset(5)
        y = net(x.to(DEV), time=t.to(DEV), condition=c.to(DEV)).cpu()
        net._engine.set_row_offset(0)
    drop = R.EngineDropout(seed, 64, 64, 64, row_offset=5)
    drop.begin_forward()
    rec = nets.DropoutSeeded(7, record=True)
    with torch.no_grad():
        e1 = rel_rms(y, nets.unet_simple_forward(P, MK64, x, t, c, dropout=drop))
        want_m = nets.unet_simple_forward(P, MK64, x, t, c, dropout=rec)
    y_m = net._engine.net_forward(0, x.to(DEV), t.to(DEV), c.to(DEV), dropout_mode=2, masks=nhwc_masks(rec.masks)).cpu()
    e2 = rel_rms(y_m, want_m)
    print(f"fp32 net_forward vs oracle: eval {e0:.3e}, engine rng {e1:.3e}, injected masks {e2:.3e}")
    assert max(e0, e1, e2) <= TOL32 and rel_rms(y, y_eval) > 0.1 and rel_rms(y_m, y_eval) > 0.1


def test_switching_the_precision_of_one_engine():
    """16 -> 32 -> 16 on one engine with graphs: the 16-bit result comes back bit for bit (no graph of the other precision is
    replayed), the 32-bit result in the middle is a fresh fp32 engine's; 24 bits is a ValueError; close() returns the arena."""
    PF, PI = seeded_pair(64, 3, 2)
    g = torch.Generator().manual_seed(2)
    x0, c = torch.randn(3, 3, 23, 11, generator=g).to(DEV), torch.rand(3, 2, 23, 11, generator=g).to(DEV)

    def used():
        free, total = torch.cuda.mem_get_info()
        return (total - free) / 2 ** 20

    fresh = build_dyffusion(PF, PI, MK64, 3, 2, HP4, max_batch=3, use_graph=True, dtype="fp32")
    want32 = {k: v.clone() for k, v in fresh.sample(x0, static_condition=c).items()}
    marks = []
    for _ in range(4):
        m = build_dyffusion(PF, PI, MK64, 3, 2, HP4, max_batch=3, use_graph=True)
        y16 = {k: v.clone() for k, v in m.sample(x0, static_condition=c).items()}
        eng = m._engine
        assert eng.sample_precision == 16 and eng.dtype == "bf16"
        eng.set_sample_precision(32)
        assert eng.sample_precision == 32
        y32 = {k: v.clone() for k, v in m.sample(x0, static_condition=c).items()}
        with pytest.raises(ValueError):
            eng.set_sample_precision(24)
        assert eng.sample_precision == 32
        eng.set_sample_precision(16)
        y16b = m.sample(x0, static_condition=c)
        for k in y16:
            assert torch.equal(y16[k], y16b[k]), k
            assert torch.equal(y32[k], want32[k]), k
            assert not torch.equal(y16[k], y32[k]), k
        eng.close()
        del m, eng, y16b
        gc.collect()
        torch.cuda.synchronize()
        marks.append(used())
    print("MiB in use after each close:", [round(v) for v in marks])
    assert marks[-1] - marks[1] <= 32.0


RESNET_GOLDENS = ["net_unet_resnet_a", "net_unet_resnet_b", "net_unet_resnet_c", "net_unet_resnet_d", "net_unet_resnet_e", "net_unet_resnet_g"]


@pytest.mark.parametrize("name", RESNET_GOLDENS)
def test_fp32_small_resnet_unets_match_reference_goldens(name):
    """unet.Unet goldens through an fp32 engine: eval, and dropout with the oracle's masks injected (activation sites NHWC, the
    attention-probability mask (b, 4, n, n) as it is)."""
    from tests.test_gpu_unet_resnet import engine_masks, mirror
    z = load_npz(name + ".npz")
    P, cfg = split_state(z, "P"), json.loads(str(z["cfg"]))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    c = torch.from_numpy(z["c"]) if "c" in z else None
    net = mirror(P, cfg, x.shape[1], 0 if c is None else c.shape[1], z["y_eval"].shape[1], "fp32")
    y = net(x.to(DEV), time=t.to(DEV), condition=None if c is None else c.to(DEV)).cpu()
    assert net._engine.dtype == "fp32"
    e_eval = rel_rms(y, z["y_eval"])
    src = nets.DropoutSeeded(int(z["dropout_seed"]), record=True)
    with torch.no_grad():
        nets.resnet_unet_forward(P, cfg, x, t, c, dropout=src)
    y = net._engine.net_forward(0, x.to(DEV), t.to(DEV), None if c is None else c.to(DEV), dropout_mode=2,
                                masks=engine_masks(src.masks, len(cfg["dim_mults"]))).cpu()
    e_drop = rel_rms(y, z["y_drop"])
    print(name, f"fp32 eval rel-rms {e_eval:.3e}, injected-mask dropout rel-rms {e_drop:.3e}")
    assert max(e_eval, e_drop) <= TOL32


def test_fp32_oisst_style_rollout_matches_oracle():
    """The OISST miniature of tests/test_gpu_unet_resnet.py (24 x 16, data+noise with injected draws, k = 2 extra steps, injected
    masks including the attention-probability mask) on an fp32 engine."""
    from tests.test_gpu_unet_resnet import mirror, rollout_masks, seeded_unet
    mcfg_i = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.3, block_dropout1=0.1, attn_dropout=0.2,
                  resnet_block_groups=8, input_dropout=0.0, upsample_dims=None)
    mcfg_f = dict(mcfg_i, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0)
    PF, PI = seeded_unet(64, (1, 2), 2, 1, seed=61), seeded_unet(64, (1, 2), 2, 1, seed=62)
    hp = dict(timesteps=4, schedule="before_t1_only", additional_interpolation_steps=2, interpolate_before_t1=True,
              sampling_type="cold", refine_intermediate_predictions=False, forward_conditioning="data+noise",
              time_encoding="dynamics", enable_interpolator_dropout=True)
    m = D.DYffusion(mirror(PF, mcfg_f, 1, 1, 1), D.InterpolatorHandle(mirror(PI, mcfg_i, 2, 0, 1), 4), max_batch=3, dtype="fp32", **hp)
    x0 = torch.randn(3, 1, 24, 16, generator=torch.Generator().manual_seed(12))
    drop = nets.DropoutSeeded(3, record=True)
    gen = torch.Generator().manual_seed(4)
    draws = []

    def nf(t):
        draws.append(torch.randn(t.shape, generator=gen))
        return draws[-1]

    with torch.no_grad():
        want = sampler.sample_loop(lambda x, t, cnd: nets.resnet_unet_forward(PF, mcfg_f, x, t, cnd),
                                   lambda x, t, cnd: nets.resnet_unet_forward(PI, mcfg_i, x, t, cnd, dropout=drop),
                                   x0, None, hp, noise_fn=nf)
    _, got, _ = m.sample_loop(x0.to(DEV), _masks=rollout_masks(drop.masks, 2, 27), _noise=torch.stack(draws, 0).to(DEV))
    assert sorted(got) == sorted(want)
    worst = max(rel_rms(got[k].cpu(), want[k]) for k in want)
    print("fp32 OISST-style rollout worst rel-rms", worst)
    assert worst <= TOL32


def test_long_resnet_unet_plans_are_accepted_in_fp32():
    """The bf16 refusal of ResNet-UNet plans beyond 32 forwards does not apply to an fp32 engine (construction and plan only)."""
    from tests.test_gpu_unet_resnet import mirror, seeded_unet
    cfg = dict(dim=64, dim_mults=[1, 2, 4], with_time_emb=True, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0,
               resnet_block_groups=8, input_dropout=0.0, upsample_dims=None)
    PF, PI = seeded_unet(64, (1, 2, 4), 2, 1, seed=1), seeded_unet(64, (1, 2, 4), 2, 1, seed=2)
    hp = dict(timesteps=7, schedule="before_t1_only", additional_interpolation_steps=25, interpolate_before_t1=True,
              sampling_type="cold", refine_intermediate_predictions=False, forward_conditioning="data", enable_interpolator_dropout=False)
    m = D.DYffusion(mirror(PF, cfg, 1, 1, 1), D.InterpolatorHandle(mirror(PI, cfg, 2, 0, 1), 7), max_batch=2, dtype="fp32", **hp)
    eng = m._ensure_engine((60, 60), 2)
    m._ensure_plan(eng)
    assert eng.dtype == "fp32" and sum(eng.forward_counts()) > 32


def test_fp32_simple_conv_net_forward_matches_reference_golden():
    """SimpleConvNet (spring-mesh backbone) through an fp32 engine: eval against the reference's golden, the oracle's masks injected,
    and the engine generator (different draws per forward)."""
    z = load_npz("net_simple_conv.npz")
    P, cfg = split_state(z, "P"), json.loads(str(z["cfg"]))
    x, t = torch.from_numpy(z["x"]), torch.from_numpy(z["t"])
    c = torch.from_numpy(z["c"]) if "c" in z else None
    net = D.SimpleConvNet(dim=cfg["dim"], with_time_emb=cfg.get("with_time_emb", True), kernel_sizes=cfg["kernel_sizes"],
                          dropout=cfg.get("dropout", 0.0), num_input_channels=x.shape[1], num_output_channels=z["y_eval"].shape[1],
                          num_conditional_channels=0 if c is None else c.shape[1])
    net.engine_dtype = "fp32"
    net.load_state_dict(P, strict=True)
    cd = None if c is None else c.to(DEV)
    y = net(x.to(DEV), time=t.to(DEV), condition=cd).cpu()
    assert net._engine.dtype == "fp32"
    e_eval = rel_rms(y, z["y_eval"])
    src = nets.DropoutSeeded(4242, record=True)
    with torch.no_grad():
        y_or = nets.simple_conv_net_forward(P, cfg, x, t, c, dropout=src)
    y = net._engine.net_forward(0, x.to(DEV), t.to(DEV), cd, dropout_mode=2, masks=nhwc_masks(src.masks)).cpu()
    e_drop = rel_rms(y, y_or)
    print(f"fp32 simple_conv eval rel-rms {e_eval:.3e}, injected-mask dropout rel-rms {e_drop:.3e}")
    assert max(e_eval, e_drop) <= TOL32
    net.enable_inference_dropout()
    a, b = net(x.to(DEV), time=t.to(DEV), condition=cd).cpu(), net(x.to(DEV), time=t.to(DEV), condition=cd).cpu()
    assert torch.isfinite(a).all() and not torch.equal(a, b)


def test_fp32_spring_mesh_rollout_of_a_simple_conv_net_pair_matches_oracle():
    """BASELINE configs[0] shapes (SimpleConvNet dim 64, k = 9, 7, 5, 3 on 10 x 10, forward_conditioning 'data', cold + refine) on an
    fp32 engine; the captured rollout replays bit for bit."""
    from oracle import init as oinit
    C, Cs, h, nb = 4, 1, 4, 5
    cfg = dict(dim=64, kernel_sizes=[9, 7, 5, 3], with_time_emb=True, dropout=0.1, residual=True)
    hp = dict(timesteps=h, forward_conditioning="data", interpolate_before_t1=True, schedule="before_t1_only",
              sampling_type="cold", refine_intermediate_predictions=True, num_input_channels=C)
    PF = oinit.seeded_state(oinit.simple_conv_net_param_shapes(64, C + C + Cs, C, cfg["kernel_sizes"]), seed=7, gain=0.8)
    PI = oinit.seeded_state(oinit.simple_conv_net_param_shapes(64, 2 * C + Cs, C, cfg["kernel_sizes"]), seed=8, gain=0.8)

    def mirror(P, n_in, n_cond):
        net = D.SimpleConvNet(dim=64, with_time_emb=True, kernel_sizes=cfg["kernel_sizes"], dropout=0.1, num_input_channels=n_in,
                              num_output_channels=C, num_conditional_channels=n_cond)
        net.load_state_dict(P, strict=True)
        return net

    m = D.DYffusion(mirror(PF, C, C + Cs), D.InterpolatorHandle(mirror(PI, 2 * C, Cs), h), timesteps=h, forward_conditioning="data",
                    interpolate_before_t1=True, refine_intermediate_predictions=True, enable_interpolator_dropout=False, max_batch=nb,
                    dtype="fp32")
    g = torch.Generator().manual_seed(9)
    x0, c = torch.randn(nb, C, 10, 10, generator=g), torch.rand(nb, Cs, 10, 10, generator=g)
    got = {k: v.clone() for k, v in m.sample(x0.to(DEV), static_condition=c.to(DEV)).items()}
    with torch.no_grad():
        want = sampler.sample_loop(lambda x, t, cond: nets.simple_conv_net_forward(PF, cfg, x, t, cond),
                                   lambda x, t, cond: nets.simple_conv_net_forward(PI, cfg, x, t, cond), x0, c, hp)
    assert sorted(got) == sorted(want)
    worst = max(rel_rms(got[k].cpu(), want[k]) for k in want)
    print("fp32 spring-mesh rollout worst rel-rms", worst)
    assert worst <= TOL32
    again = m.sample(x0.to(DEV), static_condition=c.to(DEV))
    assert all(torch.equal(got[k], again[k]) for k in got)


def test_fp32_predict_step_autoregressive_with_boundary_conditions_matches_reference_golden():
    """`predict_step` of the experiment wrapper (two autoregressive outer iterations, spring-mesh boundary conditions on the device)
    on an fp32 engine against the reference's golden `predict_step_spring_ar2`."""
    import numpy as np
    from tests.test_gpu_experiment import _SpringDataModule
    z = load_npz("predict_step_spring_ar2.npz")
    hp = json.loads(str(z["hp"]))
    N, B = hp["num_predictions"], hp["B"]
    m = build_dyffusion(split_state(z, "F"), split_state(z, "I"), hp["model"], 4, 1, hp, max_batch=N * B, dtype="fp32")
    eng = m._ensure_engine((10, 10), N * B)
    exp = D.MultiHorizonForecastingDYffusion(m, num_predictions=N, autoregressive_steps=1, datamodule=_SpringDataModule(eng))
    feats = torch.zeros(B, 5, 4, 10, 10)
    feats[:, 0, 2:] = torch.from_numpy(z["base_q"])
    batch = {"dynamics": torch.from_numpy(z["dynamics"]).to(DEV), "condition": torch.from_numpy(z["condition"]).to(DEV),
             "metadata": {"fixed_mask": torch.from_numpy(z["fixed_mask"]), "features": feats}}
    exp.predict_step(batch, 0)
    got = exp._predict_step_outputs[0]
    want = {k[len("out::"):]: v for k, v in z.items() if k.startswith("out::")}
    assert list(got) == list(want) and eng.dtype == "fp32"
    worst = 0.0
    for k, w in want.items():
        if k.endswith("targets"):
            assert np.array_equal(got[k], w), k
        else:
            worst = max(worst, rel_rms(got[k], w))
    print("fp32 predict_step (2 x h=4, spring BC) worst rel-rms", worst)
    assert worst <= TOL32
