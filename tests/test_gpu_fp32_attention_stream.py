"""-m gpu: the streaming fp32 Attention core (csrc/train_resnet.inc t_at_stream_fwd) that fp32 sampling takes past 4096 bottleneck tokens.

Reference: float64 softmax attention in torch on the CPU, head by head.  Bound of the core alone: rel-RMS <= 1e-5, the per-forward
bound of the project's fp32 kernels (tests/test_gpu_training.py); an fp32 tile-of-32 online softmax sits at 4e-7 .. 2.2e-6 against
float64 on the draws used here, so the reference arithmetic is >= 4 x inside it.  Whole networks and rollouts: 1e-4 per field
(tests/test_gpu_fp32_sampling.py TOL32).  Every test prints its worst value.
"""
import numpy as np
import pytest
import torch

import dyffusion_amd as D
from oracle import nets, sampler
from tests import rng_host as R
from tests.gpu_common import DEV
from tests.helpers import rel_rms

pytestmark = pytest.mark.gpu
TOL_CORE = 1e-5
TOL32 = 1e-4


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=2, use_graph=False)
    yield e
    e.close()


def attention64(qkv, keep=None, p=0.0):
    """float64 softmax attention, head by head: qkv (nb, N, 384) -> (nb, N, 128); keep (nb, 4, N, N): dropout on the probabilities."""
    nb, n, _ = qkv.shape
    x = qkv.double()
    q, k, v = (x[:, :, i * 128:(i + 1) * 128].reshape(nb, n, 4, 32).permute(0, 2, 1, 3) for i in range(3))
    out = torch.empty(nb, 4, n, 32, dtype=torch.float64)
    for b in range(nb):
        for h in range(4):
            pr = torch.softmax(q[b, h] @ k[b, h].T * (32 ** -0.5), dim=-1)
            if keep is not None:
                pr = pr * keep[b, h].double() * (1.0 / (1.0 - p))
            out[b, h] = pr @ v[b, h]
    return out.permute(0, 2, 1, 3).reshape(nb, n, 128)


def draw(kind, nb, n, seed):
    g = torch.Generator().manual_seed(seed)
    qkv = torch.randn(nb, n, 384, generator=g) * 1.5
    if kind == "scores_x4":  # the running max dominates
        qkv[:, :, :128] *= 4.0
    elif kind == "rising":   # q_i . k_j rises with j for every query: every key tile moves the max
        qkv[:, :, :128].view(nb, n, 4, 32)[..., 0] = 1.0 + qkv[:, :, :128].view(nb, n, 4, 32)[..., 0].abs()
        k = qkv[:, :, 128:256].view(nb, n, 4, 32)
        k.zero_()
        k[..., 0] = (torch.arange(n, dtype=torch.float32) * (40.0 / n)).view(1, n, 1)
    return qkv.contiguous()


@pytest.mark.parametrize("kind", ["randn", "scores_x4", "rising"])
@pytest.mark.parametrize("n", [1, 31, 32, 33, 97, 256, 4225])
def test_streaming_core_matches_float64_at_the_edges(eng, n, kind):
    nb = 1 if n == 4225 else 2
    qkv = draw(kind, nb, n, seed=100 + n)
    got = eng.op_attention_f32(qkv.to(DEV), form=1).cpu()
    err = rel_rms(got, attention64(qkv))
    print(f"streaming core N={n} nb={nb} {kind}: rel-rms vs float64 {err:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= TOL_CORE


@pytest.mark.parametrize("n", [225, 780, 4096])
def test_streaming_equals_materialising(eng, n):
    qkv = draw("randn", 1, n, seed=7 + n).to(DEV)
    a, b = eng.op_attention_f32(qkv, form=1).cpu(), eng.op_attention_f32(qkv, form=0).cpu()
    err = rel_rms(a, b)
    print(f"streaming vs materialising N={n}: rel-rms {err:.3e}")
    assert err <= TOL_CORE


def test_materialising_form_keeps_its_limit(eng):
    qkv = torch.zeros(1, 4097, 384, device=DEV)
    with pytest.raises(NotImplementedError):
        eng.op_attention_f32(qkv, form=0)


@pytest.mark.parametrize("n", [33, 97])
def test_dropout_with_an_injected_mask(eng, n):
    nb, p = 2, 0.2
    qkv = draw("randn", nb, n, seed=300 + n)
    keep = (torch.rand(nb, 4, n, n, generator=torch.Generator().manual_seed(n)) >= p).to(torch.uint8)
    got = eng.op_attention_f32(qkv.to(DEV), p_drop=p, mask=keep.to(DEV), form=1).cpu()
    err = rel_rms(got, attention64(qkv, keep, p))
    moved = rel_rms(got, attention64(qkv))
    print(f"streaming core N={n}, injected mask: rel-rms vs float64 {err:.3e}; vs eval {moved:.3e}")
    assert err <= TOL_CORE and moved > 0.1


@pytest.mark.parametrize("n", [33, 64])
def test_dropout_from_the_engine_generator(eng, n):
    """Same seed, forward counter (0) and row offset (5) for both forms; N = 33: a keep-word pair straddles two queries."""
    nb, p, seed = 2, 0.2, 20261018
    qkv = draw("randn", nb, n, seed=400 + n)
    out = []
    for form in (1, 0):
        eng.seed(seed)
        eng.set_row_offset(5)
        out.append(eng.op_attention_f32(qkv.to(DEV), p_drop=p, form=form).cpu())
    eng.set_row_offset(0)
    keep = torch.from_numpy(np.stack([R.row_mask_nhwc((4, n, n), p, seed, 0, 0, 5 + r) for r in range(nb)]).astype(np.uint8))
    want = attention64(qkv, keep, p)
    e_forms, e1, e0 = rel_rms(out[0], out[1]), rel_rms(out[0], want), rel_rms(out[1], want)
    print(f"engine generator N={n}: streaming vs materialising {e_forms:.3e}; vs float64 on the host mask {e1:.3e} / {e0:.3e}")
    assert max(e_forms, e1, e0) <= TOL_CORE


MCFG = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0,
            resnet_block_groups=8, input_dropout=0.0, upsample_dims=None)


def test_whole_network_past_the_old_limit():
    """dim 64, dim_mults [1, 2] on 130 x 130: 65 x 65 = 4225 bottleneck tokens.  Eval and attention dropout with the oracle's masks
    injected against the oracle; the form log names the streaming core, and at 128 x 128 (exactly 4096 tokens) it does not."""
    from tests.test_gpu_unet_resnet import engine_masks, mirror, seeded_unet
    P = seeded_unet(64, (1, 2), 2, 1, seed=71)
    g = torch.Generator().manual_seed(13)
    x, t = torch.randn(2, 2, 130, 130, generator=g), torch.tensor([1.0, 3.0])
    net = mirror(P, MCFG, 2, 0, 1, "fp32")
    y = net(x.to(DEV), time=t.to(DEV)).cpu()
    assert net._engine.dtype == "fp32"
    with torch.no_grad():
        e_eval = rel_rms(y, nets.resnet_unet_forward(P, MCFG, x, t, None))
    cfg_d = dict(MCFG, attn_dropout=0.2)
    net_d = mirror(P, cfg_d, 2, 0, 1, "fp32")
    src = nets.DropoutSeeded(5, record=True)
    with torch.no_grad():
        want = nets.resnet_unet_forward(P, cfg_d, x, t, None, dropout=src)
    eng = net_d._own_engine(2, (130, 130))
    eng.form_log(True)
    y_d = eng.net_forward(0, x.to(DEV), t.to(DEV), None, dropout_mode=2, masks=engine_masks(src.masks, 2)).cpu()
    forms = eng.form_log_read()
    eng.form_log(False)
    e_drop = rel_rms(y_d, want)
    print(f"4225-token unet.Unet in fp32: eval rel-rms {e_eval:.3e}, injected attention dropout rel-rms {e_drop:.3e}")
    assert max(e_eval, e_drop) <= TOL32
    assert "t_at_stream_fwd" in forms, sorted(forms)
    net_s = mirror(P, MCFG, 2, 0, 1, "fp32")
    eng = net_s._own_engine(2, (128, 128))
    eng.form_log(True)
    y_s = net_s(x[:, :, :128, :128].contiguous().to(DEV), time=t.to(DEV))
    forms = eng.form_log_read()
    eng.form_log(False)
    assert bool(torch.isfinite(y_s).all()) and "t_at_stream_fwd" not in forms, sorted(forms)


def test_rollout_past_the_old_limit_graph_equals_eager_and_replays():
    from tests.test_gpu_unet_resnet import mirror, seeded_unet
    PF, PI = seeded_unet(64, (1, 2), 2, 1, seed=72), seeded_unet(64, (1, 2), 2, 1, seed=73)
    hp = dict(timesteps=3, schedule="before_t1_only", interpolate_before_t1=True, sampling_type="cold",
              refine_intermediate_predictions=False, forward_conditioning="data", enable_interpolator_dropout=False)

    def build(use_graph):
        return D.DYffusion(mirror(PF, MCFG, 1, 1, 1), D.InterpolatorHandle(mirror(PI, MCFG, 2, 0, 1), 3), max_batch=2, dtype="fp32",
                           use_graph=use_graph, **hp)

    x0 = torch.randn(2, 1, 130, 130, generator=torch.Generator().manual_seed(14))
    a, b = build(True), build(False)
    ya1 = {k: v.clone() for k, v in a.sample(x0.to(DEV)).items()}
    ya2 = {k: v.clone() for k, v in a.sample(x0.to(DEV)).items()}
    yb = b.sample(x0.to(DEV))
    assert a._engine.dtype == "fp32" and a._engine.sample_precision == 32
    for k in yb:
        assert torch.equal(ya1[k], ya2[k]) and torch.equal(ya1[k], yb[k]), k
    with torch.no_grad():
        want = sampler.sample_loop(lambda x, t, cnd: nets.resnet_unet_forward(PF, MCFG, x, t, cnd),
                                   lambda x, t, cnd: nets.resnet_unet_forward(PI, MCFG, x, t, cnd), x0, None, hp)
    assert sorted(ya1) == sorted(want)
    worst = max(rel_rms(ya1[k].cpu(), want[k]) for k in want)
    print("fp32 rollout at 4225 bottleneck tokens: worst rel-rms", worst)
    assert worst <= TOL32


def test_the_new_bound_is_refused_and_named():
    """364 x 364 input: 182 x 182 = 33 124 bottleneck tokens > 32 767.  Refused when the precision is set; no forward runs."""
    cfg = D.resnet_net_config(in_channels=2, cond_channels=0, out_channels=1, dim=64, dim_mults=(1, 2))
    e = D.HipEngine(cfg, cfg, 364, 364, max_batch=1, use_graph=False, dtype="fp16")
    try:
        with pytest.raises(NotImplementedError, match="32767"):
            e.set_sample_precision(32)
        assert e.sample_precision == 16
    finally:
        e.close()
