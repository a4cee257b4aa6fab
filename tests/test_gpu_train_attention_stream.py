"""-m gpu: the streaming fp32 Attention of a recorded (training) forward -- t_at_stream_fwd keeping the softmax statistics, t_at_stream_bwd_dq /
t_at_stream_bwd_dkv recomputing the scores per 32 x 32 tile (csrc/train_resnet.inc) -- which `unet.Unet` trains with past 4096 bottleneck
tokens, and which the kernel-form switch DYF_TRAIN_ATTN_STREAM_MIN selects below that.

Bounds (the project's): 1e-5 rel-RMS per tensor for an fp32 kernel against float64 (tests/train_op_refs.TOL), losses 1e-4 relative, every
parameter's gradient within 1e-3 of the global gradient norm (tests/test_gpu_training_resnet.py).  A tensor that is zero in float64
(N = 1: dq = dk = 0) is held absolutely against the op's other gradients, as tests/test_gpu_train_ops.py holds it.  Every test prints its
worst value.

Gradient accumulation: the op seam exposes no way to start this op from a gradient `qkv` already has (DYF_TOP_GRAD_IN is up2_bilinear's),
so there is no accumulation case here; in the network `qkv` has one consumer and the adjoint's block becomes its gradient (RCtx::accum).
"""
import ctypes

import numpy as np
import pytest
import torch

import dyffusion_amd as D
from dyffusion_amd import _lib as L
from oracle import nets
from tests import rng_host as R
from tests import train_op_refs as T
from tests.gpu_common import DEV
from tests.helpers import rel_rms
from tests.train_attention_stream_ref import attention_fwd_bwd64

pytestmark = pytest.mark.gpu
ZERO = 1e-12  # tests/test_gpu_train_ops.py ZERO
KEY = "DYF_TRAIN_ATTN_STREAM_MIN"
STREAM_FORMS = ("t_at_stream_fwd", "t_at_stream_bwd_dq", "t_at_stream_bwd_dkv")
NAMES = ("y", "dq", "dk", "dv")


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False)
    e.train_set_precision(32)
    e.set_row_offset(T.ROW_OFFSET)
    yield e
    e.close()


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def run_op(eng, op, qkv, dout, p=0.0, seed=None):
    """qkv (nb, N, 384), dout (nb, N, 128) on the CPU -> {"y", "dq", "dk", "dv"} (nb, N, 128) on the CPU."""
    nb, n, _ = qkv.shape
    if p > 0.0:
        eng.seed(T.SEED if seed is None else seed)  # the forward counter restarts: forward 0, site 0
    r = eng.op_train(op, [qkv.reshape(nb, 1, n, 384).to(DEV)], [], dout.reshape(nb, 1, n, 128).to(DEV), p=p)
    d = r["dinputs"][0].cpu().reshape(nb, n, 384)
    return {"y": r["y"].cpu().reshape(nb, n, 128), "dq": d[..., :128], "dk": d[..., 128:256], "dv": d[..., 256:]}


def errors(got, want, what):
    """rel-RMS per tensor; a tensor that is zero in float64: max |got| against the rms of the op's other gradients."""
    errs = {}
    for k in NAMES:
        w = want[k].reshape(got[k].shape)
        assert bool(torch.isfinite(got[k]).all()), (what, k)
        others = torch.cat([want[n].reshape(-1) for n in NAMES if n != k and n != "y"])
        if k != "y" and rms(w) <= ZERO * rms(others):
            errs[k] = float(got[k].abs().max()) / rms(others)
            print(f"{what}: {k} is zero in float64")
        else:
            errs[k] = rel_rms(got[k], w)
    worst = max(errs, key=errs.get)
    print(f"{what}: max err {errs[worst]:.3e} ({worst}) {({k: f'{v:.2e}' for k, v in errs.items()})}")
    return errs


def host_keep(n, nb, p, seed, row0):
    return torch.from_numpy(np.stack([R.row_mask_nhwc((4, n, n), p, seed, 0, 0, row0 + r) for r in range(nb)]).astype(np.float64))


OP_CASES = [(n, nb, p, kind) for n in (1, 31, 32, 33, 97, 129, 257) for nb in (1, 3) for p in (0.0, 0.15) for kind in ("randn", "wide")]


@pytest.mark.parametrize("args", OP_CASES, ids=[f"N{n}-nb{nb}-p{p}-{kind}" for n, nb, p, kind in OP_CASES])
def test_op_matches_float64(eng, args, request):
    """1. The cases of train_op_refs.build("attention", ...) through op_train("attention_stream") against that module's float64 autograd
    reference on its host-replayed keep masks."""
    case = T.build("attention", args)
    want = case.run(keep=T.engine_keep(case))
    n, nb, p, _ = args
    got = run_op(eng, "attention_stream", case.ins[0].reshape(nb, n, 384), case.dout.reshape(nb, n, 128), p)
    errs = errors(got, want, f"attention_stream {request.node.callspec.id}")
    assert max(errs.values()) <= T.TOL, errs


def test_op_matches_float64_when_every_key_tile_moves_the_max(eng):
    """1. (the saved softmax statistics) N = 97, the "rising" draw of tests/test_gpu_fp32_attention_stream.py."""
    from tests import test_gpu_fp32_attention_stream as FS
    nb, n = 2, 97
    qkv = FS.draw("rising", nb, n, seed=197)
    dout = torch.randn(nb, n, 128, generator=torch.Generator().manual_seed(198))
    got = run_op(eng, "attention_stream", qkv, dout)
    errs = errors(got, attention_fwd_bwd64(qkv, dout), "attention_stream N97 rising")
    assert max(errs.values()) <= T.TOL, errs


def test_op_past_the_old_limit(eng):
    """2. N = 4225 (65 x 65, the OISST-like plane one level down from 130 x 130), against the closed-form float64 reference."""
    nb, n = 1, 4225
    g = torch.Generator().manual_seed(4225)
    qkv, dout = torch.randn(nb, n, 384, generator=g) * 1.5, torch.randn(nb, n, 128, generator=g)
    got = run_op(eng, "attention_stream", qkv, dout)
    errs = errors(got, attention_fwd_bwd64(qkv, dout), "attention_stream N4225")
    assert max(errs.values()) <= T.TOL, errs


@pytest.mark.parametrize("n", [33, 225])
def test_streaming_agrees_with_the_materialising_form(eng, n):
    """3. Same inputs, same engine-generator dropout (same seed, row offset 5) through both forms."""
    nb, p, seed = 2, 0.15, 20261019
    g = torch.Generator().manual_seed(300 + n)
    qkv, dout = torch.randn(nb, n, 384, generator=g) * 1.5, torch.randn(nb, n, 128, generator=g)
    eng.set_row_offset(5)
    try:
        a = run_op(eng, "attention_stream", qkv, dout, p, seed)
        b = run_op(eng, "attention", qkv, dout, p, seed)
    finally:
        eng.set_row_offset(T.ROW_OFFSET)
    want = attention_fwd_bwd64(qkv, dout, host_keep(n, nb, p, seed, 5), p)
    e_forms = errors(a, b, f"N={n} streaming vs materialising")
    e_a, e_b = errors(a, want, f"N={n} streaming vs float64"), errors(b, want, f"N={n} materialising vs float64")
    assert max(max(e.values()) for e in (e_forms, e_a, e_b)) <= T.TOL
    assert rel_rms(a["y"], attention_fwd_bwd64(qkv, dout)["y"]) > 0.1  # the masks did something


def test_gradients_are_bitwise_repeatable(eng):
    """4. No atomics: two runs with the same seed give the same bits."""
    nb, n, p = 3, 257, 0.15
    g = torch.Generator().manual_seed(257)
    qkv, dout = torch.randn(nb, n, 384, generator=g) * 1.5, torch.randn(nb, n, 128, generator=g)
    a, b = run_op(eng, "attention_stream", qkv, dout, p), run_op(eng, "attention_stream", qkv, dout, p)
    assert all(torch.equal(a[k], b[k]) for k in NAMES)
    print("attention_stream N=257 nb=3 p=0.15: two runs bit-equal")


def _forms_of(lib):
    n = lib.dyf_debug_form_log_read(None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.dyf_debug_form_log_read(buf, n + 1)
    return {item.rsplit("=", 1)[0].rsplit("@", 1)[0] for item in buf.value.decode().split(";") if item}


@pytest.mark.parametrize("dropout", [False, True], ids=["no-dropout", "engine-dropout"])
@pytest.mark.parametrize("name", ["plosses_train_resnet_a", "plosses_train_resnet_b"])
def test_whole_step_in_the_forced_streaming_form(name, dropout, monkeypatch):
    """6. The golden training steps of tests/test_gpu_training_resnet.py (its own body and bounds: losses 1e-4 relative, every parameter's
    gradient within 1e-3 of the global gradient norm) with every recorded Attention forced into the streaming form."""
    from tests import test_gpu_training_resnet as TR
    lib = L.lib("fp16")  # unet.Unet's default engine build
    L.set_form(KEY, "1")
    lib.dyf_debug_form_log(1)
    try:
        TR.test_resnet_training_step_matches_autograd_of_the_oracle(name, dropout, monkeypatch)
        forms = _forms_of(lib)
    finally:
        lib.dyf_debug_form_log(0)
        L.set_form(KEY, None)
    print(f"{name} dropout={dropout} with {KEY}=1: attention forms {sorted(f for f in forms if f.startswith('t_at_'))}")
    assert all(f in forms for f in STREAM_FORMS) and "t_at_fwd" not in forms, sorted(forms)


MCFG = dict(dim=64, dim_mults=[1, 2], with_time_emb=True, block_dropout=0.0, block_dropout1=0.0, attn_dropout=0.0)


def _get_loss_step(P, x, y, tt):
    from tests.test_gpu_training_resnet import _mirror
    net = _mirror(P, MCFG, x.shape[1], 0, 1)
    net.train()
    e = net._own_engine(x.shape[0], x.shape[-2:])
    e.form_log(True)
    try:
        loss = net.get_loss(x.to(DEV), y.to(DEV), time=tt.to(DEV))
        loss.backward()
        forms = e.form_log_read()
    finally:
        e.form_log(False)
    return net, loss, forms


def test_whole_net_past_the_old_limit_through_the_public_path():
    """7. dim 64, dim_mults [1, 2] on 130 x 130 (65 x 65 = 4225 bottleneck tokens), nb = 1, no dropout: Unet.get_loss in train mode +
    loss.backward() against torch.autograd over the oracle forward with the same MSE.  At 128 x 128 (exactly 4096 tokens) the step keeps
    the materialising form."""
    from tests.test_gpu_unet_resnet import seeded_unet
    P = seeded_unet(64, (1, 2), 2, 1, seed=81)
    g = torch.Generator().manual_seed(23)
    x, y, tt = torch.randn(1, 2, 130, 130, generator=g), torch.randn(1, 1, 130, 130, generator=g), torch.tensor([2.0])
    net, loss, forms = _get_loss_step(P, x, y, tt)
    cfg = dict(MCFG, resnet_block_groups=8, input_dropout=0.0, upsample_dims=None)
    Pg = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    want = ((nets.resnet_unet_forward(Pg, cfg, x, tt, None) - y) ** 2).mean()
    want.backward()
    gn = float(torch.cat([v.grad.reshape(-1) for v in Pg.values()]).norm())
    errs = {k: float((p.grad.cpu() - Pg[k].grad).norm()) / gn for k, p in net.named_parameters()}
    worst = max(errs, key=errs.get)
    print(f"4225-token unet.Unet get_loss: loss {float(loss):.6f} vs {float(want):.6f}, grad norm {gn:.4f}, worst gradient error / grad norm "
          f"{errs[worst]:.2e} ({worst}); attention forms {sorted(f for f in forms if f.startswith('t_at_'))}")
    assert float(loss) == pytest.approx(float(want), rel=1e-4)
    assert errs[worst] <= 1e-3
    assert all(f in forms for f in STREAM_FORMS) and "t_at_fwd" not in forms, sorted(forms)
    _, loss_s, forms_s = _get_loss_step(P, x[..., :128, :128].contiguous(), y[..., :128, :128].contiguous(), tt)
    assert bool(torch.isfinite(loss_s)) and "t_at_fwd" in forms_s and not any(f in forms_s for f in STREAM_FORMS), sorted(forms_s)


def test_bounds(eng):
    """8. The materialising op keeps its 4096-token refusal; the streaming op and the recorded forward refuse more than 32 767 tokens (the
    uint32 dropout element index) by name, before anything is allocated."""
    with pytest.raises(NotImplementedError):
        eng.op_train("attention", [torch.zeros(1, 1, 4097, 384, device=DEV)], [], torch.zeros(1, 1, 4097, 128, device=DEV))
    with pytest.raises(NotImplementedError, match="32767"):
        eng.op_train("attention_stream", [torch.zeros(1, 1, 32768, 384, device=DEV)], [], torch.zeros(1, 1, 32768, 128, device=DEV))
    from tests.test_gpu_training_resnet import _mirror
    from tests.test_gpu_unet_resnet import seeded_unet
    net = _mirror(seeded_unet(64, (1, 2), 2, 1, seed=82), MCFG, 2, 0, 1)  # 364 x 364: 182 x 182 = 33 124 bottleneck tokens
    net.train()
    with pytest.raises(NotImplementedError, match="32767"):
        net.get_loss(torch.zeros(1, 2, 364, 364, device=DEV), torch.zeros(1, 1, 364, 364, device=DEV), time=torch.ones(1, device=DEV))
