"""-m gpu: the recorded ops of the SimpleConvNet training step (csrc/train_resnet.inc sc_walk), ONE op at a time through the training
step's own launch code (dyf_op_train_f32), against float64 torch on the CPU -- in the manner of tests/test_gpu_train_ops.py.

NORM_ACT with DYF_TOP_ACT_GELU / DYF_TOP_RESIDUAL: SimpleConvNet's block behind its conv (BatchNorm2d -> FiLM -> exact GELU -> Dropout
-> + block input, simple_conv_net.py:41-54) in the fused norm kernels of csrc/train.hip -- the instantiations with GELU and the
residual operand (t_norm_fwd_ext / t_norm_fwd4_ext, t_norm_bwd_sums<.., true>, t_norm_bwd_apply / _apply4<true>).  Batch and running
statistics, with and without FiLM, with and without the residual, at 8 / 24 / 64 channels (24: no divisor of 256, the sum kernels'
one-thread-per-channel layout) on 1 x 1, 3 x 5 and 10 x 10 planes (10 x 10: the spring-mesh grid) and on one 65 x 65 plane (more
than one workgroup per sample in the sum kernels).  Dropout from the engine's generator with the masks rebuilt on the host
(tests/rng_host.py), and from an injected keep mask (the forward alone runs).  The updated running statistics are compared like a
gradient; parameter gradients accumulate over two calls.

CONV forward, data gradient and weight gradient at the walk's shapes: 9 -> 64 (the first layer: plain kernels forward and for the data
gradient), 64 -> 64 (the fp32 matrix-core kernel) and 8 -> 8 (the fixtures' width), kernel / padding 9/4, 7/3, 5/2, 3/1, on 10 x 10 and
10 x 6 grids (most taps of a 9 x 9 kernel fall outside the plane; the non-square plane catches a swapped axis), nb = 1 and 4.

Bound: rel-RMS <= 1e-5 per compared tensor against float64 (tests/train_op_refs.py TOL).  A tensor whose float64 value is zero (RMS
below 1e-12 of the op's other gradients) is compared absolutely against 1e-5 x the RMS of the op's other gradients, as
tests/test_gpu_train_ops.py describes."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import dyffusion_amd as D
from tests import rng_host as R
from tests.gpu_common import DEV
from tests.helpers import rel_rms
from tests.scn_train_refs import gelu_erf
from tests.train_op_refs import ROW_OFFSET, SEED, TOL

pytestmark = pytest.mark.gpu
ZERO = 1e-12
EPS = 1e-5


@pytest.fixture(scope="module")
def eng():
    cfg = D.net_config(in_channels=3, cond_channels=0, out_channels=3, dim=64, upsample_dims=[64, 64])
    e = D.HipEngine(cfg, cfg, 16, 16, max_batch=4, use_graph=False)
    e.train_set_precision(32)
    e.set_row_offset(ROW_OFFSET)
    yield e
    e.close()


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def compare(tag, got, want):
    errs = {}
    for k, w in want.items():
        assert bool(torch.isfinite(got[k]).all()), k
        others = [v.reshape(-1) for n, v in want.items() if n != k and n.startswith("d")]
        if others and rms(w) <= ZERO * rms(torch.cat(others)):
            errs[k] = float(got[k].abs().max()) / rms(torch.cat(others))
            print(f"{tag}: {k} is zero in float64")
        else:
            errs[k] = rel_rms(got[k].reshape(w.shape), w)
    worst = max(errs, key=errs.get)
    print(f"{tag}: max err {errs[worst]:.3e} ({worst})")
    assert errs[worst] <= TOL, errs
    return errs


def _gen(*key):
    return torch.Generator().manual_seed(sum((i + 1) * 7919 * (int(v) + 13) for i, v in enumerate(key)) % (2 ** 31))


def norm_case(nb, h, w, C, film, res, key):
    g = _gen(nb, h, w, C, film, res, key)
    rn = lambda *s: torch.randn(*s, generator=g)
    return dict(z=1.5 * rn(nb, h, w, C) + 0.3, ss=0.5 * rn(nb, 2 * C) if film else None, r=rn(nb, h, w, C) if res else None,
                gamma=1.0 + 0.1 * rn(C), beta=0.05 * rn(C), rm=0.1 * rn(C), rv=0.5 + torch.rand(C, generator=g), dout=rn(nb, h, w, C))


def norm_ref(c, running, keep, p, dtype=torch.float64):
    """BatchNorm2d (batch or running statistics) -> FiLM -> exact GELU -> keep / (1 - p) -> + r, NHWC; gradients by torch.autograd."""
    leaf = lambda t: None if t is None else t.to(dtype).clone().requires_grad_(True)
    z, ss, r, gamma, beta = leaf(c["z"]), leaf(c["ss"]), leaf(c["r"]), leaf(c["gamma"]), leaf(c["beta"])
    rm, rv = c["rm"].to(dtype), c["rv"].to(dtype)
    C = z.shape[-1]
    if running:
        mean, var, nrm, nrv = rm, rv, rm, rv
    else:
        mean = z.mean((0, 1, 2))
        var = ((z - mean) ** 2).mean((0, 1, 2))
        n = z.numel() // C
        nrm = 0.9 * rm + 0.1 * mean.detach()
        nrv = 0.9 * rv + 0.1 * var.detach() * (n / (n - 1) if n > 1 else 1.0)
    u = (z - mean) / torch.sqrt(var + EPS) * gamma + beta
    if ss is not None:
        u = u * (1 + ss[:, None, None, :C]) + ss[:, None, None, C:]
    y = gelu_erf(u)
    if keep is not None:
        y = y * keep.to(dtype) * (1.0 / (1.0 - p))
    if r is not None:
        y = y + r
    (y * c["dout"].to(dtype)).sum().backward()
    out = dict(y=y.detach(), dz=z.grad, dgamma=gamma.grad, dbeta=beta.grad, running_mean=nrm, running_var=nrv)
    if ss is not None:
        out["dss"] = ss.grad
    if r is not None:
        out["dr"] = r.grad
    return out


def engine_keep(nb, h, w, C, p):
    rows = [R.row_mask_nhwc((h, w, C), p, SEED, 0, 0, ROW_OFFSET + b) for b in range(nb)]
    return torch.from_numpy(np.stack(rows).astype(np.float64))


def run_norm(eng, c, running, p, mask=None, grads_in=None):
    ins = [c["z"].to(DEV)] + ([c["ss"].to(DEV)] if c["ss"] is not None else [])
    if p > 0 and mask is None:
        eng.seed(SEED)
    r = eng.op_train("norm_act", ins, [c["gamma"], c["beta"], c["rm"], c["rv"]], c["dout"].to(DEV), grads_in, p=p, act="gelu", running=running,
                     mask=None if mask is None else mask.to(DEV), residual=None if c["r"] is None else c["r"].to(DEV))
    got = dict(y=r["y"].cpu(), running_mean=r["dparams"][2], running_var=r["dparams"][3])
    if mask is None:
        names = ["dz"] + (["dss"] if c["ss"] is not None else []) + (["dr"] if c["r"] is not None else [])
        assert len(r["dinputs"]) == len(names)
        got.update({n: t.cpu() for n, t in zip(names, r["dinputs"])})
        got.update(dgamma=r["dparams"][0], dbeta=r["dparams"][1])
    return got


PLANES = [(3, 1, 1), (3, 3, 5), (3, 10, 10)]


@pytest.mark.parametrize("running", [False, True], ids=["batch", "running"])
@pytest.mark.parametrize("C", [8, 24, 64])
@pytest.mark.parametrize("plane", PLANES, ids=lambda s: "x".join(map(str, s)))
def test_norm_act_gelu_residual(eng, running, C, plane):
    nb, h, w = plane
    for film in (False, True):
        for res in (False, True):
            p = 0.25 if (film != res or (h, w) == (10, 10)) else 0.0  # generator dropout on most cases, none on the others
            c = norm_case(nb, h, w, C, film, res, running)
            keep = engine_keep(nb, h, w, C, p) if p > 0 else None
            want = norm_ref(c, running, keep, p)
            got = run_norm(eng, c, running, p)
            assert sorted(got) == sorted(want)
            compare(f"norm_act gelu {'running' if running else 'batch'} C={C} {nb}x{h}x{w} film={film} res={res} p={p}", got, want)


def test_norm_act_gelu_residual_on_a_65x65_plane(eng):
    for running in (False, True):
        c = norm_case(1, 65, 65, 64, True, True, running)
        keep = engine_keep(1, 65, 65, 64, 0.1)
        got, want = run_norm(eng, c, running, 0.1), norm_ref(c, running, keep, 0.1)
        compare(f"norm_act gelu 65x65 running={running}", got, want)


@pytest.mark.parametrize("C", [8, 24])
def test_norm_act_gelu_with_an_injected_mask_runs_the_forward(eng, C):
    nb, h, w, p = 3, 10, 10, 0.3
    for running in (False, True):
        for res in (False, True):
            c = norm_case(nb, h, w, C, True, res, 7)
            mask = (torch.rand(nb, h, w, C, generator=_gen(C, res)) >= p).to(torch.uint8)
            want = norm_ref(c, running, mask.double(), p)
            got = run_norm(eng, c, running, p, mask=mask)
            compare(f"norm_act gelu mask C={C} running={running} res={res}", got, {k: want[k] for k in got})


def test_norm_act_gelu_parameter_gradients_accumulate_over_two_calls(eng):
    nb, h, w, C, p = 3, 10, 10, 24, 0.25
    c = norm_case(nb, h, w, C, True, True, 3)
    want = norm_ref(c, False, engine_keep(nb, h, w, C, p), p)
    first = run_norm(eng, c, False, p)
    gin = [first["dgamma"], first["dbeta"], torch.zeros(C), torch.zeros(C)]
    second = run_norm(eng, c, False, p, grads_in=gin)  # the same masks: the generator is re-seeded
    compare("norm_act gelu, second call onto the first call's gradients",
            dict(dgamma=second["dgamma"], dbeta=second["dbeta"], dz=second["dz"]), dict(dgamma=2 * want["dgamma"], dbeta=2 * want["dbeta"], dz=want["dz"]))


@pytest.mark.parametrize("k", [9, 7, 5, 3])
@pytest.mark.parametrize("chan", [(9, 64), (64, 64), (8, 8)], ids=lambda c: f"{c[0]}to{c[1]}")
def test_conv_at_the_walks_shapes(eng, chan, k):
    cin, cout = chan
    pad = (k - 1) // 2
    for (h, w) in ((10, 10), (10, 6)):
        for nb in (1, 4):
            g = _gen(cin, cout, k, h, w, nb)
            x, wt = torch.randn(nb, h, w, cin, generator=g), torch.randn(cout, cin, k, k, generator=g) / (k * cin ** 0.5)
            b, dout = 0.1 * torch.randn(cout, generator=g), torch.randn(nb, h, w, cout, generator=g)
            xd, wd, bd = (t.double().requires_grad_(True) for t in (x, wt, b))
            y = F.conv2d(xd.permute(0, 3, 1, 2), wd, bd, padding=pad).permute(0, 2, 3, 1)
            (y * dout.double()).sum().backward()
            want = dict(y=y.detach(), dx=xd.grad, dw=wd.grad, db=bd.grad)
            r = eng.op_train("conv", [x.to(DEV)], [wt, b], dout.to(DEV), k=k, stride=1, pad=pad)
            got = dict(y=r["y"].cpu(), dx=r["dinputs"][0].cpu(), dw=r["dparams"][0], db=r["dparams"][1])
            compare(f"conv {cin}->{cout} k={k} {nb}x{h}x{w}", got, want)
