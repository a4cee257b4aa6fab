"""-m gpu: dyf_power_spectrum (power_spectrum_kernel) against the float64 full-spectrum reference of tests/power_spectrum_refs.py within
its derived bound on every case of refs.CASES: the four planes and the totals; direct writes, repeatability and both builds, Parseval,
the accumulator and the refusals, the metrics surface and the experiment's keys."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import power_spectrum_refs as refs
from tests.test_gpu_ensemble_size_metrics import _batches, _engine, _tiny_experiment

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.contiguous().view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _device_inputs(c):
    """The case in the form it names: one (N, B, C, H, W) tensor (for `strided` a view of a stack twice as large, whose other half is
    NaN: it must not be read), or lists of `segs` tensors."""
    x, y = (torch.from_numpy(np.array(a)) for a in refs.inputs(c.name))
    if c.form == "list":
        return [x[s].cuda() for s in range(c.segs)], [y[s].cuda() for s in range(c.segs)]
    assert c.segs == 1
    if not c.strided:
        return x[0].cuda(), y[0].cuda()
    big = torch.full((c.n, 2) + tuple(x.shape[2:]), float("nan"))
    big[:, 1] = x[0]
    view = big.cuda()[:, 1]
    assert not view.is_contiguous() and view.stride(0) == 2 * y[0].numel()
    return view, y[0].cuda()


def _run(eng, c, **kw):
    p, t = _device_inputs(c)
    return eng.power_spectrum(p, t, window=c.window, **kw)


@pytest.mark.parametrize("name", list(refs.CASES))
def test_cases_match_the_reference_within_the_bound(name):
    c = refs.CASES[name]
    eng = _engine()
    got = _run(eng, c)
    planes = got["planes"]
    assert got["n_bins"] == c.n_bins and planes.dtype == torch.float64 and tuple(planes.shape) == (c.segs, c.c, 4, c.n_bins + 1)
    for i, key in enumerate(refs.PLANES):
        assert tuple(got[key].shape) == (c.segs, c.c, c.n_bins) and bool(torch.equal(got[key], planes[:, :, i, :c.n_bins]))
    assert tuple(got["total"].shape) == (c.segs, c.c, 4) and bool(torch.equal(got["total"], planes[..., c.n_bins]))
    host = planes.cpu().numpy()
    ref, bound = refs.reference(name)
    with np.errstate(divide="ignore", invalid="ignore"):
        per_plane = [float(np.max(np.abs(host[:, :, i] - ref[:, :, i]) / bound[:, :, i])) for i in range(4)]
    print(f"{name}: error / bound per plane (spread, mean, target, error) = {per_plane}, worst = {refs.worst_ratio(host, name):.3e}")
    assert refs.worst_ratio(host, name) <= 1.0
    # the same call straight into sentinel-filled buffers: every entry is overwritten, with the same bits
    sentinel = -12345.0
    out = torch.full(tuple(planes.shape), sentinel, dtype=torch.float64).cuda()
    p, t = _device_inputs(c)
    plist, tlist = ([p], [t]) if torch.is_tensor(p) else (p, t)
    stride = plist[0].stride(0) if c.n > 1 else t.numel() if torch.is_tensor(t) else tlist[0].numel()
    eng._check(eng._lib.dyf_power_spectrum(eng._h, c.segs, (C.c_void_p * c.segs)(*[q.data_ptr() for q in plist]),
                                           (C.c_void_p * c.segs)(*[q.data_ptr() for q in tlist]), c.n, stride, c.b, c.c, c.h, c.w,
                                           int(c.window == "hann"), out.data_ptr(), None, eng._stream()))
    torch.cuda.synchronize()
    assert not bool((out == sentinel).any()) and _same_bits(out, planes)
    # Parseval: the target's total is mean(y^2) of the (tapered) target
    y = refs.inputs(name)[1].astype(np.float64)
    win = np.outer(refs.hann(c.h), refs.hann(c.w)) if c.window == "hann" else 1.0
    assert np.all(np.abs(host[:, :, 2, c.n_bins] - ((y * win) ** 2).mean(axis=(1, 3, 4))) <= bound[:, :, 2, c.n_bins])


def test_two_calls_and_both_builds_are_bit_equal():
    import dyffusion_amd as D

    eng = _engine()
    net = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=1, num_output_channels=1,
                 num_conditional_channels=0, spatial_shape=(16, 16))
    cfg = net.engine_net_config()
    half = D.HipEngine(cfg, cfg, height=16, width=16, max_batch=1, use_graph=False, dtype="fp16")
    assert half._lib.dyf_dtype() == 1 and eng._lib.dyf_dtype() == 0
    for name in ("5x3", "33x34", "61x42"):
        c = refs.CASES[name]
        first, second, other = _run(eng, c)["planes"], _run(eng, c)["planes"], _run(half, c)["planes"]
        assert _same_bits(first, second) and _same_bits(first, other)


def test_list_form_and_tensor_form_agree_and_segments_are_independent():
    c = refs.CASES["33x34"]
    eng = _engine()
    plist, tlist = _device_inputs(c)
    both = eng.power_spectrum(plist, tlist)["planes"]
    for s in range(c.segs):
        assert _same_bits(eng.power_spectrum(plist[s], tlist[s])["planes"], both[s:s + 1])
    assert _same_bits(eng.power_spectrum(plist[::-1], tlist[::-1])["planes"], both.flip(0))


def test_accum_adds():
    c = refs.CASES["16x30"]
    eng = _engine()
    first = _run(eng, c)["planes"]
    start = torch.arange(first.numel(), dtype=torch.float64).reshape(first.shape).cuda()
    accum = start.clone()
    second = _run(eng, c, accum=accum)["planes"]
    assert _same_bits(first, second) and _same_bits(accum, start + first)
    _run(eng, c, accum=accum)
    assert _same_bits(accum, start + first + first)
    with pytest.raises(ValueError):
        _run(eng, c, accum=torch.zeros(tuple(first.shape)).cuda())  # fp32 accumulator
    with pytest.raises(ValueError):
        _run(eng, c, accum=torch.zeros(1, c.c, 4, c.n_bins, dtype=torch.float64).cuda())


def test_refusals():
    from dyffusion_amd import _lib as L

    eng = _engine()
    z = torch.zeros
    assert tuple(eng.power_spectrum(z(2, 1, 1, 2, 3).cuda(), z(1, 1, 2, 3).cuda())["planes"].shape) == (1, 1, 4, 3)
    with pytest.raises(ValueError, match="at least 2"):
        eng.power_spectrum(z(2, 1, 1, 1, 8).cuda(), z(1, 1, 1, 8).cuda())  # H = 1
    with pytest.raises(NotImplementedError, match="DYF_SPECTRUM_MAX_DIM"):
        eng.power_spectrum(z(1, 1, 1, 2, 1025).cuda(), z(1, 1, 2, 1025).cuda())  # W = 1025
    with pytest.raises(NotImplementedError, match=r"\[1, 256\]"):
        eng.power_spectrum(z(257, 1, 1, 2, 2).cuda(), z(1, 1, 2, 2).cuda())  # N = 257
    with pytest.raises(ValueError, match="window"):
        eng.power_spectrum(z(2, 1, 1, 4, 4).cuda(), z(1, 1, 4, 4).cuda(), window="hamming")
    with pytest.raises(ValueError, match="GPU tensors"):
        eng.power_spectrum(z(2, 1, 1, 4, 4), z(1, 1, 4, 4))  # CPU tensors
    with pytest.raises(ValueError):
        eng.power_spectrum(z(2, 1, 4, 4).cuda(), z(1, 4, 4).cuda())  # not (N, B, C, H, W)
    # the C ABI's own checks, with counts far beyond the dummy tables: refused before anything is launched or read
    p, t = z(2, 1, 1, 4, 4).cuda(), z(1, 1, 4, 4).cuda()
    out = torch.zeros(1, 1, 4, 4, dtype=torch.float64).cuda()
    tab = lambda x: (C.c_void_p * 1)(x.data_ptr())  # noqa: E731

    def call(nseg=1, n=2, stride=16, b=1, c=1, h=4, w=4, window=0, outp=None):
        return eng._lib.dyf_power_spectrum(eng._h, nseg, tab(p), tab(t), n, stride, b, c, h, w, window,
                                           out.data_ptr() if outp is None else outp, None, eng._stream())
    assert call() == L.DYF_OK
    assert call(window=2) == L.DYF_ERR_INVALID_ARGUMENT and call(window=-1) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(h=1, stride=4) == L.DYF_ERR_INVALID_ARGUMENT and call(w=1, stride=4) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(h=1025, stride=1 << 20) == L.DYF_ERR_UNSUPPORTED and call(w=1025, stride=1 << 20) == L.DYF_ERR_UNSUPPORTED
    assert call(n=257) == L.DYF_ERR_UNSUPPORTED and call(n=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(nseg=0) == L.DYF_ERR_INVALID_ARGUMENT and call(outp=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(stride=15) == L.DYF_ERR_INVALID_ARGUMENT and call(b=0) == L.DYF_ERR_INVALID_ARGUMENT
    for b, c, h, w in ((1 << 30, 1 << 30, 4, 4), (1 << 14, 1, 1024, 1024), (1 << 20, 8, 64, 64)):
        assert call(b=b, c=c, h=h, w=w, stride=1 << 62) == L.DYF_ERR_UNSUPPORTED, (b, c, h, w)
        assert b"2^27" in eng._lib.dyf_last_error(eng._h)
    torch.cuda.synchronize()
    assert call() == L.DYF_OK  # the engine is as usable as before
    torch.cuda.synchronize()


def test_metrics_surface():
    from dyffusion_amd import metrics as M

    eng = _engine()
    c = refs.CASES["70x70"]
    x, y = (torch.from_numpy(np.array(a)).cuda() for a in refs.inputs(c.name))
    got = M.evaluate_power_spectrum(x[0], y[0], eng)
    keys = {"spread", "mean", "target", "error", "total", "members", "spread_fair", "wavenumber", "spectral_ssr", "coherence", "lsd",
            "lsd_ens_mean", "n_bins"}
    assert set(got) == keys and got["n_bins"] == c.n_bins
    for k in ("spread", "mean", "target", "error", "members", "spread_fair", "spectral_ssr", "coherence"):
        assert got[k].is_cuda and got[k].dtype == torch.float64 and tuple(got[k].shape) == (c.c, c.n_bins), k
    assert tuple(got["total"].shape) == (c.c, 4) and tuple(got["lsd"].shape) == tuple(got["lsd_ens_mean"].shape) == (c.c,)
    assert bool(torch.equal(got["wavenumber"].cpu(), torch.arange(c.n_bins)))
    planes = eng.power_spectrum(x[0], y[0])["planes"]
    want = refs.derived(planes[0].cpu().numpy(), c.n)  # the same formulas in numpy on the same planes
    for k, v in want.items():
        assert got[k].cpu().numpy() == pytest.approx(v, rel=1e-12, nan_ok=True), k
    many = M.evaluate_power_spectrum([x[0], x[0]], [y[0], y[0]], eng, window="hann")
    assert tuple(many["spread"].shape) == (2, c.c, c.n_bins) and tuple(many["lsd"].shape) == (2, c.c)
    assert _same_bits(many["spread"][0], many["spread"][1])
    # every member equal to the target: the members' spectrum is the target's, to the bit
    same = M.evaluate_power_spectrum(y[0][None].expand(4, -1, -1, -1, -1), y[0], eng)
    assert float(same["lsd"].abs().max()) <= 1e-9 and float(same["spread"].abs().max()) == 0.0
    with pytest.raises(ValueError, match="GPU tensors"):
        M.evaluate_power_spectrum(x[0].cpu(), y[0].cpu(), eng)


def test_log_spectral_distances_tell_sharp_members_from_their_blurred_mean():
    """Members that carry the truth's large scales and independent noise with the statistics of the truth's small scales are singly
    as sharp as the truth while their mean blurs: lsd_ens_mean > lsd.  (Members that are the target ITSELF plus independent noise of
    variance s^2 go the other way by construction: E|X_m|^2 = |Y|^2 + s^2 per coefficient but E|Xbar|^2 = |Y|^2 + s^2 / N, so the
    mean's spectrum is the closer one; that ordering is asserted too.)"""
    from dyffusion_amd import metrics as M

    eng = _engine()
    g = torch.Generator().manual_seed(11)
    hh, ww = torch.meshgrid(torch.arange(40.0), torch.arange(36.0), indexing="ij")
    smooth = torch.cos(2 * np.pi * (hh / 40 + 2 * ww / 36))
    truth = (smooth + 0.3 * torch.randn(2, 1, 40, 36, generator=g)).cuda()
    members = smooth.cuda() + (0.3 * torch.randn(6, 2, 1, 40, 36, generator=g)).cuda()
    got = M.evaluate_power_spectrum(members, truth, eng)
    print("own small scales: lsd", got["lsd"].tolist(), "lsd_ens_mean", got["lsd_ens_mean"].tolist())
    assert bool((got["lsd_ens_mean"] > got["lsd"]).all())
    noisy = truth[None] + (0.3 * torch.randn(6, 2, 1, 40, 36, generator=g)).cuda()
    got = M.evaluate_power_spectrum(noisy, truth, eng)
    print("target + noise: lsd", got["lsd"].tolist(), "lsd_ens_mean", got["lsd_ens_mean"].tolist())
    assert bool((got["lsd_ens_mean"] < got["lsd"]).all())


N, T = 4, 3
BASE = {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("mse", "ssr", "crps")}


def test_power_spectrum_keys_of_the_validation_epoch():
    from dyffusion_amd.metrics import evaluate_power_spectrum

    exp = _tiny_experiment(N, False, power_spectrum=True)
    outs = [exp.validation_step(b, 0) for b in _batches(T)]
    got = exp.on_validation_epoch_end()
    new = {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("lsd", "lsd_ens_mean")}
    new |= {f"val/{N}ens_mems/t{k}/c{j}/lsd" for k in range(1, T + 1) for j in range(2)}
    assert set(got) == BASE | new
    assert all(isinstance(got[k], float) and np.isfinite(got[k]) and got[k] > 0 for k in new)
    # a batch-weighted sum of the batches' spectra is the spectrum of the pooled fields: the per-channel lsd of the pooled call
    for k in range(1, T + 1):
        preds = torch.cat([o[f"t{k}_preds"] for o in outs], dim=1)
        targets = torch.cat([o[f"t{k}_targets"] for o in outs], dim=0)
        want = evaluate_power_spectrum(preds, targets, exp.model._engine)["lsd"].cpu().numpy()
        assert [got[f"val/{N}ens_mems/t{k}/c{j}/lsd"] for j in range(2)] == pytest.approx(list(want), rel=1e-9)
    assert got[f"val/{N}ens_mems/avg/lsd"] == pytest.approx(sum(got[f"val/{N}ens_mems/t{k}/lsd"] for k in range(1, T + 1)) / T, rel=1e-12)
    # the flag off: the same fields to the bit, the parent's keys, and the values of this very epoch, bit for bit
    exp = _tiny_experiment(N, False)
    again = [exp.validation_step(b, 0) for b in _batches(T)]
    for o, p in zip(outs, again):
        assert set(o) == set(p) and all(bool(torch.equal(o[k], p[k])) for k in o if torch.is_tensor(o[k]))
    plain = exp.on_validation_epoch_end()
    print({k: (plain[k], got[k]) for k in sorted(BASE) if plain[k] != got[k]})
    assert set(plain) == BASE and all(plain[k] == got[k] for k in BASE)
    # the taper is passed through
    exp = _tiny_experiment(N, False, power_spectrum=True, spectrum_window="hann")
    for b in _batches(T):
        exp.validation_step(b, 0)
    tapered = exp.on_validation_epoch_end()
    assert set(tapered) == set(got) and tapered[f"val/{N}ens_mems/t1/lsd"] != got[f"val/{N}ens_mems/t1/lsd"]
