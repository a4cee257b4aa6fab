"""The grouped ensemble scores on the device (dyf_ensemble_scores, HipEngine.ensemble_scores, the mean_dims surface of
dyffusion_amd.metrics and the extended keys of the validation epoch) against the float64 reference of tests/ensemble_scores_refs.py
(oracle/metrics.py per group, the reference's NLL expression, np.corrcoef; pinned to the reference's own numbers by
tests/test_ensemble_scores_refs.py).  Inputs: the generator of tests/test_gpu_ensemble_size_metrics.py.

The work map: a workgroup's tile lies inside one (outer, group) slab of n_inner points; 256 points per tile up to 64 members,
fewer beyond (64 at 65 and at 130 members).  So inner 153 is one partial tile per slab, 513 leaves one point for the third tile,
256 fills a tile exactly, inner 1 makes every point a workgroup of its own.

Bounds: mse / ssr / crps rel 2e-5, the project's bound for these fp32 per-point expressions; nll |got - ref| <= 2e-5 x the mean
over the group's points of |nll_p| (fp32 per point as well, and the mean itself can be near zero); corr abs 1e-6 (the moments are
fp64; the ensemble mean under them is an fp32 sum of up to 130 members in sequence, or of 2000 in 64 shares).  One member: nll is NaN and ssr exactly 0."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ensemble_scores_refs as refs
from tests.test_gpu_ensemble_size_metrics import _as_lists, _batches, _engine, _inputs, _tiny_experiment

pytestmark = pytest.mark.gpu
REL = 2e-5
CORR_ABS = 1e-6


def _bits(x):
    return x.contiguous().view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))  # NaNs included


def _check(got, ref, scale, n, what=""):
    """got: (5, T, G) device tensor or array; ref: the same shape, scale: (T, G), both from tests/ensemble_scores_refs.py."""
    got = got.cpu().numpy() if torch.is_tensor(got) else np.asarray(got)
    assert got.shape == ref.shape and got.dtype == np.float64
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = [float(np.nanmax(np.abs(got[i] - ref[i]) / np.abs(ref[i]))) for i in (0, 2)]
        print(what, "worst rel diff mse, crps:", rel, "ssr:", float(np.nanmax(np.abs(got[1] - ref[1]) / np.maximum(np.abs(ref[1]), 1e-300))),
              "nll / scale:", float(np.nanmax(np.abs(got[3] - ref[3]) / scale)) if n > 1 else "nan", "corr abs:",
              float(np.nanmax(np.abs(got[4] - ref[4]))))
    for i in (0, 2):
        assert got[i] == pytest.approx(ref[i], rel=REL, abs=0.0), refs.ROWS[i]
    if n == 1:
        assert np.all(got[1] == 0.0) and np.all(ref[1] == 0.0) and np.all(np.isnan(got[3])) and np.all(np.isnan(ref[3]))
    else:
        assert got[1] == pytest.approx(ref[1], rel=REL, abs=0.0)
        assert np.all(np.abs(got[3] - ref[3]) <= REL * scale), (got[3], ref[3], scale)
    assert np.all(np.isfinite(ref[4])) and np.all(np.abs(got[4] - ref[4]) <= CORR_ABS), (got[4], ref[4])


def _kept(shape, axes):
    """The (outer, groups, inner) of keeping the contiguous `axes` of a segment's `shape`."""
    a, b = axes[0], axes[-1]
    return (int(np.prod(shape[:a], dtype=np.int64)), int(np.prod(shape[a:b + 1], dtype=np.int64)), int(np.prod(shape[b + 1:], dtype=np.int64)))


CASES = [  # N, segments, a segment's target shape, kept axes
    (8, 2, (2, 3, 17, 9), (1,)),      # per channel: inner 153, one partial tile per slab
    (8, 1, (2, 2, 19, 27), (1,)),     # inner 513: the last tile of a slab holds 1 point
    (20, 3, (3, 2, 16, 16), (1,)),    # inner exactly 256
    (8, 2, (4, 3, 5, 7), (0,)),       # per sample: slabs of 105 points, the odd ones only 4-byte aligned
    (8, 1, (3, 4, 5, 7), (0, 1)),     # per sample and channel
    (4, 1, (3, 5), (1,)),             # the last axis: inner 1
    (64, 2, (2, 165), (0,)),          # the LDS edge of the one-thread-per-point form
    (65, 2, (2, 165), (0,)),          # the first tiled case
    (130, 1, (1, 2, 11, 23), (1,)),
    (2, 1, (1, 2, 300), (1,)),
    (1, 1, (2, 3, 8, 8), (1,)),       # one member
]
_REF = {}


def _case(n, t, shape, axes):
    """Inputs and references of a case, computed once."""
    key = (n, t, shape, axes)
    if key not in _REF:
        preds, truth = _inputs(n, t, shape)
        gs = _kept(shape, axes) if axes is not None else None
        _REF[key] = (preds, truth, gs, refs.segment_reference(preds.numpy(), truth.numpy(), gs), refs.nll_scale(preds.numpy(), truth.numpy(), gs))
    return _REF[key]


@pytest.mark.parametrize("n,t,shape,axes", CASES, ids=[f"N{c[0]}-T{c[1]}-{'x'.join(map(str, c[2]))}-keep{''.join(map(str, c[3]))}" for c in CASES])
def test_groups_match_the_reference(n, t, shape, axes):
    eng = _engine()
    preds, truth, gs, ref, scale = _case(n, t, shape, axes)
    assert ref.shape == (5, t, gs[1])
    if shape == (4, 3, 5, 7):
        assert gs == (1, 4, 105) and (4 * 105) % 8 == 4
    pl, tl = _as_lists(preds, truth)
    got = eng.ensemble_scores(pl, tl, group_shape=gs)
    assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (5, t, gs[1])
    _check(got, ref, scale, n, "grouped")
    # the strided layout: one (N, S, ...) tensor read in place, the same bits; and again: identical calls are bitwise equal
    assert _same_bits(eng.ensemble_scores(preds.cuda(), truth.cuda(), group_shape=gs), got)
    assert _same_bits(eng.ensemble_scores(pl, tl, group_shape=gs), got)
    # a segment alone gives the bits it has among its neighbours
    for s in range(t):
        assert _same_bits(eng.ensemble_scores([pl[s]], [tl[s]], group_shape=gs)[:, 0], got[:, s]), s
    # group g is the pooled call on a contiguous copy of its points
    outer, groups, inner = gs
    for g in range(groups):
        gp = [p.reshape(n, outer, groups, inner)[:, :, g].contiguous() for p in pl]
        gt = [y.reshape(outer, groups, inner)[:, g].contiguous() for y in tl]
        alone = eng.ensemble_scores(gp, gt).cpu().numpy()
        assert tuple(alone.shape) == (5, t, 1)
        assert alone[:, :, 0] == pytest.approx(got[:, :, g].cpu().numpy(), rel=1e-12, abs=0.0, nan_ok=True), g


# 1 / N is inexact for 6, 20, 65, 130 and 2000 members: there a product contracted differently in the two entries would show.
# 2000 members on 7 points: 4 points per workgroup, the 64 shares of a point fill a wave (the share-order walks run to k = 63).
@pytest.mark.parametrize("n,t,shape", [(8, 2, (2, 3, 17, 9)), (65, 2, (2, 165)), (1, 1, (2, 3, 8, 8)), (6, 2, (4, 3, 5, 7)),
                                       (20, 3, (3, 2, 16, 16)), (130, 1, (1, 2, 11, 23)), (2000, 1, (7,))],
                         ids=["N8", "N65", "N1", "N6-odd", "N20", "N130", "N2000"])
def test_pooled(n, t, shape):
    eng = _engine()
    preds, truth, _, ref, scale = _case(n, t, shape, None)
    pl, tl = _as_lists(preds, truth)
    got = eng.ensemble_scores(pl, tl)  # group_shape=None
    assert tuple(got.shape) == (5, t, 1)
    _check(got, ref, scale, n, "pooled")
    points = truth[0].numel()
    assert _same_bits(eng.ensemble_scores(pl, tl, group_shape=(1, 1, points)), got)
    assert _same_bits(eng.ensemble_scores(preds.cuda(), truth.cuda()), got)
    # planes 0-2 are dyf_trajectory_metrics bit for bit: the same per-point helper, tiles, block sum and finish order
    assert _same_bits(got[:3, :, 0], eng.trajectory_metrics(pl, tl))


def test_permuting_the_channels_permutes_the_outputs():
    eng = _engine()
    preds, truth = _inputs(8, 2, (2, 3, 17, 9))
    perm = [2, 0, 1]
    a = eng.ensemble_scores(preds.cuda(), truth.cuda(), group_shape=(2, 3, 153))
    b = eng.ensemble_scores(preds[:, :, :, perm].contiguous().cuda(), truth[:, :, perm].contiguous().cuda(), group_shape=(2, 3, 153))
    assert _same_bits(b, a[:, :, perm]) and not _same_bits(b, a)


def test_constant_groups_have_a_nan_correlation_as_numpy():
    eng = _engine()
    preds, truth = _inputs(8, 1, (3, 3, 11, 31))  # inner 341: two tiles per slab, three slabs per group
    truth[:, :, 1] = 0.3            # channel 1: constant targets
    # channel 2: every member the same constant, so the ensemble means are constant; eight times -1.75 add exactly in fp32: var = 0
    preds[:, :, :, 2] = -1.75
    gs = (3, 3, 341)
    ref = refs.segment_reference(preds.numpy(), truth.numpy(), gs)
    assert np.isfinite(ref[4, 0, 0]) and np.isnan(ref[4, 0, 1]) and np.isnan(ref[4, 0, 2]) and np.isnan(ref[3, 0, 2])
    got = eng.ensemble_scores(preds.cuda(), truth.cuda(), group_shape=gs).cpu().numpy()
    print("corr:", got[4], "nll:", got[3])
    assert abs(got[4, 0, 0] - ref[4, 0, 0]) <= CORR_ABS and np.isnan(got[4, 0, 1]) and np.isnan(got[4, 0, 2])
    assert np.isnan(got[3, 0, 2]) and got[1, 0, 2] == 0.0  # zero variance: NaN nll, zero spread
    assert got[:3, 0, :2] == pytest.approx(ref[:3, 0, :2], rel=REL, abs=0.0) and got[0, 0, 2] == pytest.approx(ref[0, 0, 2], rel=REL)
    # pooled over the three channels nothing is constant
    pooled = eng.ensemble_scores(preds.cuda(), truth.cuda()).cpu().numpy()
    assert abs(pooled[4, 0, 0] - refs.segment_reference(preds.numpy(), truth.numpy())[4, 0, 0]) <= CORR_ABS


def test_accum_adds_and_calls_back_to_back_share_the_pointer_table():
    eng = _engine()
    pa, ta = _inputs(6, 4, (2, 3, 50), seed=1)
    pb, tb = _inputs(6, 4, (2, 3, 50), seed=2)
    la, lb = _as_lists(pa, ta), _as_lists(pb, tb)
    gs = (2, 3, 50)
    acc = torch.zeros(5, 4, 3, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    ga = eng.ensemble_scores(*la, group_shape=gs, accum=acc)  # nothing waits in between; trajectory_metrics uses the same table
    tr = eng.trajectory_metrics(*lb)
    gb = eng.ensemble_scores(*lb, group_shape=gs, accum=acc)
    _check(ga, refs.segment_reference(pa.numpy(), ta.numpy(), gs), refs.nll_scale(pa.numpy(), ta.numpy(), gs), 6)
    _check(gb, refs.segment_reference(pb.numpy(), tb.numpy(), gs), refs.nll_scale(pb.numpy(), tb.numpy(), gs), 6)
    assert torch.equal(acc, ga + gb) and not torch.equal(ga, gb)
    assert torch.equal(tr, eng.trajectory_metrics(*lb))


def test_form_is_noted_in_the_form_log():
    eng = _engine()
    preds, truth = _inputs(5, 2, (2, 35))
    eng.form_log(True)
    try:
        eng.ensemble_scores(preds.cuda(), truth.cuda(), group_shape=(1, 2, 35))
        eng.ensemble_scores(*_as_lists(*_inputs(65, 1, (70,))))
        log = eng.form_log_read()
    finally:
        eng.form_log(False)
    assert log.get("ensemble_scores_kernel:slab") == {0: 1}
    assert log.get("ensemble_scores_kernel:slab+tiled") == {0: 1}


def test_argument_checks():
    eng = _engine()
    z = torch.zeros
    p, t = z(3, 2, 12).cuda(), z(2, 12).cuda()
    for gs in ((1, 5, 2), (2, 3, 4), (0, 1, 12), (1, -1, -12), (12,), (1, 1.5, 8), "abc"):  # a product that is not 12, and worse
        with pytest.raises(ValueError):
            eng.ensemble_scores(p, t, group_shape=gs)
    assert tuple(eng.ensemble_scores(p, t, group_shape=[2, 3, 2]).shape) == (5, 2, 3)
    with pytest.raises(ValueError):
        eng.ensemble_scores([], [])
    with pytest.raises(ValueError):
        eng.ensemble_scores(z(3, 2, 5).cuda(), z(2, 4).cuda())
    with pytest.raises(ValueError):
        eng.ensemble_scores([z(3, 5)], [z(5)])  # CPU tensors
    with pytest.raises(ValueError):
        eng.ensemble_scores(p, t, group_shape=(1, 3, 4), accum=torch.zeros(5, 2, 4, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        eng.ensemble_scores(p, t, group_shape=(1, 3, 4), accum=torch.zeros(5, 2, 3).cuda())  # fp32 accumulator
    big = 1 << 24  # one point per workgroup: one workgroup more than a segment can have
    with pytest.raises(NotImplementedError, match=r"2\^24 - 1"):
        eng.ensemble_scores(z(1, 1, big).cuda(), z(1, big).cuda(), group_shape=(big, 1, 1))
    # the C ABI's own checks
    from dyffusion_amd import _lib as L
    p, t = z(3, 12).cuda(), z(12).cuda()
    out = torch.zeros(5, 1, 12, dtype=torch.float64).cuda()
    tab = lambda x: (C.c_void_p * 1)(x.data_ptr())  # noqa: E731

    def call(nseg=1, n=3, points=12, stride=12, gs=(2, 3, 2), outp=None, preds=None):
        return eng._lib.dyf_ensemble_scores(eng._h, nseg, preds if preds is not None else tab(p), tab(t), n, points, stride, gs[0], gs[1],
                                            gs[2], out.data_ptr() if outp is None else outp, None, eng._stream())
    assert call() == L.DYF_OK
    assert call(nseg=0) == L.DYF_ERR_INVALID_ARGUMENT and call(nseg=65536) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(n=0) == L.DYF_ERR_INVALID_ARGUMENT and call(n=15361) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(points=0, stride=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(stride=11) == L.DYF_ERR_INVALID_ARGUMENT  # member_stride < n_points
    assert call(outp=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(preds=(C.c_void_p * 1)(None)) == L.DYF_ERR_INVALID_ARGUMENT
    for gs in ((2, 3, 3), (1, 5, 2), (0, 3, 4), (3, 0, 4), (3, 4, 0), (-3, -4, 1), (1, 1, 11), (1 << 62, 4, 1)):
        assert call(gs=gs) == L.DYF_ERR_INVALID_ARGUMENT, gs
    assert b"n_points" in eng._lib.dyf_last_error(eng._h)
    assert call(points=big, stride=big, gs=(big, 1, 1)) == L.DYF_ERR_UNSUPPORTED  # refused before anything is launched
    assert b"2^24 - 1" in eng._lib.dyf_last_error(eng._h)
    torch.cuda.synchronize()


def test_metrics_surface():
    from dyffusion_amd import metrics as M

    eng = _engine()
    n, b, c, h, w = 6, 3, 2, 9, 7
    preds, truth = _inputs(n, b, (c, h, w))  # (N, B, C, H, W), (B, C, H, W)
    dp, dt = preds.cuda(), truth.cuda()
    pn, tn = preds.numpy(), truth.numpy()
    pooled = refs.pooled_reference(pn, tn)
    pooled_scale = refs.nll_scale(pn[:, None], tn[None])[0, 0]
    per_c, per_c_scale = refs.group_reference(pn, tn, (b, c, h * w)), refs.nll_scale(pn[:, None], tn[None], (b, c, h * w))[0]
    per_s, per_s_scale = refs.group_reference(pn, tn, (1, b, c * h * w)), refs.nll_scale(pn[:, None], tn[None], (1, b, c * h * w))[0]
    per_sc = refs.group_reference(pn, tn, (1, b * c, h * w))

    def dev(x, shape):
        assert torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float64 and tuple(x.shape) == shape
        return x.cpu().numpy()

    # all axes: host floats
    got = M.evaluate_ensemble_scores(dp, dt, eng)
    assert list(got) == list(M.SCORE_ROWS) and all(isinstance(v, float) for v in got.values())
    _check(np.array([got[m] for m in M.SCORE_ROWS]).reshape(5, 1, 1), pooled.reshape(5, 1, 1), pooled_scale.reshape(1, 1), n, "surface")
    assert got == M.evaluate_ensemble_scores(dp, dt, eng, mean_dims=(0, 1, 2, 3))
    assert M.evaluate_ensemble_mse(dp, dt, eng) == got["mse"] and M.evaluate_ensemble_spread_skill_ratio(dp, dt, eng) == got["ssr"]
    assert M.evaluate_ensemble_nll(dp, dt, eng) == got["nll"] and M.evaluate_ensemble_corr(dp, dt, eng) == got["corr"]
    assert M.evaluate_ensemble_crps(dp, dt, eng) == got["crps"]
    old = M.evaluate_ensemble_prediction(dp, dt, eng)  # ensemble_metrics_kernel: each within REL of the reference
    assert all(got[m] == pytest.approx(old[m], rel=2 * REL) for m in ("mse", "ssr", "crps"))
    # per channel / per sample / per sample and channel: device tensors
    got = M.evaluate_ensemble_scores(dp, dt, eng, mean_dims=(0, 2, 3))
    _check(np.stack([dev(got[m], (c,)) for m in M.SCORE_ROWS])[:, None], per_c[:, None], per_c_scale[None], n, "per channel")
    assert _same_bits(M.evaluate_ensemble_mse(dp, dt, eng, mean_dims=(0, 2, 3)), got["mse"])
    assert _same_bits(M.evaluate_ensemble_mse(dp, dt, eng, mean_dims=(0, -2, -1)), got["mse"])
    got = M.evaluate_ensemble_scores(dp, dt, eng, mean_dims=(1, 2, 3))
    _check(np.stack([dev(got[m], (b,)) for m in M.SCORE_ROWS])[:, None], per_s[:, None], per_s_scale[None], n, "per sample")
    assert _same_bits(M.evaluate_ensemble_crps(dp, dt, eng, mean_over_samples=False), got["crps"])
    assert _same_bits(M.evaluate_ensemble_nll(dp, dt, eng, mean_dims=(1, 2, 3)), got["nll"])
    assert _same_bits(M.evaluate_ensemble_spread_skill_ratio(dp, dt, eng, mean_dims=(1, 2, 3)), got["ssr"])
    old = M.evaluate_ensemble_prediction(dp, dt, eng, mean_over_samples=False)  # trajectory_metrics_kernel
    assert all(old[m].cpu().numpy() == pytest.approx(got[m].cpu().numpy(), rel=1e-12) for m in ("mse", "ssr", "crps"))
    nll = dev(M.evaluate_ensemble_nll(dp, dt, eng, mean_dims=(2, 3)), (b, c))
    assert np.all(np.abs(nll.reshape(-1) - per_sc[3]) <= REL * refs.nll_scale(pn[:, None], tn[None], (1, b * c, h * w))[0])
    # a skill of the caller's: spread / skill (evaluation.py:112-119)
    spread_c = np.sqrt(pn.astype(np.float64).var(axis=0).mean(axis=(0, 2, 3)))
    ssr = dev(M.evaluate_ensemble_spread_skill_ratio(dp, dt, eng, skill_metric=2.0, mean_dims=(0, 2, 3)), (c,))
    assert ssr == pytest.approx(spread_c / 2.0, rel=REL)
    skill = torch.tensor([0.5, 4.0], dtype=torch.float64)
    for sk in (skill, skill.cuda(), skill.numpy()):
        ssr = dev(M.evaluate_ensemble_spread_skill_ratio(dp, dt, eng, skill_metric=sk, mean_dims=(0, 2, 3)), (c,))
        assert ssr == pytest.approx(spread_c / skill.numpy(), rel=REL)
    ssr = M.evaluate_ensemble_spread_skill_ratio(dp, dt, eng, skill_metric=np.float64(3.0))
    assert isinstance(float(ssr), float) and float(ssr) == pytest.approx(np.sqrt(pn.astype(np.float64).var(axis=0).mean()) / 3.0, rel=REL)
    # kept axes with a gap
    with pytest.raises(NotImplementedError, match="one contiguous run"):
        M.evaluate_ensemble_mse(dp, dt, eng, mean_dims=(1,))
    # several horizons of one shape, one value per sample: the segments of one call
    p2, t2 = _inputs(n, b, (c, h, w), seed=77)
    many = M.evaluate_ensemble_scores([dp, p2.cuda()], [dt, t2.cuda()], eng, mean_dims=(1, 2, 3))
    assert tuple(many["crps"].shape) == (2, b) and _same_bits(many["crps"][0], got["crps"]) and _same_bits(many["corr"][0], got["corr"])
    ref2 = refs.group_reference(p2.numpy(), t2.numpy(), (1, b, c * h * w))
    assert many["mse"][1].cpu().numpy() == pytest.approx(ref2[0], rel=REL) and np.all(np.abs(many["corr"][1].cpu().numpy() - ref2[4]) <= CORR_ABS)
    pooled_many = M.evaluate_ensemble_scores([dp, p2.cuda()], [dt, t2.cuda()], eng)
    assert pooled_many["mse"].shape == (2,) and pooled_many["mse"][0] == M.evaluate_ensemble_mse(dp, dt, eng)


def test_validation_epoch_with_extended_metrics():
    """validation_step x 2 + on_validation_epoch_end with extended_metrics: exactly the nll / corr and per-channel keys are added,
    against the reference on the pooled fields; every key of the flag-off epoch over the same fields keeps its value."""
    N = 4
    exp = _tiny_experiment(N, False, extended_metrics=True)
    outs = [exp.validation_step(batch, 0) for batch in _batches(3)]
    got = exp.on_validation_epoch_end()
    off = _tiny_experiment(N, False)
    assert off.extended_metrics is False
    off.__dict__["_validation_step_outputs"] = list(outs)  # the same fields through the epoch end without the flag
    base = off.on_validation_epoch_end()
    # ensemble_metrics_kernel adds with fp64 atomics: two launches agree to 1e-12, not to the bit (test_gpu_ensemble_size_metrics.py)
    assert len(base) == 12 and all(got[k] == pytest.approx(base[k], rel=1e-12) for k in base)
    stem = f"val/{N}ens_mems/"
    horizons = ("t1", "t2", "t3", "avg")
    assert set(got) - set(base) == ({f"{stem}{t}/{m}" for t in horizons for m in ("nll", "corr")}
                                    | {f"{stem}{t}/c{j}/{m}" for t in horizons for j in (0, 1) for m in refs.ROWS})
    assert all(isinstance(v, float) for v in got.values())
    for k in (1, 2, 3):
        preds = torch.cat([o[f"t{k}_preds"] for o in outs], dim=1).cpu().numpy()     # (N, 5, C, H, W)
        targets = torch.cat([o[f"t{k}_targets"] for o in outs], dim=0).cpu().numpy()
        b, c, h, w = targets.shape
        pooled = refs.pooled_reference(preds, targets)
        scale = refs.nll_scale(preds[:, None], targets[None])[0, 0]
        assert abs(got[f"{stem}t{k}/nll"] - pooled[3]) <= REL * scale and abs(got[f"{stem}t{k}/corr"] - pooled[4]) <= CORR_ABS
        per_c = refs.group_reference(preds, targets, (b, c, h * w))
        per_c_scale = refs.nll_scale(preds[:, None], targets[None], (b, c, h * w))[0]
        _check(np.array([[got[f"{stem}t{k}/c{j}/{m}"] for j in range(c)] for m in refs.ROWS])[:, None], per_c[:, None], per_c_scale[None], N,
               f"t{k} per channel")
    for m in ("nll", "corr"):
        assert got[f"{stem}avg/{m}"] == pytest.approx(np.mean([got[f"{stem}t{k}/{m}"] for k in (1, 2, 3)]))
    assert got[f"{stem}avg/c1/crps"] == pytest.approx(np.mean([got[f"{stem}t{k}/c1/crps"] for k in (1, 2, 3)]))
