"""-m gpu: the rank histogram on the device (dyf_rank_histogram, HipEngine.rank_histogram, metrics.evaluate_rank_histogram) against
the histogram written from its definition in tests/ensemble_products_refs.py: tie-free inputs bin for bin as integers, tied inputs
(members and truth rounded to multiples of 1/4, the last eighth of the points a boundary block where every member IS the truth) at
1e-12 relative per bin.

A tile is 256 consecutive points of one (outer, group) slab; a group's tiles are walked by min(tiles, 256) workgroups; a thread owns
the bins i, i + 256, ...: 255 / 256 members put the last bin on either side of that stride, 1024 members use all five bins of a
thread, 70 000 points of one group are 274 tiles on 256 workgroups: some walk a second tile."""
import numpy as np
import pytest
import torch

from tests import ensemble_products_refs as refs
from tests.test_gpu_ensemble_size_metrics import _engine

pytestmark = pytest.mark.gpu


def _same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int64), b.contiguous().view(torch.int64))


def _case(n, shape, segs, rounded):
    points = int(np.prod(shape))
    pairs = [refs.members(n, points, seed=s, rounded=rounded, offset=0.1 + 0.2 * s) for s in range(segs)]
    return [t for t, _ in pairs], [x for _, x in pairs]


def _run(eng, truths, xs, shape, gs, accum=None):
    n = xs[0].shape[0]
    plist = [torch.from_numpy(x).reshape(n, *shape).cuda() for x in xs]
    tlist = [torch.from_numpy(t).reshape(*shape).cuda() for t in truths]
    return eng.rank_histogram(plist, tlist, group_shape=gs, accum=accum), plist, tlist


GEOMETRIES = {"pooled": None, "channel": (2, 3, 35), "sample": (1, 2, 105)}  # on a (2, 3, 5, 7) target


@pytest.mark.parametrize("geometry", sorted(GEOMETRIES))
@pytest.mark.parametrize("n", [1, 2, 3, 7, 50, 64, 65, 130, 255, 256, 300, 1024])
def test_bins_match_the_definition(n, geometry):
    eng = _engine()
    shape, gs, segs = (2, 3, 5, 7), GEOMETRIES[geometry], 2
    groups = 1 if gs is None else gs[1]
    for rounded in (False, True):
        truths, xs = _case(n, shape, segs, rounded)
        got, plist, tlist = _run(eng, truths, xs, shape, gs)
        assert got.is_cuda and got.dtype == torch.float64 and tuple(got.shape) == (segs, groups, n + 1)
        host = got.cpu().numpy()
        for s in range(segs):
            ref = refs.histogram_reference(xs[s], truths[s], gs)
            refs.check_histogram(host[s], ref, tie_free=not rounded)
            if not rounded:
                assert np.array_equal(host[s].sum(axis=1), np.full(groups, 210.0 / groups))  # every point in exactly one bin
            else:
                assert host[s].sum(axis=1) == pytest.approx(np.full(groups, 210.0 / groups), rel=1e-12)
            alone = eng.rank_histogram([plist[s]], [tlist[s]], group_shape=gs)
            assert _same_bits(alone[0], got[s]), s  # a segment does not depend on its neighbours
        assert _same_bits(eng.rank_histogram(plist, tlist, group_shape=gs), got)  # identical calls, identical bits
        # the strided layout: one (N, S, ...) tensor read in place
        stack, tstack = torch.stack(plist, dim=1), torch.stack(tlist, dim=0)
        assert _same_bits(eng.rank_histogram(stack, tstack, group_shape=gs), got)


def test_groups_are_independent_and_the_boundary_block_spreads():
    eng = _engine()
    n, shape, gs = 7, (2, 3, 5, 7), (2, 3, 35)
    truths, xs = _case(n, shape, 1, True)
    got, plist, tlist = _run(eng, truths, xs, shape, gs)
    for g in range(3):
        # group g is the pooled call on a contiguous copy of its points: other tiles, so the tie weights are added in another order
        gp = plist[0].reshape(n, 2, 3, 35)[:, :, g].contiguous()
        gt = tlist[0].reshape(2, 3, 35)[:, g].contiguous()
        alone = eng.rank_histogram([gp], [gt])[0, 0].cpu().numpy()
        assert alone == pytest.approx(got[0, g].cpu().numpy(), rel=refs.HIST_TIE_REL, abs=0.0), g
        # ... and it keeps its bits whatever the other groups hold
        other_p, other_t = plist[0].reshape(n, 2, 3, 35).clone(), tlist[0].reshape(2, 3, 35).clone()
        for o in range(3):
            if o != g:
                other_p[:, :, o] = other_p[:, :, o].flip(0) * 1.5 - 0.25
                other_t[:, o] = float("nan") if o == (g + 1) % 3 else other_t[:, o] + 0.5
        changed = eng.rank_histogram([other_p.reshape(n, *shape)], [other_t.reshape(*shape)], group_shape=gs)
        assert _same_bits(changed[0, g], got[0, g]) and not _same_bits(changed[0], got[0]), g
    # every member equals the truth: 1 / (N + 1) in every bin, not one pile
    y = torch.from_numpy(truths[0]).cuda()
    flat = eng.rank_histogram([y[None].expand(n, -1).contiguous()], [y]).cpu().numpy()[0, 0]
    assert flat == pytest.approx(np.full(n + 1, 210.0 / (n + 1)), rel=1e-12)


@pytest.mark.parametrize("n,points", [(5, 1), (3, 70000), (1024, 300)])
def test_one_point_many_tiles_and_the_member_limit(n, points):
    eng = _engine()
    truths, xs = _case(n, (points,), 1, points == 70000)
    got, _, _ = _run(eng, truths, xs, (points,), None)
    refs.check_histogram(got.cpu().numpy()[0], refs.histogram_reference(xs[0], truths[0]), tie_free=points != 70000)
    if points == 70000:  # 274 tiles on 256 workgroups; and as 70 groups of 1000 points
        got, _, _ = _run(eng, truths, xs, (points,), (1, 70, 1000))
        refs.check_histogram(got.cpu().numpy()[0], refs.histogram_reference(xs[0], truths[0], (1, 70, 1000)), tie_free=False)


def test_accum_nan_and_refusals():
    eng = _engine()
    n, shape, gs = 7, (2, 3, 5, 7), (2, 3, 35)
    truths, xs = _case(n, shape, 2, True)
    acc = torch.full((2, 3, n + 1), 0.5, dtype=torch.float64, device="cuda")
    got, plist, tlist = _run(eng, truths, xs, shape, gs, accum=acc)
    again = eng.rank_histogram(plist, tlist, group_shape=gs, accum=acc)
    assert _same_bits(again, got) and torch.equal(acc, 0.5 + got + got)
    # NaN points drop out: a NaN member in group 0, a NaN target in group 2 of segment 1
    xs[1][3, 4], truths[1][80] = np.nan, np.nan
    dropped, _, _ = _run(eng, truths, xs, shape, gs)
    host = dropped.cpu().numpy()
    refs.check_histogram(host[1], refs.histogram_reference(xs[1], truths[1], gs), tie_free=False)
    assert host[1].sum(axis=1) == pytest.approx([69.0, 70.0, 69.0], rel=1e-12) and _same_bits(dropped[0], got[0])
    # refusals
    big = torch.zeros(1025, 4, device="cuda")
    with pytest.raises(NotImplementedError):
        eng.rank_histogram([big], [torch.zeros(4, device="cuda")])
    with pytest.raises(ValueError):
        eng.rank_histogram(plist, tlist, group_shape=(2, 3, 36))
    with pytest.raises(ValueError):
        eng.rank_histogram(plist, tlist, group_shape=gs, accum=torch.zeros(2, 3, n, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="GPU tensors"):
        eng.rank_histogram([p.cpu() for p in plist], [t.cpu() for t in tlist])


def test_evaluate_rank_histogram_and_the_accumulator():
    from dyffusion_amd import metrics as M

    eng = _engine()
    n, shape = 7, (2, 3, 5, 7)
    truths, xs = _case(n, shape, 2, True)
    _, plist, tlist = _run(eng, truths, xs, shape, None)
    pooled = M.evaluate_rank_histogram(plist[0], tlist[0], eng)
    f, ri = refs.frequencies(refs.histogram_reference(xs[0], truths[0]))
    assert pooled["rank_hist"] == pytest.approx(f[0], rel=1e-12) and pooled["reliability_index"] == pytest.approx(float(ri[0]), rel=1e-10)
    assert pooled["rank_hist"].sum() == pytest.approx(1.0)
    per_c = M.evaluate_rank_histogram(plist, tlist, eng, mean_dims=(0, 2, 3))
    assert tuple(per_c["rank_hist"].shape) == (2, 3, n + 1) and per_c["rank_hist"].is_cuda
    for s in range(2):
        f, ri = refs.frequencies(refs.histogram_reference(xs[s], truths[s], (2, 3, 35)))
        assert per_c["rank_hist"][s].cpu().numpy() == pytest.approx(f, rel=1e-12)
        assert per_c["reliability_index"][s].cpu().numpy() == pytest.approx(ri, rel=1e-10)
    acc = M.TrajectoryMetricsAccumulator(eng, rank_histogram=True)
    acc.update(plist, tlist)
    acc.update(plist[::-1], tlist[::-1])
    total = np.stack([refs.histogram_reference(xs[s], truths[s])[0] + refs.histogram_reference(xs[1 - s], truths[1 - s])[0] for s in range(2)])
    out = acc.compute()
    assert out["rank_hist"] == pytest.approx(refs.frequencies(total)[0], rel=1e-12) and set(out) == {"mse", "ssr", "crps", "rank_hist"}
