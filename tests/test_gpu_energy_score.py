"""-m gpu: dyf_energy_score (energy_score_kernel) against the float64 reference of tests/energy_score_refs.py within its derived bound
(u = 2^-24, K = DYF_ENERGY_TILE_POINTS; every d, D and mean of them within (K + 2) u of itself) on every case of refs.SHAPES: all four
planes and both optional matrices; determinism, the accumulator, the refusals, the metrics surface and the experiment's keys."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import energy_score_refs as refs
from tests.test_gpu_ensemble_size_metrics import _batches, _engine, _tiny_experiment

pytestmark = pytest.mark.gpu


def _bits(x):
    return x.contiguous().view(torch.int64)


def _same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(_bits(a), _bits(b)))


def _device_inputs(c):
    """The case in the form it names: one (N, S, outer, groups, inner) tensor with (S, ...) targets, or lists of S tensors."""
    preds = torch.from_numpy(np.array(c.preds)).reshape(c.n, c.segs, *c.group_shape)
    targets = torch.from_numpy(np.array(c.targets)).reshape(c.segs, *c.group_shape)
    if c.form == "tensor":
        return preds.cuda(), targets.cuda()
    return [preds[:, s].contiguous().cuda() for s in range(c.segs)], [targets[s].contiguous().cuda() for s in range(c.segs)]


def _run(eng, c, **kw):
    p, t = _device_inputs(c)
    out, mats = eng.energy_score(p, t, group_shape=c.group_shape, members=True, pairs=True, **kw)
    return out, mats["member_dist"], mats["pair_dist"]


@pytest.mark.parametrize("name", list(refs.SHAPES))
def test_cases_match_the_reference_within_the_bound(name):
    c, ref = refs.case(name), refs.reference(name)
    g = c.group_shape[1]
    sentinel = -12345.0
    eng = _engine()
    p, t = _device_inputs(c)
    out = torch.full((4, c.segs, g), sentinel, dtype=torch.float64).cuda()
    member = torch.full((c.segs, g, c.n), sentinel, dtype=torch.float64).cuda()
    pair = torch.full((c.segs, g, c.n, c.n), sentinel, dtype=torch.float64).cuda()
    got, gm, gp = _run(eng, c)
    # the same call straight into sentinel-filled buffers: every entry is overwritten, with the same bits
    n, nseg, points, stride, p_ptrs, t_ptrs, keep, dev = eng._segments(p, t, "energy_score")
    eng._check(eng._lib.dyf_energy_score(eng._h, nseg, (C.c_void_p * nseg)(*p_ptrs), (C.c_void_p * nseg)(*t_ptrs), n, points, stride,
                                         *c.group_shape, out.data_ptr(), member.data_ptr(), pair.data_ptr(), None, eng._stream()))
    torch.cuda.synchronize()
    assert not bool((out == sentinel).any()) and not bool((member == sentinel).any()) and not bool((pair == sentinel).any())
    assert _same_bits(out, got) and _same_bits(member, gm) and _same_bits(pair, gp)
    dev_out = {"planes": got.cpu().numpy(), "member": gm.cpu().numpy(), "pair": gp.cpu().numpy()}
    assert dev_out["planes"].dtype == np.float64 and dev_out["planes"].shape == (4, c.segs, g)
    worst = {k: refs.worst_ratio(dev_out, ref, c.n, keys=(k,)) for k in ("planes", "member", "pair")}
    print(f"{name}: error / bound = {worst}")
    assert max(worst.values()) <= 1.0
    # the pair matrix: bitwise symmetric, the diagonal exactly zero
    idx = torch.arange(c.n)
    assert bool((gp[..., idx, idx] == 0.0).all())
    finite = ~torch.isnan(gp)
    assert bool(torch.equal(finite, finite.transpose(-1, -2)))
    assert bool(torch.equal(_bits(torch.nan_to_num(gp)), _bits(torch.nan_to_num(gp.transpose(-1, -2)))))
    # without the matrices: the same planes
    assert _same_bits(eng.energy_score(p, t, group_shape=c.group_shape), got)
    only_members = eng.energy_score(p, t, group_shape=c.group_shape, members=True)
    assert set(only_members[1]) == {"member_dist"} and _same_bits(only_members[1]["member_dist"], gm)


@pytest.mark.parametrize("name", ["n63", "n63_points"])
def test_one_point_vectors_are_the_crps_of_ensemble_scores(name):
    """n_inner = 1: es is the CRPS estimator of ensemble_scores_kernel.  That kernel takes |x - y| and the pair term in fp32 per point
    and only the sum over points in float64, so it differs from the float64-joined energy score by fp32 rounding of sums of up to N^2
    terms per point: 1e-6 relative is the tolerance the OLDER kernel's fp32 arithmetic sets, not this one's."""
    c = refs.case(name)
    eng = _engine()
    p, t = _device_inputs(c)
    es = eng.energy_score(p, t, group_shape=c.group_shape)[0].cpu().numpy()
    crps = eng.ensemble_scores(p, t, group_shape=c.group_shape)[2].cpu().numpy()
    print(name, float(np.max(np.abs(es - crps) / np.abs(crps))))
    assert es == pytest.approx(crps, rel=1e-6)


def test_accum_adds_and_two_calls_are_bit_equal():
    c = refs.case("n65")  # a vector split into chunks
    eng = _engine()
    p, t = _device_inputs(c)
    first = eng.energy_score(p, t, group_shape=c.group_shape, members=True, pairs=True)
    start = torch.arange(4 * c.segs * c.group_shape[1], dtype=torch.float64).reshape(4, c.segs, -1).cuda()
    accum = start.clone()
    second = eng.energy_score(p, t, group_shape=c.group_shape, members=True, pairs=True, accum=accum)
    assert _same_bits(first[0], second[0]) and all(_same_bits(first[1][k], second[1][k]) for k in first[1])
    assert _same_bits(accum, start + first[0])
    eng.energy_score(p, t, group_shape=c.group_shape, accum=accum)
    assert _same_bits(accum, start + first[0] + first[0])


@pytest.mark.parametrize("name", ["n5", "n64"])
def test_reversing_the_segments_reverses_the_output(name):
    c = refs.case(name)
    eng = _engine()
    preds = torch.from_numpy(np.array(c.preds)).reshape(c.n, c.segs, *c.group_shape)
    targets = torch.from_numpy(np.array(c.targets)).reshape(c.segs, *c.group_shape)
    plist = [preds[:, s].contiguous().cuda() for s in range(c.segs)]
    tlist = [targets[s].contiguous().cuda() for s in range(c.segs)]
    fwd = eng.energy_score(plist, tlist, group_shape=c.group_shape, members=True, pairs=True)
    rev = eng.energy_score(plist[::-1], tlist[::-1], group_shape=c.group_shape, members=True, pairs=True)
    assert _same_bits(fwd[0].flip(1), rev[0])
    assert all(_same_bits(fwd[1][k].flip(0), rev[1][k]) for k in ("member_dist", "pair_dist"))
    # and the tensor form (member stride S * points) gives the bits of the list form
    both = eng.energy_score(preds.cuda(), targets.cuda(), group_shape=c.group_shape, members=True, pairs=True)
    assert _same_bits(both[0], fwd[0]) and all(_same_bits(both[1][k], fwd[1][k]) for k in fwd[1])


def test_a_nan_poisons_its_own_segment_and_group_only():
    c, at = refs.case("nan"), refs.NAN_AT
    eng = _engine()
    got, gm, gp = _run(eng, c)
    bad = torch.zeros(c.segs, c.group_shape[1], dtype=torch.bool)
    bad[at["segment"], at["group"]] = True
    assert bool(torch.equal(torch.isnan(got).cpu(), bad.expand(4, -1, -1)))
    assert int(torch.isnan(gm).sum()) == 1 and bool(torch.isnan(gm[at["segment"], at["group"], at["member"]]))
    assert int(torch.isnan(gp).sum()) == 2 * (c.n - 1)
    # the other entries carry the bits of the same call without the NaN
    clean = np.array(c.preds)
    clean[np.isnan(clean)] = 0.25
    preds = torch.from_numpy(clean).reshape(c.n, c.segs, *c.group_shape).cuda()
    targets = torch.from_numpy(np.array(c.targets)).reshape(c.segs, *c.group_shape).cuda()
    want = eng.energy_score(preds, targets, group_shape=c.group_shape)
    keep = ~bad.cuda().expand(4, -1, -1)
    assert bool(torch.equal(_bits(got)[keep], _bits(want)[keep]))


def test_refusals():
    from dyffusion_amd import _lib as L

    eng = _engine()
    z = torch.zeros
    p, t = z(3, 2, 12).cuda(), z(2, 12).cuda()
    assert tuple(eng.energy_score(p, t, group_shape=[2, 3, 2]).shape) == (4, 2, 3)
    for gs in ((1, 5, 2), (2, 3, 4), (0, 1, 12), (12,), (1, 1.5, 8), "abc"):
        with pytest.raises(ValueError):
            eng.energy_score(p, t, group_shape=gs)
    with pytest.raises(ValueError, match="GPU tensors"):
        eng.energy_score([z(3, 5)], [z(5)])  # CPU tensors
    with pytest.raises(ValueError):
        eng.energy_score(p, t, group_shape=(1, 3, 4), accum=torch.zeros(4, 2, 4, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        eng.energy_score(p, t, group_shape=(1, 3, 4), accum=torch.zeros(4, 2, 3).cuda())  # fp32 accumulator
    with pytest.raises(NotImplementedError, match=r"\[1, 256\]"):
        eng.energy_score(z(257, 1, 4).cuda(), z(1, 4).cuda())
    with pytest.raises(NotImplementedError, match=r"2\^27"):  # 256 members: 65 792 doubles per vector and 2^27 / 65 792 = 2040.03
        eng.energy_score(z(256, 1, 2041).cuda(), z(1, 2041).cuda(), group_shape=(2041, 1, 1))
    # the C ABI's own checks, with counts far beyond the dummy tables: refused before anything is launched or read
    p, t = z(3, 12).cuda(), z(12).cuda()
    out = torch.zeros(4, 1, 3, dtype=torch.float64).cuda()
    tab = lambda x: (C.c_void_p * 1)(x.data_ptr())  # noqa: E731

    def call(nseg=1, n=3, points=12, stride=12, gs=(2, 3, 2), outp=None):
        return eng._lib.dyf_energy_score(eng._h, nseg, tab(p), tab(t), n, points, stride, gs[0], gs[1], gs[2],
                                         out.data_ptr() if outp is None else outp, None, None, None, eng._stream())
    assert call() == L.DYF_OK
    assert call(n=257) == L.DYF_ERR_UNSUPPORTED
    assert b"[1, 256]" in eng._lib.dyf_last_error(eng._h)
    assert call(n=0) == L.DYF_ERR_INVALID_ARGUMENT and call(nseg=0) == L.DYF_ERR_INVALID_ARGUMENT and call(outp=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(stride=11) == L.DYF_ERR_INVALID_ARGUMENT and call(gs=(2, 3, 3)) == L.DYF_ERR_INVALID_ARGUMENT
    huge = 1 << 40
    for n, points, gs in ((256, huge, (huge, 1, 1)), (3, huge, (1, huge >> 10, 1 << 10)), (256, huge, (1 << 20, 1, 1 << 20))):
        assert call(n=n, points=points, stride=points, gs=gs) == L.DYF_ERR_UNSUPPORTED, (n, gs)
        assert b"2^27" in eng._lib.dyf_last_error(eng._h)
    torch.cuda.synchronize()
    assert call() == L.DYF_OK  # the engine is as usable as before
    torch.cuda.synchronize()


def test_form_is_noted_in_the_form_log():
    c = refs.case("n3")
    eng = _engine()
    p, t = _device_inputs(c)
    eng.form_log(True)
    try:
        eng.energy_score(p, t, group_shape=c.group_shape)
        log = eng.form_log_read()
    finally:
        eng.form_log(False)
    assert log.get("energy_score_kernel:pairs4x4") == {0: 1}


def test_fp16_build_exports_the_function_and_agrees_bitwise():
    import dyffusion_amd as D

    c = refs.case("n65")
    net = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=1, num_output_channels=1,
                 num_conditional_channels=0, spatial_shape=(16, 16))
    cfg = net.engine_net_config()
    half = D.HipEngine(cfg, cfg, height=16, width=16, max_batch=1, use_graph=False, dtype="fp16")
    assert half._lib.dyf_dtype() == 1 and _engine()._lib.dyf_dtype() == 0
    a, b = _run(_engine(), c), _run(half, c)
    assert all(_same_bits(x, y) for x, y in zip(a, b))


def test_metrics_surface():
    from dyffusion_amd import metrics as M

    eng = _engine()
    g = torch.Generator().manual_seed(5)
    n, b, ch, h, w = 6, 3, 2, 7, 5
    truth = torch.randn(2, b, ch, h, w, generator=g)
    preds = 0.8 * truth[None] + 0.5 * torch.randn(n, 2, b, ch, h, w, generator=g)
    plist, tlist = [preds[:, s].contiguous().cuda() for s in range(2)], [truth[s].contiguous().cuda() for s in range(2)]
    assert M.ENERGY_ROWS == ("es", "es_fair", "dist_target", "dist_pair")
    for s in range(2):
        x, y = preds[:, s].numpy().reshape(n, -1), truth[s].numpy().reshape(-1)
        field = refs.reference_segment(x, y, (b, 1, ch * h * w))
        chan = refs.reference_segment(x, y, (b, ch, h * w))
        one = M.evaluate_ensemble_energy_score(plist[s], tlist[s], eng)
        assert set(one) == set(M.ENERGY_ROWS) and all(isinstance(v, float) for v in one.values())
        per_c = M.evaluate_ensemble_energy_score(plist[s], tlist[s], eng, per_channel=True)
        mats = M.evaluate_member_distances(plist[s], tlist[s], eng)
        mats_c = M.evaluate_member_distances(plist[s], tlist[s], eng, per_channel=True)
        assert tuple(mats["member_dist"].shape) == (n,) and tuple(mats["pair_dist"].shape) == (n, n)
        assert tuple(mats_c["member_dist"].shape) == (ch, n) and tuple(mats_c["pair_dist"].shape) == (ch, n, n)
        for m in M.ENERGY_ROWS:
            assert per_c[m].is_cuda and per_c[m].dtype == torch.float64 and tuple(per_c[m].shape) == (ch,)
        # within the derived bound of the reference on the same members
        got = {"planes": np.array([one[m] for m in M.ENERGY_ROWS]).reshape(4, 1, 1), "member": mats["member_dist"].cpu().numpy()[None, None],
               "pair": mats["pair_dist"].cpu().numpy()[None, None]}
        assert refs.worst_ratio(got, {"planes": field[0][:, None], "member": field[1][None], "pair": field[2][None]}, n) <= 1.0
        got = {"planes": np.stack([per_c[m].cpu().numpy() for m in M.ENERGY_ROWS])[:, None], "member": mats_c["member_dist"].cpu().numpy()[None],
               "pair": mats_c["pair_dist"].cpu().numpy()[None]}
        assert refs.worst_ratio(got, {"planes": chan[0][:, None], "member": chan[1][None], "pair": chan[2][None]}, n) <= 1.0
    many = M.evaluate_ensemble_energy_score(plist, tlist, eng)
    assert all(isinstance(v, np.ndarray) and v.shape == (2,) for v in many.values())
    assert many["es"][1] == M.evaluate_ensemble_energy_score(plist[1], tlist[1], eng)["es"]
    assert tuple(M.evaluate_ensemble_energy_score(plist, tlist, eng, per_channel=True)["es"].shape) == (2, ch)
    assert tuple(M.evaluate_member_distances(plist, tlist, eng)["pair_dist"].shape) == (2, n, n)
    with pytest.raises(ValueError, match="GPU tensors"):
        M.evaluate_ensemble_energy_score(preds[:, 0], truth[0], eng)
    with pytest.raises(ValueError, match="GPU tensors"):
        M.evaluate_member_distances(preds[:, 0], truth[0], eng)
    with pytest.raises(AssertionError):
        M.evaluate_ensemble_energy_score(plist[0], tlist[0][:2], eng)


N, T = 4, 3
BASE = {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("mse", "ssr", "crps")}


def test_energy_score_keys_of_the_validation_epoch():
    from dyffusion_amd.metrics import evaluate_ensemble_energy_score

    exp = _tiny_experiment(N, False, energy_score=True)
    outs = [exp.validation_step(b, 0) for b in _batches(T)]
    got = exp.on_validation_epoch_end()
    new = {f"val/{N}ens_mems/{t}/{m}" for t in ("t1", "t2", "t3", "avg") for m in ("es", "es_fair")}
    new |= {f"val/{N}ens_mems/t{k}/c{j}/es" for k in range(1, T + 1) for j in range(2)}
    assert set(got) == BASE | new
    for m in ("es", "es_fair"):
        per_t = []
        for k in range(1, T + 1):
            preds = torch.cat([o[f"t{k}_preds"] for o in outs], dim=1)
            targets = torch.cat([o[f"t{k}_targets"] for o in outs], dim=0)
            want = evaluate_ensemble_energy_score(preds, targets, exp.model._engine)
            assert isinstance(got[f"val/{N}ens_mems/t{k}/{m}"], float) and got[f"val/{N}ens_mems/t{k}/{m}"] == want[m]
            per_c = evaluate_ensemble_energy_score(preds, targets, exp.model._engine, per_channel=True)["es"].cpu().numpy()
            assert [got[f"val/{N}ens_mems/t{k}/c{j}/es"] for j in range(2)] == list(per_c)
            per_t.append(want[m])
        assert got[f"val/{N}ens_mems/avg/{m}"] == pytest.approx(sum(per_t) / T, rel=1e-12)
    # the flag off: the parent's keys, and the values of this very epoch
    exp = _tiny_experiment(N, False)
    for b in _batches(T):
        exp.validation_step(b, 0)
    plain = exp.on_validation_epoch_end()
    assert set(plain) == BASE and all(plain[k] == got[k] for k in BASE)


def test_energy_score_curve_of_the_physical_systems_test_epoch():
    from dyffusion_amd.metrics import TrajectoryMetricsAccumulator, evaluate_ensemble_energy_score

    target = {"_target_": "src.datamodules.physical_systems_benchmark.PhysicalSystemsBenchmarkDataModule"}
    exp = _tiny_experiment(N, False, energy_score=True, datamodule_config=target)
    outs = [exp.test_step(b, 0) for b in _batches(T)]
    got = exp.on_test_epoch_end()
    stem = f"test/{N}ens_mems/"
    extra = {f"{stem}{t}/es" for t in ("t1", "t2", "t3", "avg")}
    assert extra <= set(got) and len(got) == 12 + 4
    eng = exp.model._engine
    curves = []
    for o in outs:  # one instance: its es curve is the direct call on its horizons
        plist, tlist = [o[f"t{k}_preds"] for k in range(1, T + 1)], [o[f"t{k}_targets"] for k in range(1, T + 1)]
        acc = TrajectoryMetricsAccumulator(eng, energy_score=True)
        acc.update(plist, tlist)
        curve = acc.compute()["es"]
        assert np.array_equal(curve, evaluate_ensemble_energy_score(plist, tlist, eng)["es"])
        curves.append(curve)
    mean = np.mean(curves, axis=0)
    for k in range(T):
        assert got[f"{stem}t{k + 1}/es"] == pytest.approx(mean[k], rel=1e-12)
    assert got[f"{stem}avg/es"] == pytest.approx(mean.mean(), rel=1e-12)
    exp = _tiny_experiment(N, False, datamodule_config=target)
    for b in _batches(T):
        exp.test_step(b, 0)
    plain = exp.on_test_epoch_end()
    assert len(plain) == 12 and set(plain) == set(got) - extra and all(plain[k] == got[k] for k in plain)
