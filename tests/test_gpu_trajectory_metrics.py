"""Per-segment ensemble metrics on the device (dyf_trajectory_metrics, HipEngine.trajectory_metrics, the test epoch of a
PhysicalSystemsBenchmarkDataModule) against oracle/metrics.py applied to the slices (pinned to the reference's own curves by
tests/test_trajectory_metrics_refs.py).  Inputs as in tests/test_gpu_metrics.py: truth * 0.7 + 0.6 * randn + 0.1, so MSE is
0.1-0.5 and SSR above 1; tolerance rel 2e-5 from there (same per-point fp32 arithmetic, fp64 sums)."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import metrics as om

pytestmark = pytest.mark.gpu
ROWS = ("mse", "ssr", "crps")
_ENGINE = []


def _engine():
    import dyffusion_amd as D
    from dyffusion_amd.engine import HipEngine

    if not _ENGINE:
        net = D.UNet(dim=8, with_time_emb=True, upsample_dims=[64, 64], num_input_channels=1, num_output_channels=1,
                     num_conditional_channels=0, spatial_shape=(16, 16))
        _ENGINE.append(HipEngine(net.engine_net_config(), net.engine_net_config(), height=16, width=16, max_batch=1, use_graph=False))
    return _ENGINE[0]


def _inputs(n, t, point_shape, seed=None):
    """preds (N, T, *point_shape), truth (T, *point_shape) on the CPU; the spread differs from segment to segment."""
    g = torch.Generator().manual_seed(n * 1000 + t if seed is None else seed)
    truth = torch.randn(t, *point_shape, generator=g)
    scale = (0.6 + 0.05 * torch.arange(t)).reshape(1, t, *([1] * len(point_shape)))
    preds = truth[None] * 0.7 + scale * torch.randn(n, t, *point_shape, generator=g) + 0.1
    return preds, truth


def _oracle(preds, truth):
    """(3, T) float64: oracle/metrics.py on every slice preds[:, s], truth[s]."""
    p, y = preds.numpy(), truth.numpy()
    out = np.zeros((3, p.shape[1]))
    for s in range(p.shape[1]):
        ref = om.evaluate_ensemble_prediction(p[:, s], y[s])
        out[:, s] = [ref[k] for k in ROWS]
    return out


def _check(got, ref, n, rel=2e-5):
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float64
    for i, k in enumerate(ROWS):
        if n == 1 and k == "ssr":
            assert np.all(got[i] == 0.0) and np.all(ref[i] == 0.0)  # one member: zero spread
            continue
        for s in range(ref.shape[1]):
            assert got[i, s] == pytest.approx(ref[i, s], rel=rel), (k, s)


def _as_lists(preds, truth):
    return ([preds[:, s].contiguous().cuda() for s in range(preds.shape[1])], [truth[s].contiguous().cuda() for s in range(truth.shape[0])])


CASES = [  # N, segments, points per segment, both layouts
    (20, 3, (2, 3, 17, 9), True),   # several workgroups, partial last one
    (1, 2, (63,), False),           # single member
    (64, 2, (330,), True),          # LDS edge of the small form
    (65, 2, (330,), True),          # tiled form
    (256, 3, (253,), False),        # tiled form, small P
    (2000, 1, (7,), False),         # tiled form, 4 points per workgroup: the 64 shares of a point fill a wave
    (5, 130, (70,), False),         # more segments than a wave has lanes
    (3, 1, (255,), False),          # below / exactly / one past the 256-thread tile
    (3, 1, (256,), False),
    (3, 1, (257,), False),
]


@pytest.mark.parametrize("n,t,pts,both", CASES, ids=[f"N{c[0]}-T{c[1]}-{'x'.join(map(str, c[2]))}" for c in CASES])
def test_segments_match_oracle_per_slice(n, t, pts, both):
    eng = _engine()
    preds, truth = _inputs(n, t, pts)
    ref = _oracle(preds, truth)
    _check(eng.trajectory_metrics(*_as_lists(preds, truth)), ref, n)
    if both:  # the strided layout: one (N, S, ...) tensor read in place
        _check(eng.trajectory_metrics(preds.cuda(), truth.cuda()), ref, n)


def test_strided_layout_with_an_odd_point_count():
    """105 points per segment: the pointers of the odd segments are 4-byte aligned and no more."""
    eng = _engine()
    preds, truth = _inputs(7, 5, (3, 5, 7))
    dp, dt = preds.cuda(), truth.cuda()
    assert dp.is_contiguous() and (dp.data_ptr() + 4 * 105) % 8 == 4
    _check(eng.trajectory_metrics(dp, dt), _oracle(preds, truth), 7)


def test_targets_as_views_of_the_dynamics():
    """targets = dynamics[:, k] (B = 2): strided views, made contiguous on the way in."""
    eng = _engine()
    g = torch.Generator().manual_seed(11)
    b, t = 2, 4
    dynamics = torch.randn(b, t + 1, 2, 9, 7, generator=g)
    preds = [dynamics[:, k][None] * 0.7 + 0.6 * torch.randn(6, b, 2, 9, 7, generator=g) + 0.1 for k in range(1, t + 1)]
    dyn = dynamics.cuda()
    views = [dyn[:, k] for k in range(1, t + 1)]
    assert not views[0].is_contiguous()
    got = eng.trajectory_metrics([p.cuda() for p in preds], views)
    ref = _oracle(torch.stack(preds, dim=1), torch.stack([dynamics[:, k] for k in range(1, t + 1)], dim=0))
    _check(got, ref, 6)


def test_identical_calls_are_bitwise_equal_and_segments_do_not_depend_on_their_neighbours():
    eng = _engine()
    for n, pts in ((20, (2, 3, 17, 9)), (65, (330,))):
        preds, truth = _inputs(n, 4, pts)
        pl, tl = _as_lists(preds, truth)
        a = eng.trajectory_metrics(pl, tl)
        b = eng.trajectory_metrics(pl, tl)
        assert torch.equal(a, b)
        assert torch.equal(a, eng.trajectory_metrics(preds.cuda(), truth.cuda()))  # the layout changes no bit either
        for s in range(4):
            one = eng.trajectory_metrics([pl[s]], [tl[s]])
            assert one.shape == (3, 1) and torch.equal(one[:, 0], a[:, s]), (n, s)


def test_two_calls_back_to_back_with_different_pointer_tables():
    """The second call rewrites the engine's pointer staging: only after the first call's upload has completed."""
    eng = _engine()
    pa, ta = _inputs(6, 5, (301,), seed=1)
    pb, tb = _inputs(6, 5, (301,), seed=2)
    la, lb = _as_lists(pa, ta), _as_lists(pb, tb)
    torch.cuda.synchronize()
    ga = eng.trajectory_metrics(*la)  # nothing waits in between
    gb = eng.trajectory_metrics(*lb)
    gc = eng.trajectory_metrics(*la)
    _check(ga, _oracle(pa, ta), 6)
    _check(gb, _oracle(pb, tb), 6)
    assert torch.equal(ga, gc) and not torch.equal(ga, gb)


def test_accumulator_mean_over_instances_reset_and_mismatch():
    from dyffusion_amd.metrics import TrajectoryMetricsAccumulator

    eng = _engine()
    acc = TrajectoryMetricsAccumulator(eng)
    assert acc.compute() == {}
    refs = []
    for i, b in enumerate((3, 2, 1)):  # three instances, T = 4, different batch sizes
        preds, truth = _inputs(5, 4, (b, 2, 9, 7), seed=40 + i)
        ref = _oracle(preds, truth)
        refs.append(ref)
        _check(acc.update(*_as_lists(preds, truth)), ref, 5)
    assert acc.count == 3
    got = acc.compute()
    want = np.mean(np.stack(refs), axis=0)
    assert list(got) == list(ROWS)
    for i, k in enumerate(ROWS):
        assert got[k].shape == (4,) and got[k].dtype == np.float64
        assert got[k] == pytest.approx(want[i], rel=2e-5), k
    preds, truth = _inputs(5, 3, (2, 2, 9, 7))
    with pytest.raises(ValueError):
        acc.update(*_as_lists(preds, truth))  # T = 3 after T = 4
    assert acc.count == 3
    acc.reset()
    assert acc.compute() == {} and acc.count == 0
    _check(acc.update(*_as_lists(preds, truth)), _oracle(preds, truth), 5)  # any T after a reset
    one = acc.compute()
    assert one["crps"] == pytest.approx(_oracle(preds, truth)[2], rel=2e-5)


def test_evaluate_ensemble_prediction_per_sample():
    from dyffusion_amd.metrics import evaluate_ensemble_prediction

    eng = _engine()
    preds, truth = _inputs(8, 6, (2, 11, 5))
    got = evaluate_ensemble_prediction(preds.cuda(), truth.cuda(), eng, mean_over_samples=False)
    assert set(got) == {"ssr", "crps", "mse"}
    ref = _oracle(preds, truth)
    for i, k in enumerate(ROWS):
        assert got[k].is_cuda and got[k].dtype == torch.float64 and tuple(got[k].shape) == (6,)
        assert got[k].cpu().numpy() == pytest.approx(ref[i], rel=2e-5), k
    pooled = evaluate_ensemble_prediction(preds.cuda(), truth.cuda(), eng)  # the default path: host floats over all samples
    whole = om.evaluate_ensemble_prediction(preds.numpy(), truth.numpy())
    for k in ROWS:
        assert isinstance(pooled[k], float) and pooled[k] == pytest.approx(whole[k], rel=2e-5)
    with pytest.raises(NotImplementedError):
        evaluate_ensemble_prediction(preds.cuda(), truth.cuda(), eng, also_per_member_metrics=True)
    with pytest.raises(NotImplementedError):
        evaluate_ensemble_prediction(preds.cuda(), truth.cuda(), eng, mean_over_samples=False, also_per_member_metrics=True)


def test_physical_systems_test_epoch_on_the_device():
    """test_step x 2 + on_test_epoch_end for a PhysicalSystemsBenchmarkDataModule (forecasting_multi_horizon.py:231-279): the
    curves of every instance, averaged over the instances; against the oracle on the fields the steps returned (rel 5e-5, as
    the validation-epoch test of tests/test_gpu_experiment.py).  Without the config: today's pooled keys."""
    import dyffusion_amd as D
    from tests.gpu_common import DEV, build_dyffusion, seeded_pair

    mk = dict(dim=8, outer_sample_mode="bilinear", upsample_dims=[64, 64], with_time_emb=True, input_dropout=0.0, dropout=0.2)
    hp = dict(timesteps=3, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only",
              sampling_type="cold", refine_intermediate_predictions=True, enable_interpolator_dropout=True)
    C_, Cs, N, T = 2, 1, 4, 6
    PF, PI = seeded_pair(8, C_, Cs)
    m = build_dyffusion(PF, PI, mk, C_, Cs, hp, max_batch=N * 3)
    m.seed(7)

    class DM:
        test_set_name = "test_hard"

    cfg = {"_target_": "src.datamodules.physical_systems_benchmark.PhysicalSystemsBenchmarkDataModule"}
    exp = D.MultiHorizonForecastingDYffusion(m, num_predictions=N, window=1, autoregressive_steps=1, datamodule_config=cfg)
    assert exp.prediction_horizon == T
    g = torch.Generator().manual_seed(2)
    batches = [{"dynamics": torch.randn(b, 1 + T, C_, 19, 13, generator=g).to(DEV), "condition": torch.rand(b, Cs, 19, 13, generator=g).to(DEV)}
               for b in (3, 2)]
    outs = [exp.test_step({k: v.clone() for k, v in batch.items()}, i) for i, batch in enumerate(batches)]
    assert exp.__dict__.get("_test_step_outputs", []) == []  # the fields are not kept
    got = exp.on_test_epoch_end()
    assert exp.on_test_epoch_end() == {}  # the sums were consumed
    curves = []
    for o in outs:
        assert [k for k in o if k.endswith("preds")] == [f"t{k}_preds" for k in range(1, T + 1)]
        preds = torch.stack([o[f"t{k}_preds"] for k in range(1, T + 1)], dim=1).cpu()      # (N, T, B, C, H, W)
        targets = torch.stack([o[f"t{k}_targets"] for k in range(1, T + 1)], dim=0).cpu()  # (T, B, C, H, W)
        assert preds.shape[:2] == (N, T)
        curves.append(_oracle(preds, targets))
    want = np.mean(np.stack(curves), axis=0)  # (3, T)
    stem = f"test/{N}ens_mems/"
    assert set(got) == {f"{stem}avg/{k}" for k in ROWS} | {f"{stem}t{i}/{k}" for i in range(1, T + 1) for k in ROWS}
    for r, k in enumerate(ROWS):
        for i in range(T):
            assert got[f"{stem}t{i + 1}/{k}"] == pytest.approx(want[r, i], rel=5e-5), (k, i)
        assert got[f"{stem}avg/{k}"] == pytest.approx(want[r].mean(), rel=5e-5), k
        assert got[f"{stem}avg/{k}"] == pytest.approx(np.mean([got[f"{stem}t{i}/{k}"] for i in range(1, T + 1)]))
    # the datamodule's split name becomes a level of the keys
    exp._datamodule = DM()
    exp.test_step({k: v.clone() for k, v in batches[1].items()}, 0, boundary_conditions=None)
    named = exp.on_test_epoch_end()
    assert set(named) == {k.replace("test/", "test/test_hard/", 1) for k in got}
    # without the config: the base-class path, pooled over the batches, fields kept until the epoch ends
    m.seed(7)
    base = D.MultiHorizonForecastingDYffusion(m, num_predictions=N, window=1, autoregressive_steps=1)
    outs2 = [base.test_step({k: v.clone() for k, v in batch.items()}, i) for i, batch in enumerate(batches)]
    assert len(base._test_step_outputs) == 2
    pooled = base.on_test_epoch_end()
    assert set(pooled) == set(got)  # same names, other quantities
    for k in (1, T):
        p = torch.cat([o[f"t{k}_preds"] for o in outs2], dim=1).cpu().numpy()
        y = torch.cat([o[f"t{k}_targets"] for o in outs2], dim=0).cpu().numpy()
        ref = om.evaluate_ensemble_prediction(p, y)
        for name in ROWS:
            assert pooled[f"{stem}t{k}/{name}"] == pytest.approx(ref[name], rel=5e-5), (k, name)
    assert base.on_test_epoch_end() == {}


def test_argument_checks():
    eng = _engine()
    z = torch.zeros
    with pytest.raises(ValueError):
        eng.trajectory_metrics([], [])  # 0 segments
    with pytest.raises(ValueError):
        eng.trajectory_metrics(z(15361, 1, 5).cuda(), z(1, 5).cuda())  # beyond the 60 KB staging tile
    with pytest.raises(ValueError):
        eng.trajectory_metrics(z(3, 2, 5).cuda(), z(2, 4).cuda())  # mismatched shapes, tensor form
    with pytest.raises(ValueError):
        eng.trajectory_metrics([z(3, 5).cuda(), z(3, 5).cuda()], [z(5).cuda(), z(4).cuda()])  # ... list form
    with pytest.raises(ValueError):
        eng.trajectory_metrics([z(3, 5).cuda(), z(3, 6).cuda()], [z(5).cuda(), z(6).cuda()])  # segments of different sizes
    with pytest.raises(ValueError):
        eng.trajectory_metrics([z(3, 5).cuda()], [z(5).cuda(), z(5).cuda()])
    with pytest.raises(ValueError):
        eng.trajectory_metrics([z(3, 5).cuda()], [z(5).cuda()], accum=torch.zeros(3, 2, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        eng.trajectory_metrics([z(3, 5).cuda()], [z(5).cuda()], accum=torch.zeros(3, 1).cuda())  # fp32 accumulator
    # the C ABI's own limits
    p, t = z(3, 8).cuda(), z(8).cuda()
    out = torch.zeros(3, 1, dtype=torch.float64).cuda()
    tab = lambda x: (C.c_void_p * 1)(x.data_ptr())  # noqa: E731

    def call(nseg=1, n=3, points=8, stride=8, outp=None, preds=None):
        return eng._lib.dyf_trajectory_metrics(eng._h, nseg, preds if preds is not None else tab(p), tab(t), n, points, stride,
                                               out.data_ptr() if outp is None else outp, None, eng._stream())
    from dyffusion_amd import _lib as L
    assert call() == L.DYF_OK
    assert call(nseg=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(nseg=65536) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(n=0) == L.DYF_ERR_INVALID_ARGUMENT and call(n=15361) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(points=0, stride=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(points=8, stride=7) == L.DYF_ERR_INVALID_ARGUMENT  # member_stride < n_points
    assert call(outp=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(preds=(C.c_void_p * 1)(None)) == L.DYF_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()
