"""The metrics as a function of the ensemble size on the device (dyf_ensemble_size_metrics, HipEngine.ensemble_size_metrics, the
host surface of dyffusion_amd.metrics and the epoch hooks of the experiment) against the per-prefix reference of
tests/ensemble_size_refs.py (oracle/metrics.py on predictions[:n] for every n, pinned to the reference's own numbers by
tests/test_ensemble_size_refs.py).  Inputs as in tests/test_gpu_metrics.py: truth * 0.7 + scale * randn + 0.1 with the spread
growing per segment, so MSE is 0.1-0.5; tolerance rel 2e-5 for every prefix (fp32 recurrences per point, fp64 sums over points).

The tile map: 256 points per tile up to 64 members and 64 beyond, at most 64 workgroups per segment, workgroup b walks the tiles
b, b + 64, ...  So 64 * 256 + 256 + 77 points (66 tiles: two workgroups walk two tiles, the last tile has 77 points) and, in the
one-wave form, 64 * 64 + 64 + 13 points are the smallest sizes at which a workgroup walks more than one tile."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import metrics as om
from tests import ensemble_size_refs as refs

pytestmark = pytest.mark.gpu
REL = 2e-5
_ENGINE = []
TWO_TILES = 64 * 256 + 256 + 77
TWO_TILES_WAVE = 64 * 64 + 64 + 13


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


def _as_lists(preds, truth):
    return ([preds[:, s].contiguous().cuda() for s in range(preds.shape[1])], [truth[s].contiguous().cuda() for s in range(truth.shape[0])])


def _check(got, ref, rel=REL):
    """got: (4, T, N) device tensor; ref: the same shape from tests/ensemble_size_refs.py."""
    got = got.cpu().numpy()
    assert got.shape == ref.shape and got.dtype == np.float64
    print("worst rel diff per plane:", [float(np.max(np.abs(got[i] - ref[i]) / np.maximum(np.abs(ref[i]), 1e-300))) for i in (0, 2, 3)],
          float(np.max(np.abs(got[1, :, 1:] - ref[1, :, 1:]) / np.abs(ref[1, :, 1:]))) if got.shape[2] > 1 else 0.0)
    assert np.all(got[1, :, 0] == 0.0) and np.all(ref[1, :, 0] == 0.0)  # ssr of one member: exactly zero spread
    for i, k in enumerate(refs.ROWS):
        for s in range(ref.shape[1]):
            for n in range(ref.shape[2]):
                if (i, n) != (1, 0):
                    assert got[i, s, n] == pytest.approx(ref[i, s, n], rel=rel), (k, s, n)


CASES = [  # N, segments, points per segment, both layouts
    (20, 3, (2, 3, 17, 9), True),     # several tiles, partial last one
    (1, 2, (63,), True),              # single member
    (2, 1, (257,), True),
    (64, 2, (330,), True),            # LDS edge of the 256-thread form
    (65, 2, (330,), True),            # first case of the one-wave form
    (130, 1, (253,), False),
    (256, 1, (70,), False),           # the limit
    (3, 1, (255,), False),            # below / exactly / one past the 256-point tile
    (3, 1, (256,), False),
    (3, 1, (257,), False),
    (5, 70, (70,), True),             # more segments than a wave has lanes
    (7, 5, (3, 5, 7), True),          # 105 points: the odd segments of the strided layout are only 4-byte aligned
    (3, 1, (TWO_TILES,), True),       # a workgroup walks two tiles, the last tile is partial
    (65, 1, (TWO_TILES_WAVE,), False),  # the same in the one-wave form
]


@pytest.mark.parametrize("n,t,pts,both", CASES, ids=[f"N{c[0]}-T{c[1]}-{'x'.join(map(str, c[2]))}" for c in CASES])
def test_every_prefix_matches_the_reference(n, t, pts, both):
    eng = _engine()
    preds, truth = _inputs(n, t, pts)
    ref = refs.segment_reference(preds.numpy(), truth.numpy())
    got = eng.ensemble_size_metrics(*_as_lists(preds, truth))
    _check(got, ref)
    # crps[1] is the MAE of member 0
    mae = (preds[0].double() - truth.double()).abs().reshape(t, -1).mean(dim=1).numpy()
    assert got[2, :, 0].cpu().numpy() == pytest.approx(mae, rel=REL)
    # entry N - 1 is the score of the whole ensemble: against the kernel that computes only that
    whole = eng.trajectory_metrics(*_as_lists(preds, truth)).cpu().numpy()
    for i in range(3):
        if not (i == 1 and n == 1):
            assert got[i, :, n - 1].cpu().numpy() == pytest.approx(whole[i], rel=REL), refs.ROWS[i]
    if both:  # the strided layout: one (N, S, ...) tensor read in place, the same bits
        dp, dt = preds.cuda(), truth.cuda()
        if pts == (3, 5, 7):
            assert dp.is_contiguous() and (dp.data_ptr() + 4 * 105) % 8 == 4
        assert torch.equal(eng.ensemble_size_metrics(dp, dt), got)


def test_reversed_members_change_the_prefixes_and_permute_the_members_own_mse():
    eng = _engine()
    n = 9
    preds, truth = _inputs(n, 2, (301,))
    preds = preds + 0.1 * torch.arange(n, dtype=torch.float32).reshape(n, 1, 1)  # member k is off by 0.1 k: the first and the last differ
    a = eng.ensemble_size_metrics(preds.cuda(), truth.cuda()).cpu().numpy()
    b = eng.ensemble_size_metrics(preds.flip(0).cuda(), truth.cuda()).cpu().numpy()
    _check(torch.from_numpy(b), refs.segment_reference(preds.flip(0).numpy(), truth.numpy()))
    for i in (0, 2):
        assert np.all(np.abs(a[i, :, 0] - b[i, :, 0]) > 1e-3 * np.abs(a[i, :, 0]))  # prefix 1 is another member now
    for i in range(3):
        assert b[i, :, n - 1] == pytest.approx(a[i, :, n - 1], rel=REL)  # the whole ensemble is the same set
    # a member's squared errors are the same fp32 terms, added over the points in the same order: only the slot differs
    assert b[3] == pytest.approx(a[3][:, ::-1], rel=1e-12)


def test_identical_calls_are_bitwise_equal_and_segments_do_not_depend_on_their_neighbours():
    eng = _engine()
    for n, pts in ((20, (2, 3, 17, 9)), (65, (330,)), (3, (TWO_TILES,))):
        preds, truth = _inputs(n, 3, pts)
        pl, tl = _as_lists(preds, truth)
        a = eng.ensemble_size_metrics(pl, tl)
        assert torch.equal(a, eng.ensemble_size_metrics(pl, tl))
        assert torch.equal(a, eng.ensemble_size_metrics(preds.cuda(), truth.cuda()))  # the layout changes no bit either
        for s in range(3):
            one = eng.ensemble_size_metrics([pl[s]], [tl[s]])
            assert one.shape == (4, 1, n) and torch.equal(one[:, 0], a[:, s]), (n, s)


def test_accum_adds_and_calls_back_to_back_share_the_pointer_table():
    eng = _engine()
    pa, ta = _inputs(6, 4, (301,), seed=1)
    pb, tb = _inputs(6, 4, (301,), seed=2)
    la, lb = _as_lists(pa, ta), _as_lists(pb, tb)
    acc = torch.zeros(4, 4, 6, dtype=torch.float64).cuda()
    torch.cuda.synchronize()
    ga = eng.ensemble_size_metrics(*la, accum=acc)  # nothing waits in between; trajectory_metrics uses the same table
    tr = eng.trajectory_metrics(*lb)
    gb = eng.ensemble_size_metrics(*lb, accum=acc)
    _check(ga, refs.segment_reference(pa.numpy(), ta.numpy()))
    _check(gb, refs.segment_reference(pb.numpy(), tb.numpy()))
    assert torch.equal(acc, ga + gb) and not torch.equal(ga, gb)
    assert torch.equal(tr, eng.trajectory_metrics(*lb))


def test_argument_checks():
    eng = _engine()
    z = torch.zeros
    with pytest.raises(NotImplementedError, match="256"):
        eng.ensemble_size_metrics(z(257, 1, 5).cuda(), z(1, 5).cuda())
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([], [])  # 0 segments
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics(z(3, 0, 5).cuda(), z(0, 5).cuda())  # empty
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics(z(3, 2, 5).cuda(), z(2, 4).cuda())  # mismatched shapes, tensor form
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([z(3, 5).cuda(), z(3, 5).cuda()], [z(5).cuda(), z(4).cuda()])  # ... list form
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([z(3, 5).cuda(), z(3, 6).cuda()], [z(5).cuda(), z(6).cuda()])  # segments of different sizes
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([z(3, 5).cuda()], [z(5).cuda(), z(5).cuda()])
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([z(3, 5)], [z(5)])  # CPU tensors
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([z(3, 5).cuda()], [z(5).cuda()], accum=torch.zeros(3, 1, 3, dtype=torch.float64).cuda())
    with pytest.raises(ValueError):
        eng.ensemble_size_metrics([z(3, 5).cuda()], [z(5).cuda()], accum=torch.zeros(4, 1, 3).cuda())  # fp32 accumulator
    # the C ABI's own limits
    p, t = z(3, 8).cuda(), z(8).cuda()
    out = torch.zeros(4, 1, 3, dtype=torch.float64).cuda()
    tab = lambda x: (C.c_void_p * 1)(x.data_ptr())  # noqa: E731

    def call(nseg=1, n=3, points=8, stride=8, outp=None, preds=None):
        return eng._lib.dyf_ensemble_size_metrics(eng._h, nseg, preds if preds is not None else tab(p), tab(t), n, points, stride,
                                                  out.data_ptr() if outp is None else outp, None, eng._stream())
    from dyffusion_amd import _lib as L
    assert call() == L.DYF_OK
    assert call(nseg=0) == L.DYF_ERR_INVALID_ARGUMENT and call(nseg=65536) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(n=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(n=257) == L.DYF_ERR_UNSUPPORTED and b"256" in eng._lib.dyf_last_error(eng._h)
    assert call(points=0, stride=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(points=8, stride=7) == L.DYF_ERR_INVALID_ARGUMENT  # member_stride < n_points
    assert call(outp=0) == L.DYF_ERR_INVALID_ARGUMENT
    assert call(preds=(C.c_void_p * 1)(None)) == L.DYF_ERR_INVALID_ARGUMENT
    torch.cuda.synchronize()


def test_form_is_noted_in_the_form_log():
    eng = _engine()
    preds, truth = _inputs(5, 2, (70,))
    eng.form_log(True)
    try:
        eng.ensemble_size_metrics(preds.cuda(), truth.cuda())
        eng.ensemble_size_metrics(*_as_lists(*_inputs(65, 1, (70,))))
        log = eng.form_log_read()
    finally:
        eng.form_log(False)
    assert log.get("ensemble_size_metrics_kernel:lds_transpose") == {0: 1}
    assert log.get("ensemble_size_metrics_kernel:lds_transpose+wave") == {0: 1}


def test_per_member_mse():
    from dyffusion_amd.metrics import evaluate_ensemble_prediction, evaluate_per_member_mse

    eng = _engine()
    preds, truth = _inputs(8, 6, (2, 11, 5))
    dp, dt = preds.cuda(), truth.cuda()
    per_mem = refs.mse_per_member(preds.numpy(), truth.numpy())
    got = evaluate_per_member_mse(dp, dt, eng)
    assert list(got) == ["mse_per_mem", "mse_per_mem_mean"]
    assert isinstance(got["mse_per_mem"], np.ndarray) and got["mse_per_mem"].shape == (8,) and got["mse_per_mem"].dtype == np.float64
    assert got["mse_per_mem"] == pytest.approx(per_mem, rel=REL)
    assert isinstance(got["mse_per_mem_mean"], float) and got["mse_per_mem_mean"] == pytest.approx(float(per_mem.mean()), rel=REL)
    # per sample: device tensors; the mean over the equal-sized samples is the reference's all-axes mean
    got = evaluate_per_member_mse(dp, dt, eng, mean_over_samples=False)
    assert list(got) == ["mse_per_mem", "mse_per_mem_mean"]
    assert got["mse_per_mem"].is_cuda and got["mse_per_mem"].dtype == torch.float64 and tuple(got["mse_per_mem"].shape) == (8,)
    assert got["mse_per_mem_mean"].is_cuda and got["mse_per_mem_mean"].dtype == torch.float64 and got["mse_per_mem_mean"].dim() == 0
    assert got["mse_per_mem"].cpu().numpy() == pytest.approx(per_mem, rel=REL)
    assert float(got["mse_per_mem_mean"]) == pytest.approx(float(per_mem.mean()), rel=REL)
    # the one-member ensemble's mse is member 0's own: the two kernels agree
    one = evaluate_ensemble_prediction(dp[:1], dt, eng)
    assert evaluate_per_member_mse(dp, dt, eng)["mse_per_mem"][0] == pytest.approx(one["mse"], rel=REL)


def test_varying_members_and_size_curve_keys():
    from dyffusion_amd.metrics import (eval_ensemble_predictions, eval_ensemble_size_curves,
                                       evaluate_ensemble_prediction_for_varying_members)

    eng = _engine()
    n = 6
    preds, truth = _inputs(n, 3, (4, 2, 9, 7))  # three horizons of (N, B = 4, C, H, W) forecasts
    ref = [refs.prefix_reference(preds[:, k].numpy(), truth[k].numpy()) for k in range(3)]  # (4, N) each
    got = evaluate_ensemble_prediction_for_varying_members(preds[:, 0].cuda(), truth[0].cuda(), eng)
    assert list(got) == ["ssr", "crps", "mse"]
    for m in got:
        assert len(got[m]) == n and all(isinstance(v, float) for v in got[m])
        assert got[m][1:] == pytest.approx(ref[0][refs.ROWS.index(m), 1:], rel=REL), m
    assert got["ssr"][0] == 0.0 and got["mse"][0] == pytest.approx(ref[0][0, 0], rel=REL)
    results = {}
    for k in range(3):
        results[f"t{k + 1}_preds"], results[f"t{k + 1}_targets"] = preds[:, k].cuda(), truth[k].cuda()
    curves = eval_ensemble_size_curves(results, eng, "val")
    assert set(curves) == {f"val/{j}ens_mems/{t}/{m}" for j in range(1, n) for t in ("t1", "t2", "t3", "avg") for m in ("ssr", "crps", "mse")}
    for j in range(1, n):
        for k in range(3):
            want = om.evaluate_ensemble_prediction(preds[:j, k].numpy(), truth[k].numpy())
            for m in ("ssr", "crps", "mse"):
                v = curves[f"val/{j}ens_mems/t{k + 1}/{m}"]
                assert v == (0.0 if (m, j) == ("ssr", 1) else pytest.approx(want[m], rel=REL)), (j, k, m)
        for m in ("ssr", "crps", "mse"):
            assert curves[f"val/{j}ens_mems/avg/{m}"] == pytest.approx(np.mean([curves[f"val/{j}ens_mems/t{k}/{m}"] for k in (1, 2, 3)]))
    assert not set(curves) & set(eval_ensemble_predictions(results, eng, "val", infix=f"{n}ens_mems/"))  # n = N stays where it is


def test_accumulator_by_size():
    from dyffusion_amd.metrics import TrajectoryMetricsAccumulator

    eng = _engine()
    plain, acc = TrajectoryMetricsAccumulator(eng), TrajectoryMetricsAccumulator(eng, by_size=True)
    assert acc.compute() == {}
    want = []
    for i, b in enumerate((3, 1)):
        preds, truth = _inputs(5, 4, (b, 2, 9, 7), seed=40 + i)
        assert torch.equal(acc.update(*_as_lists(preds, truth)), plain.update(*_as_lists(preds, truth)))
        want.append(refs.segment_reference(preds.numpy(), truth.numpy()))
    got, base = acc.compute(), plain.compute()
    assert list(got) == ["mse", "ssr", "crps", "by_size"] and list(base) == ["mse", "ssr", "crps"]
    assert all(np.array_equal(got[k], base[k]) for k in base)
    assert got["by_size"].shape == (4, 4, 5) and got["by_size"].dtype == np.float64
    _check(torch.from_numpy(got["by_size"]), np.mean(np.stack(want), axis=0))
    with pytest.raises(ValueError):
        acc.update(*_as_lists(*_inputs(6, 4, (1, 2, 9, 7))))  # six members after five
    acc.reset()
    assert acc.compute() == {}


def _tiny_experiment(n, flag, **kwargs):
    import dyffusion_amd as D
    from tests.gpu_common import build_dyffusion, seeded_pair

    mk = dict(dim=8, outer_sample_mode="bilinear", upsample_dims=[64, 64], with_time_emb=True, input_dropout=0.0, dropout=0.2)
    hp = dict(timesteps=3, forward_conditioning="none", interpolate_before_t1=True, schedule="before_t1_only",
              sampling_type="cold", refine_intermediate_predictions=True, enable_interpolator_dropout=True)
    if not hasattr(_tiny_experiment, "model"):
        PF, PI = seeded_pair(8, 2, 1)
        _tiny_experiment.model = build_dyffusion(PF, PI, mk, 2, 1, hp, max_batch=n * 3)
    _tiny_experiment.model.seed(7)
    return D.MultiHorizonForecastingDYffusion(_tiny_experiment.model, num_predictions=n, window=1, ensemble_size_curves=flag, **kwargs)


def _batches(t):
    from tests.gpu_common import DEV

    g = torch.Generator().manual_seed(2)
    return [{"dynamics": torch.randn(b, 1 + t, 2, 19, 13, generator=g).to(DEV), "condition": torch.rand(b, 1, 19, 13, generator=g).to(DEV)}
            for b in (3, 2)]


def test_validation_epoch_with_ensemble_size_curves():
    """validation_step x 2 + on_validation_epoch_end with the flag: the keys of the first n members, n < N, against the oracle on
    the prefixes of the pooled fields; every key of the flag-off epoch over the same fields keeps its bits."""
    N = 4
    exp = _tiny_experiment(N, True)
    outs = [exp.validation_step(batch, 0) for batch in _batches(3)]
    eng, served = exp.model._engine, []
    pooled_kernel = eng.ensemble_metrics
    eng.ensemble_metrics = lambda p, t: served.append(pooled_kernel(p, t)) or served[-1]  # what ensemble_metrics_kernel returns
    try:
        got = exp.on_validation_epoch_end()
    finally:
        del eng.ensemble_metrics
    # the N-member keys are, bit for bit, what the kernel they come from today returned for the three horizons
    assert len(served) == 3
    for k, (mse, ssr, crps) in enumerate(served, start=1):
        assert (got[f"val/{N}ens_mems/t{k}/mse"], got[f"val/{N}ens_mems/t{k}/ssr"], got[f"val/{N}ens_mems/t{k}/crps"]) == (mse, ssr, crps)
    off = _tiny_experiment(N, False)
    off.__dict__["_validation_step_outputs"] = list(outs)  # the same fields through the epoch end without the flag
    base = off.on_validation_epoch_end()
    # ensemble_metrics_kernel adds its fp64 wave sums with atomics, in an order that differs from launch to launch: two launches
    # over the same 2470 points agree to (terms - 1) * 2^-53 = 2.7e-13 relative, not to the bit
    assert len(base) == 12 and all(got[k] == pytest.approx(base[k], rel=1e-12) for k in base)
    assert set(got) - set(base) == {f"val/{n}ens_mems/{t}/{m}" for n in range(1, N) for t in ("t1", "t2", "t3", "avg")
                                    for m in ("ssr", "crps", "mse")}
    for k in (1, 2, 3):
        preds = torch.cat([o[f"t{k}_preds"] for o in outs], dim=1).cpu().numpy()     # (N, 5, C, H, W)
        targets = torch.cat([o[f"t{k}_targets"] for o in outs], dim=0).cpu().numpy()
        ref = refs.prefix_reference(preds, targets)
        for n in range(1, N):
            for i, m in enumerate(("mse", "ssr", "crps")):
                v = got[f"val/{n}ens_mems/t{k}/{m}"]
                assert v == (0.0 if (m, n) == ("ssr", 1) else pytest.approx(ref[i, n - 1], rel=REL)), (k, n, m)
    assert got["val/2ens_mems/avg/crps"] == pytest.approx(np.mean([got[f"val/2ens_mems/t{k}/crps"] for k in (1, 2, 3)]))


def test_physical_systems_test_epoch_with_ensemble_size_curves():
    """test_step x 2 + on_test_epoch_end for a PhysicalSystemsBenchmarkDataModule with the flag: test/{n}ens_mems/t{i}/{m} is the
    mean over the instances of the per-prefix reference; the flag-off epoch over the same fields keeps its bits."""
    N, T = 4, 6
    cfg = {"_target_": "src.datamodules.physical_systems_benchmark.PhysicalSystemsBenchmarkDataModule"}
    exp = _tiny_experiment(N, True, autoregressive_steps=1, datamodule_config=cfg)
    assert exp.prediction_horizon == T
    batches = _batches(T)
    outs = [exp.test_step({k: v.clone() for k, v in batch.items()}, i) for i, batch in enumerate(batches)]
    got = exp.on_test_epoch_end()
    assert exp.on_test_epoch_end() == {}
    off = _tiny_experiment(N, False, autoregressive_steps=1, datamodule_config=cfg)
    off.evaluation_step = lambda batch, batch_idx=0, split="test", **kw: outs[batch_idx]  # the same fields without the flag
    for i, batch in enumerate(batches):
        off.test_step(batch, i)
    base = off.on_test_epoch_end()
    assert len(base) == 3 * (T + 1) and all(got[k] == base[k] for k in base)
    assert set(got) - set(base) == {f"test/{n}ens_mems/{t}/{m}" for n in range(1, N) for t in [f"t{i}" for i in range(1, T + 1)] + ["avg"]
                                    for m in ("ssr", "crps", "mse")}
    per_instance = []
    for o in outs:
        preds = torch.stack([o[f"t{k}_preds"] for k in range(1, T + 1)], dim=1).cpu().numpy()      # (N, T, B, C, H, W)
        targets = torch.stack([o[f"t{k}_targets"] for k in range(1, T + 1)], dim=0).cpu().numpy()  # (T, B, C, H, W)
        per_instance.append(refs.segment_reference(preds, targets))
    want = np.mean(np.stack(per_instance), axis=0)  # (4, T, N)
    for n in range(1, N):
        for r, m in enumerate(("mse", "ssr", "crps")):
            for i in range(T):
                v = got[f"test/{n}ens_mems/t{i + 1}/{m}"]
                assert v == (0.0 if (m, n) == ("ssr", 1) else pytest.approx(want[r, i, n - 1], rel=REL)), (n, m, i)
            assert got[f"test/{n}ens_mems/avg/{m}"] == pytest.approx(want[r, :, n - 1].mean(), rel=REL, abs=0.0 if (m, n) != ("ssr", 1) else 1e-300)

    class DM:
        test_set_name = "test_hard"

    exp._datamodule = DM()  # the datamodule's split name becomes a level of the keys
    exp.test_step({k: v.clone() for k, v in batches[1].items()}, 0, boundary_conditions=None)
    assert set(exp.on_test_epoch_end()) == {k.replace("test/", "test/test_hard/", 1) for k in got}
