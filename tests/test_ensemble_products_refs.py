"""The references of the ensemble products and the rank histogram, on the CPU (tests/ensemble_products_refs.py):

  * header, ctypes table and ABI version agree on dyf_ensemble_products, dyf_products_spec and dyf_rank_histogram;
  * the fp32 emulation of the kernel's stated expressions equals the float64 / exact reference where the contract says "equal as
    numbers", and stays within HALF of each derived bound on the inputs of the GPU tests, so the device has room;
  * every mutant of the emulation misses a bound or an equality on those inputs: the GPU tests can tell them apart;
  * the host surface that needs no GPU: names, defaults, the refusal of CPU tensors, the key layout of the epoch ends.
"""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import ensemble_products_refs as refs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
MEMBERS = (1, 2, 3, 7, 50, 64, 65, 130, 300)
POINTS = 257


def _params(hdr, name):
    m = re.search(r"dyf_status\s+" + name + r"\s*\(([^;]*)\)\s*;", hdr)
    assert m, f"{name} is not declared in include/dyffusion_hip.h"
    return [" ".join(p.split()) for p in m.group(1).split(",")], m


def test_header_binding_and_abi_version_agree():
    from dyffusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "dyffusion_hip.h")).read()
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", hdr, re.M) and _lib.DYF_ABI_VERSION == 9
    assert re.search(r"^#define\s+DYF_MAX_PRODUCT_QUANTILES\s+16\s*$", hdr, re.M) and _lib.MAX_PRODUCT_QUANTILES == 16
    assert re.search(r"^#define\s+DYF_MAX_PRODUCT_THRESHOLDS\s+16\s*$", hdr, re.M) and _lib.MAX_PRODUCT_THRESHOLDS == 16
    struct = re.search(r"typedef struct dyf_products_spec \{(.*?)\} dyf_products_spec;", hdr, re.S)
    assert struct, "dyf_products_spec is not declared"
    body = re.sub(r"/\*.*?\*/", "", struct.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t mean, std, min, max", "int32_t n_quantiles", "double quantiles[DYF_MAX_PRODUCT_QUANTILES]",
                      "int32_t n_thresholds", "float thresholds[DYF_MAX_PRODUCT_THRESHOLDS]"]
    assert [(n, t) for n, t in _lib.ProductsSpec._fields_] == [
        ("mean", C.c_int32), ("std", C.c_int32), ("min", C.c_int32), ("max", C.c_int32), ("n_quantiles", C.c_int32),
        ("quantiles", C.c_double * 16), ("n_thresholds", C.c_int32), ("thresholds", C.c_float * 16)]
    assert C.sizeof(_lib.ProductsSpec) == 16 + 8 + 128 + 8 + 64  # n_quantiles and n_thresholds are padded to the doubles' alignment

    want = {"dyf_ensemble_products": ["dyf_engine* engine", "int32_t n_segments", "const float* const* preds_dev", "int32_t n_members",
                                      "int64_t n_points", "int64_t member_stride", "const dyf_products_spec* spec", "float* out_dev",
                                      "void* stream"],
            "dyf_rank_histogram": ["dyf_engine* engine", "int32_t n_segments", "const float* const* preds_dev",
                                   "const float* const* targets_dev", "int32_t n_members", "int64_t n_points", "int64_t member_stride",
                                   "int64_t n_outer", "int32_t n_groups", "int64_t n_inner", "double* out_dev", "double* accum_dev",
                                   "void* stream"]}
    for name, params in want.items():
        got, m = _params(hdr, name)
        assert got == params, name
        rows = [s for s in _lib.SYMBOLS if s[0] == name]
        assert len(rows) == 1 and rows[0][1] is C.c_int and len(rows[0][2]) == len(params), name
        for arg, p in zip(rows[0][2], params):
            if p.startswith("int32_t"):
                assert arg is C.c_int32, (name, p)
            elif p.startswith("int64_t"):
                assert arg is C.c_int64, (name, p)
            elif p.startswith("const float* const*"):
                assert arg == C.POINTER(C.c_void_p), (name, p)
            elif p.startswith("const dyf_products_spec*"):
                assert arg == C.POINTER(_lib.ProductsSpec), (name, p)
            else:
                assert arg is C.c_void_p, (name, p)
        comment = hdr[m.start() - 3200:m.start()].replace("\n * ", " ")
        assert "Does NOT synchronise" in comment and "no atomics" in comment and "Additive: no ABI change" in comment, name
    comment = hdr[_params(hdr, "dyf_rank_histogram")[1].start() - 2400:_params(hdr, "dyf_rank_histogram")[1].start()].replace("\n * ", " ")
    assert "256 x (n_members + 1) doubles" in comment  # the workspace bound is stated


def test_build_lists_the_new_unit():
    import __graft_entry__ as g

    assert "ensemble_products.hip" in g.SOURCES and os.path.exists(os.path.join(g.CSRC, "ensemble_products.hip"))
    kernels = open(os.path.join(g.CSRC, "kernels.hip")).read()
    assert "ensemble_products" not in kernels and "rank_histogram" not in kernels  # the new kernels have their own unit


def _used(n, rounded, fraction, mutant=None, spec=refs.FULL_SPEC, **kw):
    _, x = refs.members(n, POINTS, rounded=rounded, **kw)
    return refs.check_products(refs.emulate_products(x, mutant=mutant, **spec), x, fraction=fraction, **spec)


@pytest.mark.parametrize("n", MEMBERS)
def test_emulation_meets_the_equalities_and_half_of_every_bound(n):
    worst = {}
    for rounded in (False, True):
        for k, v in _used(n, rounded, 0.5).items():
            worst[k] = max(v, worst.get(k, 0.0))
    print(n, {k: round(v, 3) for k, v in worst.items() if v})
    assert all(v <= 0.5 for v in worst.values())
    # the planes the contract calls equal are checked as equalities: min, max, exceedances, quantiles with frac == 0
    _, x = refs.members(n, POINTS, rounded=True)
    got, order = refs.emulate_products(x, **refs.FULL_SPEC), refs.sorted_members(x)
    assert refs.equal_as_numbers(got["q0"], got["min"]) and refs.equal_as_numbers(got["q1"], got["max"])
    assert refs.equal_as_numbers(got["min"], order[0]) and refs.equal_as_numbers(got["max"], order[-1])
    if n % 2 == 1:
        assert refs.order_statistics(n, 0.5)[2] == 0 and refs.equal_as_numbers(got["q0.5"], order[n // 2])
    for t in refs.THRESHOLDS:
        assert refs.equal_as_numbers(got[f"gt{t:g}"], (x > np.float32(t)).sum(axis=0).astype(np.float32) / np.float32(n))
    assert np.any(x == np.float32(0.25)) and np.any(x == np.float32(1.0))  # a threshold that equals member values


def test_bounds_hold_for_the_issue_data():
    """offsets 0, 300, -5, 1e4 x scales 0, 1e-3, 1, 2 and N up to 1000: the emulation stays inside every (full) bound."""
    spec = dict(mean=True, std=True, quantiles=(0.05, 1.0 / 3.0, 0.5, 0.95))
    worst = {}
    for n in (1, 2, 3, 7, 50, 64, 65, 130, 300, 1000):
        for offset in (0.0, 300.0, -5.0, 1e4):
            for scale in (0.0, 1e-3, 1.0, 2.0):
                rng = np.random.default_rng(n)
                x = (offset + scale * rng.normal(size=(n, 40))).astype(np.float32)
                for k, v in refs.check_products(refs.emulate_products(x, **spec), x, **spec).items():
                    worst[k] = max(v, worst.get(k, 0.0))
    print({k: round(v, 3) for k, v in worst.items()})


def test_nan_poisons_its_own_point_only():
    _, x = refs.members(7, 40)
    x[3, 11] = np.nan
    got = refs.emulate_products(x, **refs.FULL_SPEC)
    refs.check_products(got, x, **refs.FULL_SPEC)
    for name, v in got.items():
        if name.startswith("gt"):
            assert not np.any(np.isnan(v)) and v[11] == np.float32((x[:, 11] > np.float32(name[2:])).sum()) / np.float32(7)
        else:
            assert np.isnan(v[11]) and np.isnan(v).sum() == 1, name


def _misses(fn):
    try:
        fn()
    except AssertionError:
        return True
    return False


@pytest.mark.parametrize("mutant", [m for m in refs.PRODUCT_MUTANTS if m != "stride_is_n_points"])
def test_every_product_mutant_is_caught(mutant):
    """On the inputs of the GPU tests: the mutant misses for at least one N of the list, at the FULL bound."""
    caught = [n for n in MEMBERS for rounded in (False, True) if _misses(lambda: _used(n, rounded, 1.0, mutant=mutant))]
    assert caught, mutant
    if mutant not in ("ddof1", "mean_over_n_minus_1", "last_member_ignored"):  # those need two members; the rest more
        assert 50 in caught, (mutant, caught)
    assert not [n for n in MEMBERS for rounded in (False, True) if _misses(lambda: _used(n, rounded, 1.0))]  # the emulation itself passes


def _strided_case(n=7, segs=3, points=41):
    """One (N, S, P) buffer read in place: member stride S * P > P, the segments differ in value."""
    truth = np.stack([refs.members(n, points, seed=s, rounded=True, offset=0.1 + s)[0] for s in range(segs)])
    preds = np.stack([refs.members(n, points, seed=s, rounded=True, offset=0.1 + s)[1] for s in range(segs)], axis=1)
    return truth, preds  # (S, P), (N, S, P)


def test_member_stride_mutant_is_caught():
    truth, preds = _strided_case()
    n, segs, points = preds.shape
    spec = dict(mean=True, min=True, quantiles=(0.5,))
    for s in range(segs):
        x = refs.gather_members(preds, n, points, segs * points, s * points)
        assert np.array_equal(x, preds[:, s])
        refs.check_products(refs.emulate_products(x, **spec), preds[:, s], **spec)
        ref = refs.histogram_reference(preds[:, s], truth[s])
        refs.check_histogram(refs.emulate_histogram(preds, truth, n, points, segs * points, s * points, s * points), ref, tie_free=False)
        wrong = refs.gather_members(preds, n, points, segs * points, s * points, mutant="stride_is_n_points")
        assert _misses(lambda: refs.check_products(refs.emulate_products(wrong, **spec), preds[:, s], **spec))
        got = refs.emulate_histogram(preds, truth, n, points, segs * points, s * points, s * points, mutant="stride_is_n_points")
        assert _misses(lambda: refs.check_histogram(got, ref, tie_free=False))


def test_histogram_reference_and_its_mutants():
    n, points = 7, 2 * 3 * 35
    gs = (2, 3, 35)
    # tie-free: integers, every point in one bin, the bins of a group sum to its points
    truth, preds = refs.members(n, points)
    h = refs.histogram_reference(preds, truth, gs)
    assert h.shape == (3, n + 1) and np.array_equal(h, np.round(h)) and np.array_equal(h.sum(axis=1), [70.0, 70.0, 70.0])
    pooled = refs.histogram_reference(preds, truth)
    assert np.array_equal(pooled[0], h.sum(axis=0))
    assert np.array_equal(pooled[0], np.bincount((preds < truth[None]).sum(axis=0), minlength=n + 1).astype(np.float64))
    # ties and the boundary block: all members equal the truth -> 1 / (N + 1) in every bin
    truth, preds = refs.members(n, points, rounded=True)
    tied = refs.histogram_reference(preds, truth, gs)
    assert tied.sum(axis=1) == pytest.approx([70.0, 70.0, 70.0], rel=1e-12) and not np.array_equal(tied, np.round(tied))
    block = refs.histogram_reference(preds[:, -26:], truth[-26:])
    assert block[0] == pytest.approx(np.full(n + 1, 26.0 / (n + 1)), rel=1e-12)
    # a NaN target or member drops the point
    preds[2, 5], truth[100] = np.nan, np.nan
    dropped = refs.histogram_reference(preds, truth, gs)
    assert dropped.sum() == pytest.approx(points - 2, rel=1e-12)
    for mutant in refs.HISTOGRAM_MUTANTS[:3]:
        assert _misses(lambda: refs.check_histogram(refs.histogram_reference(preds, truth, gs, mutant=mutant), dropped, tie_free=False)), mutant
    f, ri = refs.frequencies(tied)
    assert f.sum(axis=1) == pytest.approx(1.0) and ri.shape == (3,) and np.all(ri >= 0)
    assert refs.frequencies(np.full((1, 5), 3.0))[1][0] == 0.0


class _CudaLike(torch.Tensor):
    """A CPU tensor that says it is on the GPU: the stub engine never reads it."""

    @property
    def is_cuda(self):
        return True


class _StubEngine:
    def __init__(self):
        self.calls = []

    def rank_histogram(self, preds, targets, group_shape=None, accum=None):
        preds = list(preds)
        self.calls.append((len(preds), tuple(preds[0].shape), group_shape))
        n = preds[0].shape[0]
        bins = torch.ones(len(preds), 1 if group_shape is None else group_shape[1], n + 1, dtype=torch.float64)
        bins[:, :, 0] += torch.arange(len(preds), dtype=torch.float64)[:, None] * (n + 1)  # segment s: bin 0 holds s (N + 1) more
        if accum is not None:
            accum += bins
        return bins

    def ensemble_products(self, preds, **spec):
        names = refs.plane_names(**spec)
        one = torch.is_tensor(preds)
        plist = [preds] if one else list(preds)
        out = torch.stack([torch.stack([p[0] * 0 + 10 * s + k for k in range(len(names))]) for s, p in enumerate(plist)])
        return (out[0] if one else out), names


def test_names_defaults_and_host_surface():
    import dyffusion_amd as D
    from dyffusion_amd import metrics as M
    from dyffusion_amd.engine import HipEngine

    p = inspect.signature(HipEngine.ensemble_products).parameters
    assert list(p) == ["self", "preds", "mean", "std", "min", "max", "quantiles", "exceed"]
    assert [p[k].default for k in list(p)[2:]] == [True, True, False, False, (), ()]
    p = inspect.signature(HipEngine.rank_histogram).parameters
    assert list(p) == ["self", "preds", "targets", "group_shape", "accum"] and p["group_shape"].default is None and p["accum"].default is None
    p = inspect.signature(D.MultiHorizonForecastingDYffusion.__init__).parameters
    assert p["predict_products"].default is None and p["keep_members"].default is True and p["rank_histogram"].default is False
    assert inspect.signature(M.TrajectoryMetricsAccumulator.__init__).parameters["rank_histogram"].default is False
    assert list(inspect.signature(M.evaluate_rank_histogram).parameters) == ["predictions", "targets", "engine", "mean_dims"]
    assert refs.plane_names(quantiles=(0.05, 0.5, 0.95), exceed=(0.5,)) == ["mean", "std", "q0.05", "q0.5", "q0.95", "gt0.5"]
    # CPU tensors are refused before anything is launched (self is never used on that path)
    with pytest.raises(ValueError, match="GPU tensors"):
        HipEngine.ensemble_products(None, torch.zeros(3, 4))
    with pytest.raises(ValueError, match="GPU tensors"):
        HipEngine.rank_histogram(HipEngine, [torch.zeros(3, 4)], [torch.zeros(4)])
    with pytest.raises(ValueError, match="GPU tensors"):
        M.evaluate_rank_histogram(torch.zeros(3, 2, 4), torch.zeros(2, 4), None)
    with pytest.raises(ValueError, match="segments differ"):
        HipEngine.ensemble_products(None, [torch.zeros(3, 4), torch.zeros(3, 5)])
    # the dict of names, one tensor and a list
    eng = _StubEngine()
    one = M.ensemble_products(torch.zeros(3, 2, 4), eng, quantiles=(0.5,))
    assert list(one) == ["mean", "std", "q0.5"] and one["q0.5"].shape == (2, 4) and float(one["q0.5"][0, 0]) == 2.0
    many = M.ensemble_products([torch.zeros(3, 2, 4)] * 2, eng, std=False, exceed=(1.5,))
    assert list(many) == ["mean", "gt1.5"] and many["gt1.5"].shape == (2, 2, 4) and float(many["gt1.5"][1, 0, 0]) == 11.0


def test_rank_histogram_key_layout_and_frequencies():
    from dyffusion_amd import metrics as M

    n = 4
    z = lambda *s: torch.zeros(*s).as_subclass(_CudaLike)  # noqa: E731
    eng = _StubEngine()
    got = M.evaluate_rank_histogram(z(n, 2, 3, 5), z(2, 3, 5), eng)
    assert eng.calls == [(1, (n, 2, 3, 5), None)] and got["rank_hist"].shape == (n + 1,) and got["rank_hist"].sum() == pytest.approx(1.0)
    assert got["reliability_index"] == 0.0 and isinstance(got["reliability_index"], float)
    per_c = M.evaluate_rank_histogram(z(n, 2, 3, 5), z(2, 3, 5), eng, mean_dims=(0, 2))
    assert eng.calls[-1] == (1, (n, 2, 3, 5), (2, 3, 5)) and tuple(per_c["rank_hist"].shape) == (3, n + 1)
    assert tuple(per_c["reliability_index"].shape) == (3,)
    results = {"t1_preds": z(n, 2, 3, 5), "t1_targets": z(2, 3, 5), "t2_preds": z(n, 2, 3, 5), "t2_targets": z(2, 3, 5), "t3_preds": z(n, 2, 3, 5)}
    eng.calls.clear()
    keys = M.eval_rank_histograms(results, eng, "val", infix="4ens_mems/")
    assert eng.calls == [(2, (n, 2, 3, 5), None)]  # both horizons as the segments of one call
    assert sorted(keys) == sorted(f"val/4ens_mems/{t}/{m}" for t in ("t1", "t2", "avg") for m in ("rank_hist", "reliability_index"))
    assert isinstance(keys["val/4ens_mems/t2/rank_hist"], np.ndarray) and keys["val/4ens_mems/t2/rank_hist"].shape == (n + 1,)
    # segment 1 of the stub: bins (6, 1, 1, 1, 1) -> frequencies (.6, .1, .1, .1, .1), reliability index .4 + 4 x .1
    assert keys["val/4ens_mems/t2/rank_hist"] == pytest.approx([0.6, 0.1, 0.1, 0.1, 0.1])
    assert keys["val/4ens_mems/t2/reliability_index"] == pytest.approx(0.8) and keys["val/4ens_mems/t1/reliability_index"] == 0.0
    assert keys["val/4ens_mems/avg/reliability_index"] == pytest.approx(0.4)
    assert keys["val/4ens_mems/avg/rank_hist"] == pytest.approx([0.4, 0.15, 0.15, 0.15, 0.15])
    # the accumulator sums the histograms through `accum`; compute() gives the frequencies of the sum
    class _Acc(_StubEngine):
        def trajectory_metrics(self, preds, targets, accum=None):
            return torch.zeros(3, len(list(preds)), dtype=torch.float64)

    acc = M.TrajectoryMetricsAccumulator(_Acc(), rank_histogram=True)
    for _ in range(2):
        acc.update([torch.zeros(n, 2, 6)] * 2, [torch.zeros(2, 6)] * 2)
    out = acc.compute()
    assert out["rank_hist"].shape == (2, n + 1) and out["rank_hist"][1] == pytest.approx([0.6, 0.1, 0.1, 0.1, 0.1])
    assert "rank_hist" not in M.TrajectoryMetricsAccumulator(_Acc()).compute()
