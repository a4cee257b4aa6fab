"""-m gpu: the forecast products on the device (dyf_ensemble_products, HipEngine.ensemble_products) against the float64 / exact
references and the derived bounds of tests/ensemble_products_refs.py (nothing here is tuned to what the device returns).

Forms: up to 64 members one thread per point, 256 points per workgroup; beyond, P points per workgroup and 256 / P threads per point
(P = 128 at 65 members, 64 at 130, 32 at 300).  So 64 | 65 is the form boundary, 255 / 257 / 1000 points are partial last tiles of
either form, 1 point leaves one live thread, and 257 and 1000 are no multiple of any tiled P that divides 256."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import ensemble_products_refs as refs
from tests.test_gpu_ensemble_size_metrics import _engine

pytestmark = pytest.mark.gpu
MEMBERS = (1, 2, 3, 7, 50, 64, 65, 130, 300)
_INPUTS = {}


def _members(n, points, rounded, seed=0):
    key = (n, points, rounded, seed)
    if key not in _INPUTS:
        _INPUTS[key] = refs.members(n, points, seed=seed, rounded=rounded)[1]
    return _INPUTS[key]


def _planes(fields, names):
    return {name: fields[k].reshape(-1).cpu().numpy() for k, name in enumerate(names)}


def _same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype == torch.float32 and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _check(fields, names, x, spec, what=""):
    assert names == refs.plane_names(**spec) and fields.dtype == torch.float32 and fields.is_cuda
    got = _planes(fields, names)
    used = refs.check_products(got, x, **spec)
    print(what, {k: round(v, 3) for k, v in used.items() if v})
    if "q0" in got and "min" in got:
        assert np.array_equal(got["q0"], got["min"], equal_nan=True) and np.array_equal(got["q1"], got["max"], equal_nan=True)
    return got


@pytest.mark.parametrize("rounded", [False, True], ids=["spread", "ties"])
@pytest.mark.parametrize("n", MEMBERS)
def test_one_tensor_all_planes(n, rounded):
    eng = _engine()
    x = _members(n, 257, rounded)
    preds = torch.from_numpy(x).reshape(n, 1, 257).cuda()
    fields, names = eng.ensemble_products(preds, **refs.FULL_SPEC)
    assert tuple(fields.shape) == (len(names), 1, 257)
    got = _check(fields, names, x, refs.FULL_SPEC, f"N{n}")
    if n % 2 == 1:  # the median of an odd ensemble is a member
        assert refs.equal_as_numbers(got["q0.5"], refs.sorted_members(x)[n // 2])
    again, _ = eng.ensemble_products(preds, **refs.FULL_SPEC)
    assert _same_bits(again, fields)  # identical calls, identical bits


@pytest.mark.parametrize("points", [1, 255, 257, 1000])
@pytest.mark.parametrize("n", [7, 65, 130])
def test_point_counts(n, points):
    eng = _engine()
    x = _members(n, points, True)
    fields, names = eng.ensemble_products(torch.from_numpy(x).cuda(), **refs.FULL_SPEC)
    assert tuple(fields.shape) == (len(names), points)
    _check(fields, names, x, refs.FULL_SPEC, f"N{n} P{points}")


@pytest.mark.parametrize("n", [3, 50, 64, 65, 300])
def test_segments_are_independent_and_read_in_place(n):
    """A list of 3 separately allocated segments: every segment against its reference, bit-equal to the segment computed alone; the
    strided form at the C level -- one (N, S, P) buffer, member stride S * P -- writes the same bits, overwrites a sentinel in
    exactly [S][K][P] and leaves the guard region behind it alone."""
    eng = _engine()
    points, segs = 263, 3
    xs = [refs.members(n, points, seed=s, rounded=True, offset=0.1 + s)[1] for s in range(segs)]
    plist = [torch.from_numpy(x).reshape(n, 1, points).cuda() for x in xs]
    spec = dict(mean=True, std=True, min=True, max=False, quantiles=(0.05, 0.5, 0.95), exceed=(0.25,))
    fields, names = eng.ensemble_products(plist, **spec)
    k = len(names)
    assert tuple(fields.shape) == (segs, k, 1, points)
    for s in range(segs):
        _check(fields[s], names, xs[s], spec, f"N{n} segment {s}")
        alone, _ = eng.ensemble_products(plist[s], **spec)
        assert _same_bits(alone, fields[s]), s
    # the strided form
    from dyffusion_amd import _lib
    stack = torch.stack([p.reshape(n, points) for p in plist], dim=1).contiguous()  # (N, S, P)
    cspec = _lib.ProductsSpec(mean=1, std=1, min=1, max=0, n_quantiles=3, n_thresholds=1)
    cspec.quantiles[0], cspec.quantiles[1], cspec.quantiles[2], cspec.thresholds[0] = 0.05, 0.5, 0.95, 0.25
    guard = 4096
    out = torch.full((segs * k * points + guard,), -12345.0, dtype=torch.float32, device="cuda")
    ptrs = (C.c_void_p * segs)(*[stack.data_ptr() + 4 * s * points for s in range(segs)])
    eng._check(eng._lib.dyf_ensemble_products(eng._h, segs, ptrs, n, points, segs * points, C.byref(cspec), out.data_ptr(), eng._stream()))
    torch.cuda.synchronize()
    assert _same_bits(out[:segs * k * points].reshape(segs, k, 1, points), fields)
    assert not torch.any(out[:segs * k * points] == -12345.0) and torch.all(out[segs * k * points:] == -12345.0)


@pytest.mark.parametrize("n", [7, 130])
def test_single_plane_specs(n):
    eng = _engine()
    x = _members(n, 300, True)
    preds = torch.from_numpy(x).cuda()
    full, full_names = eng.ensemble_products(preds, **refs.FULL_SPEC)
    for spec in (dict(mean=True, std=False), dict(mean=False, std=True), dict(mean=False, std=False, max=True),
                 dict(mean=False, std=False, quantiles=(1.0 / 3.0,)), dict(mean=False, std=False, exceed=(1.0,))):
        fields, names = eng.ensemble_products(preds, **spec)
        assert tuple(fields.shape) == (1, 300) and len(names) == 1
        _check(fields, names, x, spec, f"N{n} {names[0]}")
        assert _same_bits(fields[0], full[full_names.index(names[0])])  # a plane does not depend on the others asked for


@pytest.mark.parametrize("n", [7, 64, 65])
def test_nan_member_poisons_exactly_its_point(n):
    eng = _engine()
    x = _members(n, 300, False).copy()
    clean, names = eng.ensemble_products(torch.from_numpy(x).cuda(), **refs.FULL_SPEC)
    x[n // 2, 131] = np.nan
    fields, _ = eng.ensemble_products(torch.from_numpy(x).cuda(), **refs.FULL_SPEC)
    got = _check(fields, names, x, refs.FULL_SPEC, f"N{n} NaN")
    for k, name in enumerate(names):
        if name.startswith("gt"):
            assert not np.any(np.isnan(got[name]))
        else:
            assert np.isnan(got[name][131]) and np.isnan(got[name]).sum() == 1
        keep = torch.arange(300, device="cuda") != 131
        assert _same_bits(fields[k][keep], clean[k][keep]), name  # the neighbours keep their bits


def test_infinite_members_in_min_max_and_exceedance():
    eng = _engine()
    x = _members(7, 64, False).copy()
    x[2, 5], x[4, 9] = np.inf, -np.inf
    spec = dict(mean=False, std=False, min=True, max=True, exceed=(0.0, float("inf")))
    fields, names = eng.ensemble_products(torch.from_numpy(x).cuda(), **spec)
    got = _planes(fields, names)
    assert np.array_equal(got["min"], x.min(axis=0)) and np.array_equal(got["max"], x.max(axis=0))
    assert np.array_equal(got["gt0"], (x > 0).sum(axis=0).astype(np.float32) / np.float32(7)) and np.all(got["gtinf"] == 0.0)


def test_argument_errors():
    eng = _engine()
    preds = torch.zeros(4, 10, device="cuda")
    for bad in (dict(mean=False, std=False), dict(quantiles=(1.5,)), dict(quantiles=(-0.1,)), dict(quantiles=(float("nan"),)),
                dict(exceed=(float("nan"),)), dict(quantiles=[0.5] * 17), dict(exceed=[0.5] * 17), dict(quantiles="ab")):
        with pytest.raises(ValueError):
            eng.ensemble_products(preds, **bad)
    with pytest.raises(ValueError, match="GPU tensors"):
        eng.ensemble_products(preds.cpu())
    with pytest.raises(ValueError):
        eng.ensemble_products([])
    # non-contiguous and non-fp32 inputs are made contiguous fp32 first
    x = _members(5, 40, True)
    want, _ = eng.ensemble_products(torch.from_numpy(x).cuda(), quantiles=(0.5,))
    got, _ = eng.ensemble_products(torch.from_numpy(x.T.copy()).cuda().T.double(), quantiles=(0.5,))
    assert _same_bits(got, want)
    # the C level: member counts beyond 15 360 and segment counts beyond 65 535 are unsupported, not invalid
    from dyffusion_amd import _lib
    spec = _lib.ProductsSpec(mean=1)
    out = torch.zeros(16, device="cuda")
    ptrs = (C.c_void_p * 1)(preds.data_ptr())
    assert eng._lib.dyf_ensemble_products(eng._h, 1, ptrs, 15361, 1, 1, C.byref(spec), out.data_ptr(), eng._stream()) == _lib.DYF_ERR_UNSUPPORTED
    many = (C.c_void_p * 65536)(*([preds.data_ptr()] * 65536))
    assert eng._lib.dyf_ensemble_products(eng._h, 65536, many, 4, 1, 10, C.byref(spec), out.data_ptr(), eng._stream()) == _lib.DYF_ERR_UNSUPPORTED
    assert eng._lib.dyf_ensemble_products(eng._h, 1, ptrs, 4, 10, 9, C.byref(spec), out.data_ptr(), eng._stream()) == _lib.DYF_ERR_INVALID_ARGUMENT
    assert eng._lib.dyf_ensemble_products(eng._h, 1, ptrs, 0, 10, 10, C.byref(spec), out.data_ptr(), eng._stream()) == _lib.DYF_ERR_INVALID_ARGUMENT
    with pytest.raises(NotImplementedError):
        eng._check(eng._lib.dyf_ensemble_products(eng._h, 1, ptrs, 15361, 1, 1, C.byref(spec), out.data_ptr(), eng._stream()))
