"""The references of the energy score, on the CPU (tests/energy_score_refs.py):

  * header, ctypes table, tile constant and ABI version agree on dyf_energy_score;
  * the float64 reference equals torch.cdist in float64 on the permuted copy, the oracle's CRPS where a vector is one point, and the
    closed form of two members;
  * the fp32 emulation of the kernel's stated arithmetic stays within HALF the derived bound on every case of the GPU tests, so the
    device has room;
  * every mutant of the emulation misses the bound by at least a factor of ten on the case that targets it
    (refs.MUTANT_CASE): the GPU tests can tell them apart.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from tests import energy_score_refs as refs

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))


def test_header_binding_tile_constant_and_abi_version_agree():
    from dyffusion_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "dyffusion_hip.h")).read()
    assert re.search(r"^#define\s+DYF_ABI_VERSION\s+9\s*$", hdr, re.M) and _lib.DYF_ABI_VERSION == 9
    tile = re.search(r"^#define\s+DYF_ENERGY_TILE_POINTS\s+(\d+)\s*$", hdr, re.M)
    assert tile and int(tile.group(1)) == _lib.ENERGY_TILE_POINTS == refs.K and refs.K <= 256
    most = re.search(r"^#define\s+DYF_ENERGY_MAX_MEMBERS\s+(\d+)\s*$", hdr, re.M)
    assert most and int(most.group(1)) == _lib.ENERGY_MAX_MEMBERS == 256
    cap = re.search(r"^#define\s+DYF_ENERGY_MAX_WORKSPACE_DOUBLES\s+(\d+)\b", hdr, re.M)
    assert cap and int(cap.group(1)) == _lib.ENERGY_MAX_WORKSPACE_DOUBLES
    m = re.search(r"dyf_status\s+dyf_energy_score\s*\(([^;]*)\)\s*;", hdr)
    assert m, "dyf_energy_score is not declared in include/dyffusion_hip.h"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == ["dyf_engine* engine", "int32_t n_segments", "const float* const* preds_dev", "const float* const* targets_dev",
                      "int32_t n_members", "int64_t n_points", "int64_t member_stride", "int64_t n_outer", "int32_t n_groups",
                      "int64_t n_inner", "double* out_dev", "double* member_out_dev", "double* pair_out_dev", "double* accum_dev",
                      "void* stream"]
    rows = [s for s in _lib.SYMBOLS if s[0] == "dyf_energy_score"]
    assert len(rows) == 1 and rows[0][1] is C.c_int and len(rows[0][2]) == len(params)
    src = open(os.path.join(ROOT, "dyffusion_amd", "csrc", "kernels.h")).read()
    assert re.search(r"ENERGY_SCORE_TILE_POINTS\s*=\s*%d\s*;" % refs.K, src)
    import __graft_entry__ as entry
    assert "energy_score.hip" in entry.SOURCES


def test_cases_cover_the_limits():
    ns = {s[0] for s in refs.SHAPES.values()}
    inner = {s[2][2] for s in refs.SHAPES.values()}
    assert {1, 2, 3, 5, 63, 64, 65, 130, 256} <= ns
    assert {1, 3, refs.K - 1, refs.K, refs.K + 1, 2 * refs.K + 5} <= inner
    assert {s[2][0] for s in refs.SHAPES.values()} >= {1, 3} and {s[2][1] for s in refs.SHAPES.values()} >= {1, 3}
    assert {s[3] for s in refs.SHAPES.values()} == {"tensor", "list"}
    assert any(s[3] == "tensor" and s[1] == 2 for s in refs.SHAPES.values())  # member_stride != n_points
    assert set(refs.MUTANT_CASE) == set(refs.MUTANTS) and set(refs.MUTANT_CASE.values()) <= set(refs.SHAPES)
    for name in refs.SHAPES:
        c = refs.case(name)
        assert c.preds.nbytes < (1 << 20), name  # every tensor under a megabyte


@pytest.mark.parametrize("name", list(refs.SHAPES))
def test_reference_equals_cdist_on_the_permuted_copy(name):
    c, ref = refs.case(name), refs.reference(name)
    o, g, i = c.group_shape
    for s in range(c.segs):
        x = torch.from_numpy(c.preds[:, s].astype(np.float64)).reshape(c.n, o, g, i).permute(1, 2, 0, 3)  # (outer, groups, N, inner)
        y = torch.from_numpy(c.targets[s].astype(np.float64)).reshape(o, g, 1, i)
        pair = torch.cdist(x, x, compute_mode="donot_use_mm_for_euclid_dist").mean(dim=0).numpy()  # (groups, N, N)
        member = torch.cdist(x, y, compute_mode="donot_use_mm_for_euclid_dist")[..., 0].mean(dim=0).numpy()  # (groups, N)
        ok = ~np.isnan(ref["pair"][s])
        apart = np.broadcast_to(~np.eye(c.n, dtype=bool), ok.shape)  # the reference's diagonal is 0 by definition, never computed
        assert np.array_equal(np.isnan(pair)[apart], ~ok[apart])
        off = ok & apart
        assert np.allclose(pair[off], ref["pair"][s][off], rtol=1e-12, atol=1e-15)
        okm = ~np.isnan(ref["member"][s])
        assert np.allclose(member[okm], ref["member"][s][okm], rtol=1e-12, atol=0)
        for k in range(g):
            if ok[k].all() and c.n > 1:
                dt, dp = member[k].mean(), pair[k].sum() / (c.n * (c.n - 1))
                want = [dt - (c.n - 1) / (2.0 * c.n) * dp, dt - dp / 2, dt, dp]
                assert np.allclose(ref["planes"][:, s, k], want, rtol=1e-12, atol=0)


@pytest.mark.parametrize("name", ["n63", "n63_points", "n1"])
def test_one_point_vectors_give_the_crps(name):
    from oracle import metrics as om

    c, ref = refs.case(name), refs.reference(name)
    o, g, i = c.group_shape
    for s in range(c.segs):
        x, y = c.preds[:, s].reshape(c.n, o, g, i), c.targets[s].reshape(o, g, i)
        for k in range(g):
            if i == 1:
                assert ref["planes"][0, s, k] == pytest.approx(om.crps_ensemble(x[:, :, k], y[:, k]), rel=1e-12)
            else:  # one member: the energy score is its distance, whatever the vector
                assert ref["planes"][0, s, k] == ref["planes"][2, s, k] and np.isnan(ref["planes"][1, s, k]) and np.isnan(ref["planes"][3, s, k])


def test_two_members_closed_form():
    c, ref = refs.case("n2"), refs.reference("n2")
    x, y = c.preds[:, 0].astype(np.float64), c.targets[0].astype(np.float64)
    d1, d2, d12 = np.linalg.norm(x[0] - y), np.linalg.norm(x[1] - y), np.linalg.norm(x[0] - x[1])
    want = [(d1 + d2) / 2 - d12 / 4, (d1 + d2) / 2 - d12 / 2, (d1 + d2) / 2, d12]
    assert np.allclose(ref["planes"][:, 0, 0], want, rtol=1e-12, atol=0)
    assert np.allclose(ref["member"][0, 0], [d1, d2], rtol=1e-12) and np.allclose(ref["pair"][0, 0], [[0, d12], [d12, 0]], rtol=1e-12)


def test_special_cases_are_what_they_claim():
    twins = refs.reference("twins")["pair"]
    assert np.all(twins[:, :, 1, 3] == 0.0) and np.all(twins[:, :, 3, 1] == 0.0) and np.all(twins[:, :, 0, 1] > 0.0)
    close = refs.reference("close")["pair"]
    assert np.allclose(close[:, :, 1, 2], 1e-3, rtol=1e-3)
    nan, at = refs.reference("nan"), refs.NAN_AT
    bad = np.zeros(nan["planes"].shape[1:], dtype=bool)
    bad[at["segment"], at["group"]] = True
    assert np.array_equal(np.isnan(nan["planes"]), np.broadcast_to(bad, nan["planes"].shape))
    m = np.isnan(nan["member"])
    assert m.sum() == 1 and m[at["segment"], at["group"], at["member"]]
    p = np.isnan(nan["pair"][at["segment"], at["group"]])
    want = np.zeros_like(p)
    want[at["member"], :] = want[:, at["member"]] = True
    want[at["member"], at["member"]] = False
    assert np.array_equal(p, want) and np.isnan(nan["pair"]).sum() == want.sum()
    one = refs.reference("n1")
    assert np.all(np.isnan(one["planes"][[1, 3]])) and np.array_equal(one["planes"][0], one["planes"][2]) and np.all(one["pair"] == 0.0)


@pytest.mark.parametrize("name", list(refs.SHAPES))
def test_emulation_sits_inside_half_the_bound(name):
    c, ref = refs.case(name), refs.reference(name)
    got = refs.evaluate(c, refs.emulate_segment)
    worst = refs.worst_ratio(got, ref, c.n)
    print(f"{name}: emulation / bound = {worst:.3f}")
    assert worst <= 0.5
    assert np.array_equal(got["pair"], np.swapaxes(got["pair"], -1, -2)) or name == "nan"
    idx = np.arange(c.n)
    assert np.all(got["pair"][..., idx, idx] == 0.0)


@pytest.mark.parametrize("mutant", refs.MUTANTS)
def test_every_mutant_misses_the_bound_tenfold_on_its_case(mutant):
    name = refs.MUTANT_CASE[mutant]
    c, ref = refs.case(name), refs.reference(name)
    got = refs.evaluate(c, refs.emulate_segment, mutant)
    worst = refs.worst_ratio(got, ref, c.n, keys=tuple(got))
    print(f"{mutant} on {name}: error / bound = {worst:.3g}")
    assert worst >= 10.0
