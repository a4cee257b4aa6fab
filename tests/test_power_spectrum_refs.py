"""dyf_power_spectrum without a GPU: the ABI row, the shell rule, the identities of the float64 reference, the fp32 emulation of the
kernel's scheme inside half the derived bound, and ten mutants of the scheme far outside it (tests/power_spectrum_refs.py)."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from tests import power_spectrum_refs as refs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(refs.CASES)

# the cases every mutant can affect: there it must be more than 10 x the bound away from the reference
ALL = NAMES
MUTANT_CASES = {
    # even W.  Not 221x42: there the whole Nyquist column has kappa >= 110.5, shell 111 = n_bins, so it lies in the dropped corners and
    # the mutant changes no shell, only `total`, whose worst-case bound is summed over all 9282 coefficients: measured 5.3 x the bound
    # (test_nyquist_column_of_the_ns_field_is_all_corners holds that to > 1).
    "nyquist_twice": ["2x2", "16x30", "33x34", "33x34_hann", "61x42", "70x70"],
    "dc_twice": ALL,
    "bin_trunc": [n for n in NAMES if n != "2x2"],  # at 2 x 2 kappa is 0, 1, 1, 1.41: floor and round agree
    "isotropic": ["5x3", "13x7", "16x30", "33x34", "33x34_hann", "61x42", "221x42"],  # H != W
    "ky_unfolded": [n for n in NAMES if n != "2x2"],  # H = 2: min(ky, H - ky) = ky
    "norm_hw": ALL,
    "spread_n_minus_1": [n for n in NAMES if refs.CASES[n].n > 1],
    "window_one_axis": [n for n in NAMES if refs.CASES[n].window == "hann"],
    # not 61x42: its Hann taper leaves row H - 1 the weight (1 - cos(2 pi 60 / 61)) / 2 = 2.6e-3, so dropping the row moves a coefficient
    # by less than the worst-case bound allows twice over (measured 3.2 x the bound); the un-tapered and the smaller tapered cases stay
    "last_row_missing": [n for n in NAMES if n != "61x42"],
    "anomaly_vs_target": ALL,
}


def test_header_ctypes_row_and_sources_agree():
    from dyffusion_amd import _lib

    import __graft_entry__ as entry

    with open(os.path.join(ROOT, "include", "dyffusion_hip.h")) as f:
        header = f.read()
    m = re.search(r"dyf_status dyf_power_spectrum\(([^;]*)\);", header)
    assert m, "dyf_power_spectrum is not declared in include/dyffusion_hip.h"
    params = [p.strip() for p in m.group(1).replace("\n", " ").split(",")]
    rows = [r for r in _lib.SYMBOLS if r[0] == "dyf_power_spectrum"]
    assert len(rows) == 1 and len(rows[0][2]) == len(params) == 14
    kinds = ["int32" if p.startswith("int32_t") else "int64" if p.startswith("int64_t") else "ptr" for p in params]
    assert kinds == ["ptr", "int32", "ptr", "ptr", "int32", "int64", "int32", "int32", "int32", "int32", "int32", "ptr", "ptr", "ptr"]
    import ctypes as C
    want = {"int32": C.c_int32, "int64": C.c_int64}
    for kind, ctype in zip(kinds, rows[0][2]):
        assert ctype is want[kind] if kind in want else ctype not in want.values()
    assert "power_spectrum.hip" in entry.SOURCES and os.path.exists(os.path.join(entry.CSRC, "power_spectrum.hip"))
    assert int(re.search(r"#define DYF_SPECTRUM_MAX_DIM (\d+)", header).group(1)) == _lib.SPECTRUM_MAX_DIM == 1024
    assert int(re.search(r"#define DYF_SPECTRUM_MAX_MEMBERS (\d+)", header).group(1)) == _lib.SPECTRUM_MAX_MEMBERS == 256


@pytest.mark.parametrize("name", NAMES)
def test_integer_bin_rule_is_round_half_up_in_exact_rationals(name):
    c = refs.CASES[name]
    h, w, big = c.h, c.w, max(c.h, c.w)
    bins = refs.bin_map(h, w)
    for ky in range(h):
        for kx in range(w):
            kyf, kxf = min(ky, h - ky), min(kx, w - kx)
            q = 4 * big * big * (Fraction(kxf, w) ** 2 + Fraction(kyf, h) ** 2)  # (2 kappa)^2, exact
            s = math.isqrt(q.numerator // q.denominator)  # floor(2 kappa)
            assert Fraction(s) ** 2 <= q < Fraction(s + 1) ** 2
            assert bins[ky, kx] == (s + 1) // 2  # floor(kappa + 1/2) = floor((2 kappa + 1) / 2)
    assert bins[0, 0] == 0 and bins.max() >= c.n_bins - 1  # the longer axis reaches its Nyquist shell


@pytest.mark.parametrize("name", NAMES)
def test_reference_identities(name):
    c = refs.CASES[name]
    x, y = (a.astype(np.float64) for a in refs.inputs(name))
    planes, _ = refs.reference(name)
    win = np.outer(refs.hann(c.h), refs.hann(c.w)) if c.window == "hann" else 1.0
    d = refs.derived(planes, c.n)
    # members = spread + mean is the mean power spectrum of the single members
    bins = refs.bin_map(c.h, c.w)
    per_member = refs._shells(np.abs(np.fft.fft2(x * win)) ** 2 / float(c.h * c.w) ** 2, bins, c.n_bins).mean(axis=(1, 2))  # (segs, C, .)
    assert d["members"] == pytest.approx(per_member[..., :c.n_bins], rel=1e-12)
    # the coherence is that of the cross spectrum: |Xbar|^2 + |Y|^2 - |Xbar - Y|^2 = 2 Re(Xbar conj(Y))
    xbar = x.mean(axis=1)
    cross = 2.0 * np.real(np.fft.fft2(xbar * win) * np.conj(np.fft.fft2(y * win))) / float(c.h * c.w) ** 2
    cross = refs._shells(cross, bins, c.n_bins).mean(axis=1)[..., :c.n_bins]
    mean, target, error = planes[:, :, 1, :c.n_bins], planes[:, :, 2, :c.n_bins], planes[:, :, 3, :c.n_bins]
    scale = mean + target + error
    assert np.max(np.abs((mean + target - error) - cross) / scale) <= 1e-12
    assert d["coherence"] == pytest.approx(cross / (2.0 * np.sqrt(mean * target)), rel=1e-9, abs=1e-12)
    assert np.all(np.abs(d["coherence"]) <= 1.0 + 1e-12)
    # Parseval: the totals are the mean squares of the fields
    total = planes[..., c.n_bins]
    assert total[:, :, 2] == pytest.approx(((y * win) ** 2).mean(axis=(1, 3, 4)), rel=1e-12)
    assert total[:, :, 1] == pytest.approx(((xbar * win) ** 2).mean(axis=(1, 3, 4)), rel=1e-12)
    assert total[:, :, 0] == pytest.approx((((x - xbar[:, None]) * win) ** 2).mean(axis=(1, 2, 4, 5)), rel=1e-12)
    # white noise loses part of its power to the dropped corners; the shells never exceed the total
    assert np.all(planes[..., :c.n_bins].sum(-1) <= total * (1 + 1e-12))


@pytest.mark.parametrize("name", NAMES)
def test_emulation_is_inside_half_the_bound(name):
    ratio = refs.worst_ratio(refs.emulate(name), name)
    print(f"{name}: emulation error / bound = {ratio:.3e}")
    assert ratio <= 0.5


@pytest.mark.parametrize("mutant", refs.MUTANTS)
def test_every_mutant_is_far_outside_the_bound(mutant):
    cases = MUTANT_CASES[mutant]
    assert len(cases) >= 1 and set(cases) <= set(NAMES)
    for name in cases:
        ratio = refs.worst_ratio(refs.emulate(name, mutant), name)
        print(f"{mutant} at {name}: error / bound = {ratio:.3e}")
        assert ratio > 10.0, (mutant, name, ratio)


def test_nyquist_column_of_the_ns_field_is_all_corners():
    c = refs.CASES["221x42"]
    assert refs.bin_map(c.h, c.w)[:, c.w // 2].min() == c.n_bins
    got, (planes, bound) = refs.emulate("221x42", "nyquist_twice"), refs.reference("221x42")
    assert np.max(np.abs(got - planes)[..., :c.n_bins] / bound[..., :c.n_bins]) <= 0.5  # no shell moves
    assert refs.worst_ratio(got, "221x42") > 1.0  # the total does, and is outside the bound


def test_mutant_table_is_complete():
    assert set(MUTANT_CASES) == set(refs.MUTANTS) and len(refs.MUTANTS) == 10
