"""The reference, the error bound, an fp32 emulation and the mutants for dyf_power_spectrum (no GPU).

Reference: float64, np.fft.fft2 on the FULL spectrum (so independent of the kernel's half-spectrum weights), the exact (unrounded)
float64 ensemble mean, the float64 Hann window, the shell of every coefficient from the exact integer rule of the header.

Bound: with u = 2^-24 a transformed field z has per-coefficient error at most delta(z) = 2 (H + W + 8) u ||z||_1 (the Higham gamma bound
of two chained fp32 sums with rounded twiddles, with a factor for the complex parts); for the anomalies and the error u (||xbar||_1 +
||z||_1) is added for the rounded mean and the subtraction.  A bin's bound is sum_{k in bin} (2 |Z_k| delta + delta^2) / (H W)^2,
averaged like the bin itself.

Emulation: the kernel's scheme in numpy fp32 (rounded mean, fp32 anomalies, rounded tables, row DFT then column DFT as running fp32
sums over the half spectrum, float64 from |Z|^2 on), with switches for the ten mutants of tests/test_power_spectrum_refs.py."""
import functools
from dataclasses import dataclass

import numpy as np

U = 2.0 ** -24
PLANES = ("spread", "mean", "target", "error")


@dataclass(frozen=True)
class Case:
    name: str
    h: int
    w: int
    n: int
    b: int
    c: int
    segs: int = 1
    form: str = "tensor"  # "tensor": one (N, B, C, H, W) tensor; "list": a list of `segs` such tensors
    window: str = "none"
    strided: bool = False  # the members are a view of a larger stack: member stride 2 * B * C * H * W

    @property
    def n_bins(self):
        return max(self.h, self.w) // 2 + 1


# the smallest shapes at which the kernel can go wrong; N in {1, 2, 5}, B in {1, 3}, C in {1, 2}, both forms, both windows
CASES = {c.name: c for c in (
    Case("2x2", 2, 2, n=2, b=1, c=1),                                       # smallest transform
    Case("5x3", 5, 3, n=5, b=3, c=2, segs=2, form="list", window="hann"),   # odd W, H < 16, H mod 4 != 0
    Case("13x7", 13, 7, n=1, b=3, c=1),                                     # small odd shape, one member
    Case("16x30", 16, 30, n=2, b=1, c=2, window="hann"),                    # even W, exact tile
    Case("33x34", 33, 34, n=5, b=1, c=1, segs=2, form="list"),              # ragged ky tile and ragged K, 18 columns: 2 kx tiles
    Case("33x34_hann", 33, 34, n=2, b=3, c=1, window="hann"),
    Case("61x42", 61, 42, n=2, b=3, c=1, window="hann", strided=True),      # L = H > W
    Case("70x70", 70, 70, n=5, b=1, c=2),                                   # 3 kx tiles
    Case("221x42", 221, 42, n=3, b=1, c=1),                                 # the NS field itself, 37 KB
)}


@functools.lru_cache(maxsize=None)
def inputs(name):
    """(preds (segs, N, B, C, H, W), targets (segs, B, C, H, W)) fp32, read-only: white noise plus one smooth mode."""
    c = CASES[name]
    rng = np.random.default_rng(sum(name.encode()) * 7919 + c.h * 31 + c.w)
    hh, ww = np.meshgrid(np.arange(c.h), np.arange(c.w), indexing="ij")
    mode = np.cos(2 * np.pi * (2 * hh / c.h + ww / c.w))
    y = rng.standard_normal((c.segs, c.b, c.c, c.h, c.w)) + 1.5 * mode + 0.25
    x = 0.8 * y[:, None] + 0.5 * rng.standard_normal((c.segs, c.n, c.b, c.c, c.h, c.w)) + 0.3 * mode
    x, y = x.astype(np.float32), y.astype(np.float32)
    x.setflags(write=False), y.setflags(write=False)
    return x, y


def hann(n):
    return 0.5 * (1.0 - np.cos(2.0 * np.pi * np.arange(n) / n))


def bin_map(h, w, mutant=None):
    """The shell of every coefficient of the full (H, W) spectrum by the exact integer rule: bin = k <=> (2k - 1)^2 H^2 W^2 <=
    4 L^2 (kx'^2 H^2 + ky'^2 W^2) < (2k + 1)^2 H^2 W^2 (may be >= n_bins: a corner).  Mutants: "bin_trunc", "isotropic", "ky_unfolded"."""
    big = max(h, w)
    ky, kx = np.meshgrid(np.arange(h, dtype=np.int64), np.arange(w, dtype=np.int64), indexing="ij")
    kyf = ky if mutant == "ky_unfolded" else np.minimum(ky, h - ky)
    kxf = np.minimum(kx, w - kx)
    if mutant == "isotropic":  # kappa^2 = kx'^2 + ky'^2: as if H = W = L = 1 in the rule
        num, den = 4 * (kxf * kxf + kyf * kyf), np.int64(1)
    else:
        num, den = 4 * big * big * (kxf * kxf * h * h + kyf * kyf * w * w), np.int64(h * h * w * w)
    if mutant == "bin_trunc":  # floor(kappa): k^2 den <= num / 4 < (k + 1)^2 den
        k = np.floor(np.sqrt(num / (4.0 * den))).astype(np.int64)
        k += (4 * (k + 1) ** 2 * den <= num)
        k -= (4 * k ** 2 * den > num)
        return k
    k = np.floor(np.sqrt(num / (4.0 * den)) + 0.5).astype(np.int64)
    k += ((2 * k + 1) ** 2 * den <= num)
    k -= ((k > 0) & ((2 * k - 1) ** 2 * den > num))
    assert np.all((2 * k + 1) ** 2 * den > num) and np.all((k == 0) | ((2 * k - 1) ** 2 * den <= num))
    return k


def _shells(power, bins, n_bins):
    """(..., H, W) -> (..., n_bins + 1): the shells 0 .. n_bins - 1 and the total over ALL coefficients."""
    lead = power.shape[:-2]
    flat = power.reshape(-1, power.shape[-2] * power.shape[-1])
    b = bins.reshape(-1)
    keep = b < n_bins
    out = np.zeros((flat.shape[0], n_bins + 1))
    for i in range(flat.shape[0]):
        out[i, :n_bins] = np.bincount(b[keep], weights=flat[i, keep], minlength=n_bins)
        out[i, n_bins] = flat[i].sum()
    return out.reshape(*lead, n_bins + 1)


@functools.lru_cache(maxsize=None)
def reference(name):
    """(planes, bound), each (segs, C, 4, n_bins + 1) float64, read-only."""
    c = CASES[name]
    x32, y32 = inputs(name)
    x, y = x32.astype(np.float64), y32.astype(np.float64)
    win = np.outer(hann(c.h), hann(c.w)) if c.window == "hann" else np.ones((c.h, c.w))
    bins = bin_map(c.h, c.w)
    hw2 = float(c.h * c.w) ** 2
    xbar = x.mean(axis=1)  # (segs, B, C, H, W)
    fields = {"spread": (x - xbar[:, None]) * win, "mean": xbar * win, "target": y * win, "error": (xbar - y) * win}
    l1 = lambda z: np.abs(z).sum(axis=(-2, -1), keepdims=True)  # noqa: E731
    gamma = 2.0 * (c.h + c.w + 8) * U
    planes, bound = [], []
    for key in PLANES:
        z = fields[key]
        delta = gamma * l1(z)
        if key in ("spread", "error"):
            delta = delta + U * (l1(fields["mean"])[:, None] if key == "spread" else l1(fields["mean"])) + U * l1(z)
        spec = np.abs(np.fft.fft2(z))
        p = _shells(spec ** 2 / hw2, bins, c.n_bins)
        e = _shells((2.0 * spec * delta + delta ** 2) / hw2, bins, c.n_bins)
        if key == "spread":
            p, e = p.mean(axis=1), e.mean(axis=1)  # over the members
        planes.append(p.mean(axis=1))  # over the batch: (segs, C, n_bins + 1)
        bound.append(e.mean(axis=1))
    planes, bound = np.stack(planes, axis=2), np.stack(bound, axis=2)
    planes.setflags(write=False), bound.setflags(write=False)
    return planes, bound


MUTANTS = ("nyquist_twice", "dc_twice", "bin_trunc", "isotropic", "ky_unfolded", "norm_hw", "spread_n_minus_1", "window_one_axis",
           "last_row_missing", "anomaly_vs_target")


def emulate(name, mutant=None):
    """The kernel's scheme in numpy fp32 -> (segs, C, 4, n_bins + 1) float64; `mutant` one of MUTANTS."""
    assert mutant is None or mutant in MUTANTS
    c = CASES[name]
    f32 = np.float32
    x, y = inputs(name)
    h, w, wh = c.h, c.w, c.w // 2 + 1
    xbar = (x.astype(np.float64).sum(axis=1) / c.n).astype(f32)  # rounded once
    anomalies = x - (y[:, None] if mutant == "anomaly_vs_target" else xbar[:, None])
    fields = [anomalies[:, m] for m in range(c.n)] + [xbar, y, xbar - y]  # each (segs, B, C, H, W) fp32
    if c.window == "hann":
        wh_tab, ww_tab = hann(h).astype(f32), hann(w).astype(f32)
        win = wh_tab[:, None] * (np.ones(w, f32) if mutant == "window_one_axis" else ww_tab)[None, :]
        fields = [z * win for z in fields]
    cw, sw = np.cos(2 * np.pi * np.arange(w) / w).astype(f32), np.sin(2 * np.pi * np.arange(w) / w).astype(f32)
    ch, sh = np.cos(2 * np.pi * np.arange(h) / h).astype(f32), np.sin(2 * np.pi * np.arange(h) / h).astype(f32)
    kx, ky = np.arange(wh), np.arange(h)
    weight = np.full(wh, 2.0)
    weight[0] = 2.0 if mutant == "dc_twice" else 1.0
    if w % 2 == 0:
        weight[w // 2] = 2.0 if mutant == "nyquist_twice" else 1.0
    bins = bin_map(h, w, mutant if mutant in ("bin_trunc", "isotropic", "ky_unfolded") else None)[:, :wh]
    rows = h - 1 if mutant == "last_row_missing" else h
    power = []
    for z in fields:
        tr, ti = np.zeros(z.shape[:-1] + (wh,), f32), np.zeros(z.shape[:-1] + (wh,), f32)
        for j in range(w):  # the row DFT, w order
            idx = (kx * j) % w
            tr = tr + z[..., j, None] * cw[idx]
            ti = ti - z[..., j, None] * sw[idx]
        r1, r2, i1, i2 = (np.zeros(z.shape[:-2] + (h, wh), f32) for _ in range(4))
        for r in range(rows):  # the column DFT, h order, four chains
            idx = (ky * r) % h
            co, si = ch[idx][:, None], sh[idx][:, None]
            r1 = r1 + co * tr[..., r, None, :]
            r2 = r2 + si * ti[..., r, None, :]
            i1 = i1 + co * ti[..., r, None, :]
            i2 = i2 - si * tr[..., r, None, :]
        zr, zi = (r1 + r2).astype(np.float64), (i1 + i2).astype(np.float64)
        assert r1.dtype == f32 and tr.dtype == f32
        power.append(weight * (zr * zr + zi * zi))
    norm = float(h * w) if mutant == "norm_hw" else float(h * w) ** 2
    members = c.n - 1 if mutant == "spread_n_minus_1" else c.n
    spread = sum(power[:c.n]) / members if members else np.full_like(power[0], np.inf)
    planes = [_shells(p / norm, bins, c.n_bins).mean(axis=1) for p in (spread, power[c.n], power[c.n + 1], power[c.n + 2])]
    return np.stack(planes, axis=2)


def worst_ratio(got, name):
    """max |got - reference| / bound over the planes and the total of case `name` (got: (segs, C, 4, n_bins + 1)); a bound of exactly 0
    (an empty shell) demands exactly 0."""
    planes, bound = reference(name)
    err = np.abs(np.asarray(got, dtype=np.float64) - planes)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err == 0, 0.0, np.inf))
    return float(np.nanmax(np.where(np.isnan(err), np.inf, ratio)))


def derived(planes, n):
    """members, spread_fair, spectral_ssr, coherence, lsd, lsd_ens_mean from (..., 4, n_bins + 1) planes, in float64 numpy."""
    nb = planes.shape[-1] - 1
    spread, mean, target, error = (planes[..., i, :nb] for i in range(4))
    members = spread + mean
    with np.errstate(divide="ignore", invalid="ignore"):
        fair = spread * (n / (n - 1.0)) if n > 1 else np.full_like(spread, np.nan)
        out = {"members": members, "spread_fair": fair, "spectral_ssr": np.sqrt((n + 1.0) / n * fair / error),
               "coherence": (mean + target - error) / (2.0 * np.sqrt(mean * target))}
        use = target[..., 1:] > 0
        for key, p in (("lsd", members), ("lsd_ens_mean", mean)):
            db = 10.0 * np.log10(p[..., 1:] / np.where(use, target[..., 1:], 1.0))
            out[key] = np.sqrt(np.where(use, db * db, 0.0).sum(-1) / use.sum(-1))
    return out
