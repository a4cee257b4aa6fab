"""References of the ensemble products and the rank histogram (dyf_ensemble_products, dyf_rank_histogram).  Nothing here touches the
GPU; tests/test_ensemble_products_refs.py checks this module against itself, the GPU tests check the device against it.

  * float64 / exact references: numpy on the float64 copy of the members (np.mean, np.std, np.min, np.max, np.quantile "linear",
    (x > t).mean()), and the tie-split histogram written from its definition;
  * `emulate_products` / `emulate_histogram`: the kernel's STATED fp32 expressions in numpy (include/dyffusion_hip.h), with named
    mutants -- each one a plausible slip of an implementation;
  * the bounds, u = 2^-24 (none of them comes from what the device returns):
      mean      |err| <= (N + 2) u mean_n|x_n|                      recursive summation of N terms in any order, 1 / N and the product
      std       |err| <= (N + 4) u std_ref + (N + 2) u mean_n|x_n|  the same for the squares, the square root; the second term is the
                                                                     error of the mean entering every deviation (all that is left
                                                                     when the members are equal)
      quantile  |err| <= 8 u max(|x_(lo)|, |x_(hi)|)                roundings of the fraction, the difference, the product and the sum,
                                                                     |x_(hi) - x_(lo)| <= 2 max; frac == 0: equal as numbers
      min, max, exceedance, tie-free histograms: equal as numbers; histograms with ties: 1e-12 relative per bin.
"""
import numpy as np

U = 2.0 ** -24
HIST_TIE_REL = 1e-12
F32 = np.float32

PRODUCT_MUTANTS = ("lo_plus_one", "one_minus_frac", "nearest_rank", "no_tie_break", "ddof1", "mean_over_n_minus_1", "last_member_ignored",
                   "exceed_ge", "stride_is_n_points")
HISTOGRAM_MUTANTS = ("le_instead_of_lt", "ties_to_lowest_bin", "group_is_p_mod_groups", "stride_is_n_points")


def plane_names(mean=True, std=True, min=False, max=False, quantiles=(), exceed=()):
    names = [m for m, on in (("mean", mean), ("std", std), ("min", min), ("max", max)) if on]
    return names + [f"q{float(q):g}" for q in quantiles] + [f"gt{float(t):g}" for t in exceed]


def order_statistics(n, q):
    """numpy's "linear": (lo, hi, frac) with h = (n - 1) q in double, the fraction rounded to fp32."""
    h = float(n - 1) * float(q)
    lo = min(int(np.floor(h)), n - 1)
    return lo, min(lo + 1, n - 1), F32(h - lo)


def gather_members(buf, n_members, n_points, member_stride, start=0, mutant=None):
    """(n_members, n_points) out of a flat buffer: member n of the segment starts at start + n * member_stride."""
    stride = n_points if mutant == "stride_is_n_points" else member_stride
    buf = np.asarray(buf).reshape(-1)
    return np.stack([buf[start + n * stride: start + n * stride + n_points] for n in range(n_members)])


# ---------------------------------------------------------------------------------------------------------------- products
def product_reference(x, mean=True, std=True, min=False, max=False, quantiles=(), exceed=()):
    """x (N, P) fp32 -> {name: (P,)}: float64 from numpy on the float64 members; exceedances np.float32(count) / np.float32(N)."""
    x32 = np.asarray(x, dtype=F32)
    x64 = x32.astype(np.float64)
    n = x64.shape[0]
    out = {}
    with np.errstate(invalid="ignore"):
        if mean:
            out["mean"] = np.mean(x64, axis=0)
        if std:
            out["std"] = np.std(x64, axis=0)
        if min:
            out["min"] = np.min(x64, axis=0)
        if max:
            out["max"] = np.max(x64, axis=0)
        for q in quantiles:
            out[f"q{float(q):g}"] = np.quantile(x64, float(q), axis=0, method="linear")
        for t in exceed:
            out[f"gt{float(t):g}"] = (x32 > F32(t)).sum(axis=0).astype(F32) / F32(n)
    return out


def sorted_members(x):
    return np.sort(np.asarray(x, dtype=F32), axis=0)


def _ranks(x, mutant=None):
    """rank(i) = #{j : x_j < x_i} + #{j < i : x_j == x_i}, (N, P) ints: a permutation per point (NaN-free points)."""
    n = x.shape[0]
    rank = np.zeros(x.shape, dtype=np.int64)
    for j in range(n):
        rank += x[j][None] < x
        if mutant != "no_tie_break":
            rank[j + 1:] += x[j][None] == x[j + 1:]
    return rank


def emulate_products(x, mean=True, std=True, min=False, max=False, quantiles=(), exceed=(), mutant=None):
    """The kernel's stated fp32 expressions on x (N, P) fp32 -> {name: (P,) fp32}."""
    x = np.asarray(x, dtype=F32)
    n, p = x.shape
    bad = np.isnan(x).any(axis=0)
    nan = F32(np.nan)
    out = {}
    with np.errstate(invalid="ignore", over="ignore"):
        total = np.zeros(p, dtype=F32)
        for i in range(n):  # the sum in member order
            total = total + x[i]
        inv = F32(1.0) / F32(n - 1 if mutant == "mean_over_n_minus_1" and n > 1 else n)
        mu = total * inv
        if mean:
            out["mean"] = mu
        if std:
            m2 = np.zeros(p, dtype=F32)
            for i in range(n):
                d = x[i] - mu
                m2 = m2 + d * d
            inv_var = F32(1.0) / F32(n - 1) if mutant == "ddof1" and n > 1 else F32(1.0) / F32(n)
            out["std"] = np.sqrt(m2 * inv_var)
        ext = x[:-1] if mutant == "last_member_ignored" and n > 1 else x
        if min:
            out["min"] = np.where(bad, nan, np.fmin.reduce(ext, axis=0))
        if max:
            out["max"] = np.where(bad, nan, np.fmax.reduce(ext, axis=0))
        if len(quantiles):
            rank = _ranks(np.where(bad[None], F32(0.0), x), mutant)
            ordered = np.zeros((n, p), dtype=F32)  # a skipped rank (the mutant without the tie-break) leaves its slot at zero
            np.put_along_axis(ordered, rank, x, axis=0)
            for q in quantiles:
                lo, hi, frac = order_statistics(n, q)
                if mutant == "lo_plus_one":
                    lo, hi = np.minimum(lo + 1, n - 1), np.minimum(hi + 1, n - 1)
                if mutant == "one_minus_frac" and frac != 0:
                    frac = F32(1.0) - frac
                if mutant == "nearest_rank":
                    lo, frac = int(np.minimum(np.floor(float(n - 1) * float(q) + 0.5), n - 1)), F32(0.0)
                a, b = ordered[lo], ordered[hi]
                v = a if frac == 0 else a + F32(frac) * (b - a)  # numpy rounds the product and the sum separately
                out[f"q{float(q):g}"] = np.where(bad, nan, v).astype(F32)
        for t in exceed:
            hit = x >= F32(t) if mutant == "exceed_ge" else x > F32(t)
            out[f"gt{float(t):g}"] = hit.sum(axis=0).astype(F32) / F32(n)
    return out


def product_bounds(x, quantiles=()):
    """{name: (P,) float64}: the derived bound of every plane that has one (see the module docstring); the others are equalities."""
    x64 = np.asarray(x, dtype=F32).astype(np.float64)
    n = x64.shape[0]
    mean_abs = np.mean(np.abs(x64), axis=0)
    out = {"mean": (n + 2) * U * mean_abs, "std": (n + 4) * U * np.std(x64, axis=0) + (n + 2) * U * mean_abs}
    order = np.sort(x64, axis=0)
    for q in quantiles:
        lo, hi, frac = order_statistics(n, q)
        if frac != 0:
            out[f"q{float(q):g}"] = 8 * U * np.maximum(np.abs(order[lo]), np.abs(order[hi]))
    return out


def equal_as_numbers(a, b):
    """np.array_equal on the values: +0 and -0 are one number, NaN equals NaN."""
    return np.array_equal(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64), equal_nan=True)


def check_products(got, x, fraction=1.0, **spec):
    """Hold `got` ({name: (P,)}) to the float64 reference of x (N, P): the equalities, and `fraction` of each derived bound.
    Returns {name: the worst |err| / bound, or 0.0 for an equality}; AssertionError names the plane that misses."""
    ref, bounds = product_reference(x, **spec), product_bounds(x, spec.get("quantiles", ()))
    assert list(got) == list(ref) == plane_names(**spec), (list(got), list(ref))
    bad = np.isnan(np.asarray(x, dtype=F32)).any(axis=0)
    used = {}
    for name, r in ref.items():
        g = np.asarray(got[name])
        assert g.shape == r.shape, (name, g.shape, r.shape)
        if name.startswith("gt"):
            assert equal_as_numbers(g, r), name
            used[name] = 0.0
            continue
        assert np.all(np.isnan(g[bad])) and not np.any(np.isnan(g[~bad])), f"{name}: NaN exactly where a member is NaN"
        g, r = g[~bad].astype(np.float64), r[~bad]
        if name in bounds:
            err, bound = np.abs(g - r), fraction * bounds[name][~bad]
            assert np.all(err <= bound), (name, float(np.max(err - bound)), int(np.argmax(err - bound)))
            with np.errstate(invalid="ignore", divide="ignore"):
                ratio = np.where(bound > 0, err / bounds[name][~bad], 0.0)
            used[name] = float(ratio.max()) if ratio.size else 0.0
        else:
            assert equal_as_numbers(g, r), name
            used[name] = 0.0
    return used


# ---------------------------------------------------------------------------------------------------------------- histogram
def histogram_reference(x, y, group_shape=None, mutant=None):
    """x (N, P) fp32 members, y (P,) fp32 targets, the points row-major (outer, groups, inner) -> (groups, N + 1) float64.  From the
    definition: b = #{x_n < y}, e = #{x_n == y}, each of the bins b .. b + e receives 1 / (e + 1); a NaN anywhere drops the point."""
    x, y = np.asarray(x, dtype=F32), np.asarray(y, dtype=F32)
    n, p = x.shape
    outer, groups, inner = (1, 1, p) if group_shape is None else group_shape
    assert outer * groups * inner == p
    hist = np.zeros((groups, n + 1), dtype=np.float64)
    with np.errstate(invalid="ignore"):
        below = (x <= y[None]).sum(axis=0) if mutant == "le_instead_of_lt" else (x < y[None]).sum(axis=0)
        equal = np.zeros(p, dtype=np.int64) if mutant == "le_instead_of_lt" else (x == y[None]).sum(axis=0)
    ok = ~(np.isnan(y) | np.isnan(x).any(axis=0))
    index = np.arange(p)
    group = index % groups if mutant == "group_is_p_mod_groups" else (index // inner) % groups
    for pt in np.nonzero(ok)[0]:
        b, e = int(below[pt]), int(equal[pt])
        if mutant == "ties_to_lowest_bin":
            hist[group[pt], b] += 1.0
        else:
            hist[group[pt], b:b + e + 1] += 1.0 / (e + 1)
    return hist


def emulate_histogram(buf_x, buf_y, n_members, n_points, member_stride, start_x=0, start_y=0, group_shape=None, mutant=None):
    """The histogram of one segment read out of flat buffers the way the kernel addresses them."""
    x = gather_members(buf_x, n_members, n_points, member_stride, start_x, mutant)
    y = np.asarray(buf_y).reshape(-1)[start_y:start_y + n_points]
    return histogram_reference(x, y, group_shape, mutant if mutant != "stride_is_n_points" else None)


def check_histogram(got, ref, tie_free):
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape and got.dtype == np.float64, (got.shape, ref.shape, got.dtype)
    if tie_free:
        assert np.array_equal(got, ref), "tie-free bins are integers and equal the reference"
    else:
        assert np.all(np.abs(got - ref) <= HIST_TIE_REL * np.abs(ref)), float(np.max(np.abs(got - ref)))


def frequencies(hist):
    f = hist / hist.sum(axis=-1, keepdims=True)
    return f, np.abs(f - 1.0 / hist.shape[-1]).sum(axis=-1)


# ---------------------------------------------------------------------------------------------------------------- inputs
THRESHOLDS = (0.25, -0.5, 1.0)  # 0.25 and 1.0 are member values of the rounded inputs
QUANTILES = (0.0, 0.05, 1.0 / 3.0, 0.5, 0.95, 1.0)
FULL_SPEC = dict(mean=True, std=True, min=True, max=True, quantiles=QUANTILES, exceed=THRESHOLDS)


def members(n, points, seed=0, rounded=False, offset=0.1, scale=0.6):
    """(truth (points,), preds (n, points)) fp32.  `rounded`: members and truth are multiples of 1/4 -- many ties, among the members
    and with the truth -- and the LAST eighth of the points (at least one) is a boundary block: every member equals the truth."""
    rng = np.random.default_rng(1000 * n + points + 7919 * seed)
    truth = rng.normal(size=points)
    preds = 0.7 * truth[None] + scale * rng.normal(size=(n, points)) + offset
    if rounded:
        truth, preds = np.round(truth * 4) / 4, np.round(preds * 4) / 4
        k = max(1, points // 8)
        preds[:, points - k:] = truth[None, points - k:]
    return truth.astype(F32), preds.astype(F32)
