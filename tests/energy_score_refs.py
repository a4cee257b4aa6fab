"""References of the energy score and the member-distance matrix (dyf_energy_score).  Nothing here touches the GPU;
tests/test_energy_score_refs.py checks this module against itself, torch.cdist and the oracle's CRPS, the GPU tests check the device
against it.

  * `reference_segment`: float64 numpy on the float64 copy of the fp32 members, written from the definition with explicit loops over
    the vectors, the members and the pairs (d_i = ||x_i - y||, D_ij = ||x_i - x_j||, then the means) -- not the tiled expression of
    the kernel;
  * `emulate_segment`: the kernel's STATED arithmetic in numpy (include/dyffusion_hip.h): fp32 differences, fp32 sums of squares
    over tiles of K points (without FMA), float64 joins, float64 sqrt once per vector -- with named mutants, each a slip this
    kernel could make;
  * the bound, u = 2^-24, K = DYF_ENERGY_TILE_POINTS (nothing of it comes from what the device returns): a sum of K non-negative
    squares of rounded differences, accumulated in fp32, has relative error <= (K + 2) u (two roundings per term, K - 1 of the
    sum); the square root halves it, and the half is given back as margin.  So every d and D, and every mean of them, is within
    (K + 2) u of itself; dist_target and dist_pair likewise, es within (K + 2) u (dist_target + (N - 1) / (2 N) dist_pair), es_fair
    within (K + 2) u (dist_target + dist_pair / 2).  An exact zero stays an exact zero, a NaN stays a NaN.
"""
import functools

import numpy as np

U = 2.0 ** -24
K = 64  # DYF_ENERGY_TILE_POINTS
F32 = np.float32
ROWS = ("es", "es_fair", "dist_target", "dist_pair")

MUTANTS = ("fair_divisor_in_es", "half_missing", "diagonal_counted", "sqrt_after_outer_mean", "sqrt_per_tile", "tail_points_dropped",
           "l1_instead_of_l2", "gram_raw", "gram_centred", "last_member_ignored", "pad_members_counted", "stride_is_n_points",
           "group_is_p_mod_groups", "target_of_segment_0")
# the case on which each mutant has to miss the bound by a factor of ten
MUTANT_CASE = {"fair_divisor_in_es": "n5", "half_missing": "n5", "diagonal_counted": "n5", "sqrt_after_outer_mean": "n3",
               "sqrt_per_tile": "n5", "tail_points_dropped": "n5", "l1_instead_of_l2": "n5", "gram_raw": "far", "gram_centred": "close",
               "last_member_ignored": "n5", "pad_members_counted": "n5", "stride_is_n_points": "n3", "group_is_p_mod_groups": "n5",
               "target_of_segment_0": "n3"}


def gather_members(buf, n_members, n_points, member_stride, start=0, mutant=None):
    """(n_members, n_points) out of a flat buffer: member n of the segment starts at start + n * member_stride."""
    stride = n_points if mutant == "stride_is_n_points" else member_stride
    buf = np.asarray(buf).reshape(-1)
    return np.stack([buf[start + n * stride: start + n * stride + n_points] for n in range(n_members)])


def _view(a, group_shape, mutant=None):
    """(..., P) -> (..., outer, groups, inner): point p of a segment lies in vector (p // (groups * inner), (p // inner) % groups)."""
    o, g, i = group_shape
    if mutant == "group_is_p_mod_groups":
        return np.swapaxes(a.reshape(*a.shape[:-1], o, i, g), -1, -2)
    return a.reshape(*a.shape[:-1], o, g, i)


def scores(member, pair, n, mutant=None):
    """(es, es_fair, dist_target, dist_pair) of one (segment, group) from mean_o d_i (N,) and mean_o D_ij (N, N)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        dist_target = np.sum(member) / n
        dist_pair = np.sum(pair) / np.float64(n * n if mutant == "diagonal_counted" else n * (n - 1))
        weight = 0.5 if mutant == "fair_divisor_in_es" else (n - 1) / n if mutant == "half_missing" else (n - 1) / (2.0 * n)
        es = dist_target - weight * dist_pair if n > 1 else dist_target
        return np.array([es, dist_target - 0.5 * dist_pair, dist_target, dist_pair])


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def reference_segment(x32, y32, group_shape):
    """x32 (N, P) fp32, y32 (P,) fp32 -> (planes (4, G), member (G, N), pair (G, N, N)) in float64, from the definition."""
    x = _view(np.asarray(x32, dtype=F32).astype(np.float64), group_shape)
    y = _view(np.asarray(y32, dtype=F32).astype(np.float64), group_shape)
    n, n_outer, n_groups = x.shape[0], group_shape[0], group_shape[1]
    planes, member, pair = np.zeros((4, n_groups)), np.zeros((n_groups, n)), np.zeros((n_groups, n, n))
    with np.errstate(invalid="ignore"):
        for g in range(n_groups):
            for o in range(n_outer):
                for i in range(n):
                    xi = x[i, o, g]
                    member[g, i] += np.sqrt(np.sum(np.square(xi - y[o, g])))
                    for j in range(i + 1, n):
                        dij = np.sqrt(np.sum(np.square(xi - x[j, o, g])))
                        pair[g, i, j] += dij
                        pair[g, j, i] += dij
            member[g] /= n_outer
            pair[g] /= n_outer
            planes[:, g] = scores(member[g], pair[g], n)
    return planes, member, pair


# ---------------------------------------------------------------------------------------------------------------- fp32 emulation
def _tile_sums(terms):
    """(..., I) fp32 terms -> list of (...) fp32 sums of consecutive tiles of K terms, each accumulated in term order."""
    out = []
    for t0 in range(0, terms.shape[-1], K):
        acc = np.zeros(terms.shape[:-1], dtype=F32)
        for p in range(t0, min(t0 + K, terms.shape[-1])):
            acc = (acc + terms[..., p]).astype(F32)
        out.append(acc)
    return out


def _distance(a, b, mutant):
    """Rows of a (..., I) against rows of b (broadcast), fp32 in -> float64 (sum of squares, distance): the stated arithmetic."""
    if mutant in ("gram_raw", "gram_centred"):
        with np.errstate(invalid="ignore"):
            ss = (np.sum(a * a, axis=-1, dtype=F32) + np.sum(b * b, axis=-1, dtype=F32)).astype(F32) - F32(2) * np.sum(a * b, axis=-1, dtype=F32)
            ss = ss.astype(F32).astype(np.float64)
            return ss, np.sqrt(ss)  # NaN where the cancellation went below zero
    diff = (a - b).astype(F32)
    if mutant == "l1_instead_of_l2":
        total = sum(t.astype(np.float64) for t in _tile_sums(np.abs(diff)))
        return total, total
    tiles = _tile_sums((diff * diff).astype(F32))
    ss = np.zeros(tiles[0].shape)
    for t in tiles:
        ss = ss + t.astype(np.float64)
    with np.errstate(invalid="ignore"):
        if mutant == "sqrt_per_tile":
            return ss, sum(np.sqrt(t.astype(np.float64)) for t in tiles)
        return ss, np.sqrt(ss)


def emulate_segment(x32, y32, group_shape, mutant=None):
    """As reference_segment, in the kernel's stated arithmetic (or with one named slip)."""
    x32, y32 = np.asarray(x32, dtype=F32), np.asarray(y32, dtype=F32)
    if mutant == "last_member_ignored" and x32.shape[0] > 1:
        x32 = x32[:-1]
    if mutant == "pad_members_counted":
        x32 = np.concatenate([x32, np.zeros((-x32.shape[0] % 64, x32.shape[1]), dtype=F32)])
    x, y = _view(x32, group_shape, mutant), _view(y32, group_shape, mutant)
    n, n_outer, n_groups, n_inner = x.shape[0], group_shape[0], group_shape[1], group_shape[2]
    if mutant == "tail_points_dropped" and n_inner > K:
        x, y = x[..., : n_inner // K * K], y[..., : n_inner // K * K]
    planes, member, pair = np.zeros((4, n_groups)), np.zeros((n_groups, n)), np.zeros((n_groups, n, n))
    for g in range(n_groups):
        m_ss, m_d, p_ss, p_d = np.zeros(n), np.zeros(n), np.zeros((n, n)), np.zeros((n, n))
        for o in range(n_outer):
            a, t = x[:, o, g], y[o, g][None]
            if mutant == "gram_centred":
                a, t = (a - t).astype(F32), np.zeros_like(t)
            ss, d = _distance(a, t, mutant)
            m_ss, m_d = m_ss + ss, m_d + d
            ss, d = _distance(a[:, None], a[None], mutant)
            np.fill_diagonal(d, 0.0), np.fill_diagonal(ss, 0.0)  # D_ii is 0 by definition, never computed (nor NaN - NaN)
            p_ss, p_d = p_ss + ss, p_d + d
        with np.errstate(invalid="ignore"):
            member[g] = np.sqrt(m_ss / n_outer) if mutant == "sqrt_after_outer_mean" else m_d / n_outer
            pair[g] = np.sqrt(p_ss / n_outer) if mutant == "sqrt_after_outer_mean" else p_d / n_outer
        planes[:, g] = scores(member[g], pair[g], n, mutant)
    if mutant in ("last_member_ignored", "pad_members_counted"):  # their matrices have another shape: only the planes are compared
        return planes, None, None
    return planes, member, pair


# ---------------------------------------------------------------------------------------------------------------- cases
class Case:
    """One call: `buffers[s]` holds segment s's members at start `starts[s]` with `stride`; targets (S, P)."""

    def __init__(self, name, n, segs, group_shape, form, preds, targets):
        self.name, self.n, self.segs, self.group_shape, self.form = name, n, segs, tuple(group_shape), form
        self.points = int(np.prod(group_shape))
        self.preds, self.targets = preds, targets  # (N, S, P) fp32, (S, P) fp32
        if form == "tensor":  # one (N, S, ...) tensor read in place: member stride S * P
            self.stride, self.starts, self.buffers = segs * self.points, [s * self.points for s in range(segs)], [preds] * segs
        else:  # a list of S contiguous (N, ...) tensors
            self.stride, self.starts = self.points, [0] * segs
            self.buffers = [np.ascontiguousarray(preds[:, s]) for s in range(segs)]

    def segment(self, s, mutant=None):
        x = gather_members(self.buffers[s], self.n, self.points, self.stride, self.starts[s], mutant)
        return x, self.targets[0 if mutant == "target_of_segment_0" else s]


SHAPES = {  # name: (N, segments, (outer, groups, inner), form): every N and n_inner of the limits, both outer and groups, both forms
    "n1": (1, 2, (3, 3, 3), "tensor"),
    "n2": (2, 1, (1, 1, K - 1), "list"),
    "n3": (3, 2, (3, 1, K), "tensor"),
    "n5": (5, 2, (1, 3, K + 1), "list"),
    "n63": (63, 1, (3, 3, 1), "tensor"),
    "n63_points": (63, 2, (9, 1, 1), "tensor"),
    "n64": (64, 2, (1, 3, 2 * K + 5), "tensor"),
    "n65": (65, 1, (3, 1, 2 * K + 5), "list"),
    "n130": (130, 2, (3, 3, 3), "tensor"),
    "n256": (256, 1, (3, 3, K + 1), "list"),
    "far": (5, 2, (1, 3, K + 1), "tensor"),     # members at 1000 + 0.01 randn
    "close": (3, 1, (3, 1, K), "tensor"),       # member 2 is member 1 but for 1e-3 at one point of every vector
    "twins": (5, 2, (3, 3, 3), "list"),         # members 1 and 3 are identical
    "nan": (5, 2, (3, 3, K + 1), "tensor"),     # a NaN in member 1, segment 0, vector (outer 1, group 2)
}
NAN_AT = dict(member=1, segment=0, outer=1, group=2)


@functools.lru_cache(maxsize=None)
def case(name):
    n, segs, gs, form = SHAPES[name]
    points = int(np.prod(gs))
    rng = np.random.default_rng(sorted(SHAPES).index(name) + 17)
    truth = rng.standard_normal((segs, points))
    scale = (0.6 + 0.1 * np.arange(segs))[None, :, None]
    preds = 0.7 * truth[None] + scale * rng.standard_normal((n, segs, points)) + 0.1
    if name == "far":
        truth = 1000.0 + 0.01 * truth
        preds = 1000.0 + 0.01 * preds
    preds, truth = preds.astype(F32), truth.astype(F32)
    if name == "close":
        preds[2] = preds[1]
        v = _view(preds[2], gs)  # (S, outer, groups, inner): a view
        v[..., 5] += F32(1e-3)
    if name == "twins":
        preds[3] = preds[1]
    if name == "nan":
        _view(preds[NAN_AT["member"]], gs)[NAN_AT["segment"], NAN_AT["outer"], NAN_AT["group"], 7] = np.nan
    preds.setflags(write=False), truth.setflags(write=False)
    return Case(name, n, segs, gs, form, preds, truth)


def evaluate(c, fn, mutant=None):
    """{"planes": (4, S, G), "member": (S, G, N), "pair": (S, G, N, N)} of a case under fn = reference_segment or emulate_segment."""
    outs = []
    for s in range(c.segs):
        x, y = c.segment(s, mutant)
        outs.append(fn(x, y, c.group_shape) if mutant is None else fn(x, y, c.group_shape, mutant))
    res = {"planes": np.stack([o[0] for o in outs], axis=1)}
    if outs[0][1] is not None:
        res["member"], res["pair"] = np.stack([o[1] for o in outs]), np.stack([o[2] for o in outs])
    return res


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case, computed once and shared (read-only)."""
    res = evaluate(case(name), reference_segment)
    for v in res.values():
        v.setflags(write=False)
    return res


def bounds(ref, n):
    """The derived bound of every entry of `ref` (NaN where the reference is NaN)."""
    e = (K + 2) * U
    dt, dp = ref["planes"][2], ref["planes"][3]
    with np.errstate(invalid="ignore"):
        w = dp if n > 1 else np.zeros_like(dt)
        planes = np.stack([e * (dt + (n - 1) / (2.0 * n) * w), e * (dt + 0.5 * dp), e * dt, e * dp])
    return {"planes": planes, "member": e * ref["member"], "pair": e * ref["pair"]}


def worst_ratio(got, ref, n, keys=("planes", "member", "pair")):
    """max |got - ref| / bound over the entries of `keys`; inf where a NaN is not where the reference has one, or where an exact zero
    of the reference is not an exact zero."""
    bnd = bounds(ref, n)
    worst = 0.0
    for k in keys:
        g, r, b = np.asarray(got[k], dtype=np.float64), ref[k], bnd[k]
        if g.shape != r.shape or np.any(np.isnan(g) != np.isnan(r)):
            return float("inf")
        ok = ~np.isnan(r)
        err = np.abs(g[ok] - r[ok])
        zero = b[ok] == 0.0
        if np.any(err[zero] != 0.0):
            return float("inf")
        if np.any(~zero):
            worst = max(worst, float(np.max(err[~zero] / b[ok][~zero])))
    return worst
