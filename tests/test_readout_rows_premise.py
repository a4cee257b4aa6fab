"""What the row-staged body of the readout (csrc/kernels.hip, readout_dma_rows_kernel) rests on, checked without a GPU.

The body streams the decoder rows of a band of output rows in DESCENDING order and blends, per staged row, the kernel rows kh
that read it, kh ascending.  That is the gather body's tap order kh = 0..3 exactly when, for every output row,

  * the input rows of kh = 0..3 never increase with kh, and span at most three rows;
  * taps outside the image are a prefix of kh (rows >= ih: blended while the sum is still +0) or a suffix (rows < 0: one
    fmaf(0, 0, out) after the stream);

and a band's rows are one contiguous range to stream when the largest input row never decreases with the output row.

Two statements of the stencil are held to this: the reference stencil of tests/sample_op_refs.py (taps with a weight), and a host
mirror of readout_tables_kernel's own arithmetic (every tap the tables give a row, also those of weight 0, which the kernels blend
like any other: they carry inf / NaN).  Where the reference gives a tap a weight, the mirror names the same row.
"""
import numpy as np
import pytest

from tests import sample_op_refs as S

# ((ih, iw), (oh, ow)): the NS decoder plane -> native grid, and the geometries of tests/test_gpu_readout_rows.py
GEOMS = [((256, 256), (221, 42)), ((6, 16), (5, 3)), ((32, 32), (27, 5)), ((40, 24), (33, 9)), ((8, 8), (48, 48)), ((1, 1), (3, 3)),
         ((6, 40), (5, 70)), ((20, 12), (21, 7)), ((2, 128), (3, 20)), ((2, 129), (3, 20)), ((8, 8), (192, 192)), ((2, 3), (4, 6)),
         ((6, 8), (5, 7)), ((2, 2), (9, 11))]
AXES = sorted({(g[0][0], g[1][0]) for g in GEOMS} | {(g[0][1], g[1][1]) for g in GEOMS})


def table_rows(n_in, n_out, nearest):
    """readout_tables_kernel on the host: (input index of tap k per output (n_out, 4), possibly outside 0..n_in-1; weight (n_out, 4))
    with bilinear_coord (csrc/common.h) in float32."""
    t = 2 * n_in
    scale = np.float32(t) / np.float32(n_out)
    dst = np.arange(n_out)
    if nearest:
        u0 = np.minimum(np.floor(dst.astype(np.float32) * scale).astype(np.int64), t - 1)
        u1, lam = u0.copy(), np.zeros(n_out, np.float32)
    else:
        src = np.maximum((dst.astype(np.float32) + np.float32(0.5)) * scale - np.float32(0.5), np.float32(0))
        u0 = np.minimum(src.astype(np.int64), t - 1)
        u1 = np.where(u0 + 1 < t, u0 + 1, t - 1)
        lam = (src - u0.astype(np.float32)).astype(np.float32)
    idx, wgt = np.zeros((n_out, 4), np.int64), np.zeros((n_out, 4), np.float32)
    for k in range(4):
        par = (k + 1) & 1
        wgt[:, k] = np.where((u0 & 1) == par, np.float32(1) - lam, np.float32(0)) + np.where((u1 & 1) == par, lam, np.float32(0))
        u = np.where((u1 & 1) == par, u1, u0)
        idx[:, k] = ((u + 1) >> 1) - (k >> 1)
    return idx, wgt


def check_order(idx, n_in, tag):
    """idx (n_out, 4) objects, None where a tap has no row: the streaming order's premises."""
    last_top = -1
    for o, rows in enumerate(idx.tolist()):
        have = [r for r in rows if r is not None]
        assert all(a >= b for a, b in zip(have, have[1:])), (tag, o, rows)          # never increasing with kh
        assert not have or have[0] - have[-1] <= 2, (tag, o, rows)                 # at most three rows
        inside = [0 <= r < n_in for r in have]
        first, last = (inside.index(True), len(inside) - 1 - inside[::-1].index(True)) if any(inside) else (0, -1)
        assert all(inside[first:last + 1]), (tag, o, rows)                          # outside taps: a prefix and a suffix only
        assert all(r >= n_in for r in have[:first]) and all(r < 0 for r in have[last + 1:]), (tag, o, rows)
        top = max((r for r in have if 0 <= r < n_in), default=last_top)
        assert top >= last_top, (tag, o, rows)                                      # the largest row never decreases with o
        last_top = top


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_kernel_tables_name_rows_in_streaming_order(axis, nearest):
    n_in, n_out = axis
    idx, wgt = table_rows(n_in, n_out, nearest)
    check_order(idx.astype(object), n_in, ("tables", axis, nearest))
    # the mirror is the reference stencil wherever the reference gives a tap a weight
    ridx, rwgt = S.readout_taps(n_in, n_out, nearest)
    ridx, rwgt = ridx.numpy(), rwgt.numpy()
    hit = rwgt != 0
    assert np.array_equal(idx[hit], ridx[hit]), (axis, nearest)
    atol = 4 * 2 * n_in * 2.0 ** -24  # the fp32 source coordinate (< 2 n_in): scale, product, sum and lam rounded once each
    assert np.allclose(wgt[hit], rwgt[hit], rtol=0, atol=atol) and np.all(np.abs(wgt[~hit]) <= atol), (axis, nearest)


@pytest.mark.parametrize("nearest", [False, True])
@pytest.mark.parametrize("axis", AXES, ids=lambda a: f"{a[0]}to{a[1]}")
def test_reference_stencil_rows_are_in_streaming_order(axis, nearest):
    n_in, n_out = axis
    ridx, rwgt = S.readout_taps(n_in, n_out, nearest)
    rows = np.empty(ridx.shape, dtype=object)
    for o in range(n_out):
        for k in range(4):
            rows[o, k] = int(ridx[o, k]) if float(rwgt[o, k]) != 0 else None  # (a tap without a weight has no row in the reference)
    check_order(rows, n_in, ("reference", axis, nearest))


def test_ns_compact_width_fits_the_rows_plan():
    """The NS decoder's compact width (the stored columns of 256 -> 42) and the LDS plan of the rows body: z of 16-pixel groups
    G = ceil(iw_store / 16) is 4 G KB, three staging buffers of 2 G KB each; inside 80 KB up to 128 stored columns."""
    for nearest in (False, True):
        used, cmap = S.readout_columns(256, 42, nearest)
        assert len(used) <= 104 and int(cmap.max()) == len(used) - 1
    plan = lambda w: -(-w // 16) * (4096 + 3 * 2048)
    assert plan(104) == 70 * 1024 and plan(128) == 80 * 1024 and plan(129) > 80 * 1024
