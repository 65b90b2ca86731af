"""Plain float64 numpy references for the GATv2 score and backward kernels
and the layer built on them, on top of tests/edge_ref.py and
tests/heads_ref.py.  A helper module: no tests here.

  t[e, c]     = x_l[src(e), c] + x_r[dst(e), c]        c < f = K*C, head-major
  score[e, k] = sum_{j<C} att[k*C + j] * lrelu(t[e, k*C + j])
  alpha       = softmax of score over dst(e)'s in-edges, per head
  y[d, c]     = sum_{e into d} alpha[e, c // C] * x_l[src(e), c]

t and the leaky-relu mask are formed in FLOAT32, one add of the float32
inputs, exactly what include/nts_hip.h promises of the kernels; everything
after that is float64.  lrelu(t) = t > 0 ? t : slope*t and lrelu'(t) =
t > 0 ? 1 : slope, so t == 0 takes the slope.  Every function also returns
`mag`, the sum of the absolute values of the terms that were added (prefill
included), for the tests' bounds.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402

COLS = 64   # columns per pass: bounded (E, COLS) temporaries at wide f


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _t32(own, nbr_rows, voe, rows, cols):
    """float32 t of the edges for a block of columns: ONE float32 add."""
    t = own[voe][:, cols] + nbr_rows[rows][:, cols]
    assert t.dtype == np.float32
    return t


def _lrelu(t32, slope):
    t = t32.astype(np.float64)
    return np.where(t32 > 0, t, float(np.float32(slope)) * t)


def _dlrelu(t32, slope):
    return np.where(t32 > 0, 1.0, float(np.float32(slope)))


def score(column_offset, row_indices, src_start, dst_rows, src_rows, att,
          slope, heads):
    """score[e, k] = sum_j att[k*C+j] * lrelu(dst_rows[dst(e)] + src_rows[src(e)
    - src_start]) over head k's columns.  Returns (score, mag), both (E, K)."""
    a, b = _f32(dst_rows), _f32(src_rows)
    f = a.shape[1]
    assert f % heads == 0 and b.shape[1] == f
    c_per = f // heads
    w = _f64(_f32(att)).reshape(-1)
    assert w.size == f
    doe = R._dst_of_edge(column_offset)
    rows = np.asarray(row_indices).astype(np.int64) - int(src_start)
    out = np.zeros((len(rows), heads))
    mag = np.zeros((len(rows), heads))
    for k in range(heads):
        for lo in range(k * c_per, (k + 1) * c_per, COLS):
            cols = np.arange(lo, min((k + 1) * c_per, lo + COLS))
            term = _lrelu(_t32(a, b, doe, rows, cols), slope) * w[cols]
            out[:, k] += term.sum(axis=1)
            mag[:, k] += np.abs(term).sum(axis=1)
    return out, mag


def backward(offset, nbr, nbr_start, grad_score, own_rows, nbr_rows, att,
             slope, heads, own_prefill, att_prefill=None):
    """One walk over `offset` (CSC: own = x_r, nbr = x_l; CSR: own = x_l,
    nbr = x_r) with grad_score (E, K) in that array's edge order:
      grad_own[v, c] = own_prefill + sum_e gs[e, c//C] * att[c] * lrelu'(t)
      grad_att[c]    = att_prefill + sum_v sum_e gs[e, c//C] * lrelu(t)
    att_prefill None: zero.  Returns (grad_own, mag_own, grad_att, mag_att),
    grad_att and mag_att of shape (f,)."""
    return _walk(offset, nbr, nbr_start, _f64(_f32(grad_score)), own_rows,
                 nbr_rows, att, slope, heads, own_prefill, None, att_prefill)


def _walk(offset, nbr, nbr_start, grad_score, own_rows, nbr_rows, att, slope,
          heads, own_prefill, own_prefill_mag, att_prefill):
    """backward() with grad_score in float64 as given (inside the layer chain
    it is an intermediate, not a float32 input) and the prefill's own mag."""
    own, nb = _f32(own_rows), _f32(nbr_rows)
    f = own.shape[1]
    assert f % heads == 0 and nb.shape[1] == f
    c_per = f // heads
    w = _f64(_f32(att)).reshape(-1)
    gs = _f64(grad_score).reshape(-1, heads)
    voe = R._dst_of_edge(offset)
    rows = np.asarray(nbr).astype(np.int64) - int(nbr_start)
    g_own = _f64(own_prefill).copy()
    m_own = (np.abs(g_own) if own_prefill_mag is None
             else _f64(own_prefill_mag).copy())
    pa = np.zeros(f) if att_prefill is None else _f64(att_prefill).reshape(-1)
    g_att, m_att = pa.copy(), np.abs(pa)
    for lo in range(0, f, COLS):
        cols = np.arange(lo, min(f, lo + COLS))
        t = _t32(own, nb, voe, rows, cols)
        g = gs[:, cols // c_per]
        term = g * w[cols] * _dlrelu(t, slope)
        g_own[:, cols] += R.segment_sum(term, offset)
        m_own[:, cols] += R.segment_sum(np.abs(term), offset)
        term = g * _lrelu(t, slope)
        g_att[cols] += term.sum(axis=0)
        m_att[cols] += np.abs(term).sum(axis=0)
    return g_own, m_own, g_att, m_att


def softmax(column_offset, x):
    """edge_ref.softmax_forward with the destination's maximum subtracted
    first (the same value in exact arithmetic, and finite for any score)."""
    off = np.asarray(column_offset, dtype=np.int64)
    doe = R._dst_of_edge(off)
    x = _f64(x)
    top = np.full((len(off) - 1,) + x.shape[1:], -np.inf)
    live = np.diff(off) > 0
    if live.any():
        top[live] = np.maximum.reduceat(x, off[:-1][live], axis=0)
    return R.softmax_forward(off, x - top[doe])


# --------------------------------------------------------------------------
# the layer: the composition gat.GATv2Layer runs
# --------------------------------------------------------------------------
def layer_forward(g, x_l, x_r, att, heads, slope):
    """x_l (v_src, K*C) by source row, x_r (batch, K*C), att (K, C).
    Returns (y, mag, score, alpha): y and its mag (batch, K*C), score and
    alpha (E, K), all float64."""
    sc, _ = score(g.column_offset, g.row_indices, g.src_start, x_r, x_l, att,
                  slope, heads)
    alpha = softmax(g.column_offset, sc)
    f = np.asarray(x_l).shape[1]
    y, mag = H.gather(g.column_offset, g.row_indices, g.src_start, x_l, alpha,
                      heads, np.zeros((g.batch, f)))
    return y, mag, sc, alpha


def layer_backward(g, x_l, x_r, att, alpha, grad_y, heads, slope):
    """The backward chain of gat.GATv2Layer: CSR gather with the CSR-order
    softmax, per-head edge dot, softmax backward (no mask), the CSC walk
    (grad x_r, grad att) and the CSR walk added into grad x_l.  Destination d
    is global vertex src_start + d.  Returns ((grad_xl, grad_xr, grad_att),
    (mag_xl, mag_xr, mag_att)), grad_att of shape (K, C)."""
    perm, _ = R.csc_to_csr(g.row_indices)
    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    col_idx = g.src_start + g.dst_of_edge[perm]
    f = np.asarray(x_l).shape[1]
    gxl, mxl = H.gather(roff, col_idx, g.src_start, grad_y, _f64(alpha)[perm],
                        heads, np.zeros((g.v_src, f)))
    galpha, _ = H.edge_dot(g.column_offset, g.row_indices, g.src_start,
                           grad_y, x_l, heads)
    gscore, _ = R.softmax_backward(g.column_offset, galpha, alpha)
    zero = np.zeros((g.batch, f))
    gxr, mxr, gatt, matt = _walk(
        g.column_offset, g.row_indices, g.src_start, gscore, x_r, x_l, att,
        slope, heads, zero, None, None)
    gxl, mxl, _, _ = _walk(roff, col_idx, g.src_start, gscore[perm], x_l, x_r,
                           att, slope, heads, gxl, mxl, None)
    shape = (heads, f // heads)
    return ((gxl, gxr, gatt.reshape(shape)), (mxl, mxr, matt.reshape(shape)))
