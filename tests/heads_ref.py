"""Plain float64 numpy references for the multi-head (per-head edge weight)
kernels, built on tests/edge_ref.py.  A helper module: no tests here.

Layout, as in include/nts_hip.h: K heads of C columns, feature columns
head-major (column c belongs to head c // C), per-edge values (E, K),
per-vertex attention scalars (rows, K).  At K = 1 every function here is the
edge_ref function of the same name (tests/test_heads_ref.py).  Functions
whose bound needs the size of the computation also return `mag`, the sum of
the absolute values of the terms that were added (prefill included).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def gather(offset, nbr, nbr_start, x, w, heads, prefill):
    """out[v, c] = prefill[v, c] + sum over v's edge range of
    w[e, c // C] * x[nbr[e] - nbr_start, c].  Forward: (column_offset,
    row_indices, src_start), w in CSC order; backward: (row_offset,
    column_indices, dst_start), w in CSR order.  Returns (out, mag)."""
    x, p = _f64(x), _f64(prefill)
    f = x.shape[1]
    assert f % heads == 0
    c_per = f // heads
    w = _f64(w).reshape(-1, heads)
    rows = np.asarray(nbr).astype(np.int64) - int(nbr_start)
    out, mag = p.copy(), np.abs(p)
    for lo in range(0, f, 64):          # bounded temporaries at wide f
        cols = np.arange(lo, min(f, lo + 64))
        prod = x[rows][:, cols] * w[:, cols // c_per]
        out[:, cols] += R.segment_sum(prod, offset)
        mag[:, cols] += R.segment_sum(np.abs(prod), offset)
    return out, mag


def attention_forward(column_offset, row_indices, s_src, s_dst, mirror_index,
                      slope):
    """Per head k: edge_ref.attention_forward on column k of s_src (rows, K)
    and s_dst (batch, K).  Returns (m float32 (E, K), softmax float64 (E, K))."""
    s_src, s_dst = np.asarray(s_src), np.asarray(s_dst)
    heads = s_dst.shape[1]
    cols = [R.attention_forward(column_offset, row_indices, s_src[:, k],
                                s_dst[:, k], mirror_index, slope)
            for k in range(heads)]
    return (np.stack([c[0] for c in cols], axis=1),
            np.stack([c[1] for c in cols], axis=1))


def edge_dot(column_offset, row_indices, src_start, dst_rows, src_rows, heads):
    """out[e, k] = dst_rows[dst(e), head k] . src_rows[src(e), head k].
    Returns (dot, mag), both (E, K), mag = sum over the head of |a_j b_j|."""
    a, b = np.asarray(dst_rows), np.asarray(src_rows)
    c_per = a.shape[1] // heads
    assert c_per * heads == a.shape[1]
    cols = [R.edge_dot(column_offset, row_indices, src_start,
                       a[:, k * c_per:(k + 1) * c_per],
                       b[:, k * c_per:(k + 1) * c_per]) for k in range(heads)]
    return (np.stack([c[0] for c in cols], axis=1),
            np.stack([c[1] for c in cols], axis=1))


def weight_sum(offset, weights, prefill):
    """out[v, k] = prefill[v, k] + sum of weights[e, k] over v's edge range.
    Returns (out, mag), both (n, K)."""
    w, p = _f64(weights), _f64(prefill)
    return (p + R.segment_sum(w, offset),
            np.abs(p) + R.segment_sum(np.abs(w), offset))


# --------------------------------------------------------------------------
# the layer: the composition gat.GATLayer runs with heads = K
# --------------------------------------------------------------------------
def layer_forward(g, h, s_src, s_dst, heads, slope):
    """h (v_src, K*C), s_src (v_src, K) by source row, s_dst (batch, K).
    Returns (y (batch, K*C) float64, m float32 (E, K), s float64 (E, K))."""
    full = np.zeros((g.src_start + g.v_src, heads), dtype=np.float32)
    full[g.src_start:] = s_src
    m, s = attention_forward(g.column_offset, g.row_indices, full, s_dst,
                             None, slope)
    y, _ = gather(g.column_offset, g.row_indices, g.src_start, h, s, heads,
                  np.zeros((g.batch, np.asarray(h).shape[1])))
    return y, m, s


def layer_backward(g, h, s, m, grad_y, heads, slope):
    """The backward chain: CSR gather with the CSR-order softmax, per-head
    edge dot, softmax backward with the leaky-relu mask, then the sums of the
    edge gradient by source (CSR order) and by destination (CSC order).
    Destination d is global vertex src_start + d.  Returns (grad_h, g_src,
    g_dst)."""
    perm, _ = R.csc_to_csr(g.row_indices)
    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    col_idx = g.src_start + g.dst_of_edge[perm]
    f = np.asarray(h).shape[1]
    grad_h, _ = gather(roff, col_idx, g.src_start, grad_y, _f64(s)[perm],
                       heads, np.zeros((g.v_src, f)))
    gs, _ = edge_dot(g.column_offset, g.row_indices, g.src_start, grad_y, h,
                     heads)
    ge, _ = R.softmax_backward(g.column_offset, gs, s, m, slope)
    g_src, _ = weight_sum(roff, ge[perm], np.zeros((g.v_src, heads)))
    g_dst, _ = weight_sum(g.column_offset, ge, np.zeros((g.batch, heads)))
    return grad_h, g_src, g_dst
