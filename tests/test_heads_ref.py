"""tests/heads_ref.py, the float64 references of the multi-head kernels,
checked on the CPU: at one head they are the edge_ref functions exactly, and
their composition into a layer agrees with an independent dense-index
multi-head GAT layer under torch float64 autograd."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402

SLOPE = 0.2


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    assert (a == b).all()


def test_one_head_is_edge_ref():
    g = R.small_graph()
    rng = np.random.default_rng(1)
    full, mirror, s_dst = R.attention_inputs(g)
    for s_src, mi in ((mirror, g.mirror_index), (full, None)):
        m1, s1 = R.attention_forward(g.column_offset, g.row_indices, s_src,
                                     s_dst, mi, SLOPE)
        mk, sk = H.attention_forward(g.column_offset, g.row_indices,
                                     s_src[:, None], s_dst[:, None], mi, SLOPE)
        _same(mk[:, 0], m1)
        _same(sk[:, 0], s1)

    f = 7
    a = rng.normal(size=(g.batch, f)).astype(np.float32)
    b = rng.normal(size=(g.v_src, f)).astype(np.float32)
    d1, mag1 = R.edge_dot(g.column_offset, g.row_indices, g.src_start, a, b)
    dk, magk = H.edge_dot(g.column_offset, g.row_indices, g.src_start, a, b, 1)
    _same(dk[:, 0], d1)
    _same(magk[:, 0], mag1)

    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    for off in (g.column_offset, roff):
        n = len(off) - 1
        w = rng.normal(size=g.edges).astype(np.float32)
        pre = rng.normal(size=n).astype(np.float32)
        o1, mag1 = R.weight_sum(off, w, pre)
        ok, magk = H.weight_sum(off, w[:, None], pre[:, None])
        _same(ok[:, 0], o1)
        _same(magk[:, 0], mag1)

    # one head: the scalar-weight SpMM, written out edge by edge
    w = rng.uniform(-1, 1, g.edges).astype(np.float32)
    pre = rng.normal(size=(g.batch, f)).astype(np.float32)
    out, mag = H.gather(g.column_offset, g.row_indices, g.src_start, b, w, 1,
                        pre)
    ref, rmag = pre.astype(np.float64), np.abs(pre.astype(np.float64))
    for e in range(g.edges):
        term = np.float64(w[e]) * b[g.row_indices[e] - g.src_start].astype(
            np.float64)
        ref[g.dst_of_edge[e]] += term
        rmag[g.dst_of_edge[e]] += np.abs(term)
    np.testing.assert_allclose(out, ref, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(mag, rmag, rtol=1e-13, atol=1e-13)


def test_gather_heads_by_hand():
    """Three heads of two columns on the ten-vertex graph, edge by edge."""
    g = R.tiny_graph()
    rng = np.random.default_rng(2)
    heads, c_per = 3, 2
    x = rng.normal(size=(g.v_src, heads * c_per)).astype(np.float32)
    w = rng.uniform(-1, 1, (g.edges, heads)).astype(np.float32)
    pre = rng.normal(size=(g.batch, heads * c_per)).astype(np.float32)
    out, _ = H.gather(g.column_offset, g.row_indices, g.src_start, x, w, heads,
                      pre)
    ref = pre.astype(np.float64)
    for e in range(g.edges):
        for c in range(heads * c_per):
            ref[g.dst_of_edge[e], c] += (np.float64(w[e, c // c_per])
                                         * x[g.row_indices[e] - g.src_start, c])
    np.testing.assert_allclose(out, ref, rtol=1e-13, atol=1e-13)


def _torch_layer(g, h, s_src, s_dst, heads, slope):
    """Dense-index multi-head layer: softmax without max subtraction over
    each destination's in-edges, per head."""
    src = torch.from_numpy(g.row_indices.astype(np.int64) - g.src_start)
    dst = torch.from_numpy(np.array(g.dst_of_edge, dtype=np.int64))
    c_per = h.shape[1] // heads
    e = torch.nn.functional.leaky_relu(s_src[src] + s_dst[dst], slope)
    ex = torch.exp(e)
    den = torch.zeros(g.batch, heads, dtype=h.dtype).index_add_(0, dst, ex)
    s = ex / den[dst]                                      # (E, K)
    msg = s[:, :, None] * h[src].view(-1, heads, c_per)    # (E, K, C)
    y = torch.zeros(g.batch, heads, c_per, dtype=h.dtype).index_add_(
        0, dst, msg)
    return y.view(g.batch, heads * c_per)


@pytest.mark.parametrize("heads,c_per", [(1, 5), (3, 4), (4, 1)])
def test_layer_composition_against_torch_autograd(heads, c_per):
    """Forward and the three gradients the layer's backward returns (to h
    through the aggregation, to s_src, to s_dst).  The attention scalars are
    multiples of 1/64 in [-4, 4], so the float32 add the kernel performs is
    exact and both sides compute from the same m."""
    g = R.small_graph()
    rng = np.random.default_rng(3)
    f = heads * c_per
    h = rng.normal(size=(g.v_src, f)).astype(np.float32)
    s_src = (rng.integers(-256, 257, (g.v_src, heads)) / 64).astype(np.float32)
    s_dst = (rng.integers(-256, 257, (g.batch, heads)) / 64).astype(np.float32)
    grad_y = rng.normal(size=(g.batch, f)).astype(np.float32)

    y, m, s = H.layer_forward(g, h, s_src, s_dst, heads, SLOPE)
    grad_h, g_src, g_dst = H.layer_backward(g, h, s, m, grad_y, heads, SLOPE)
    assert m.dtype == np.float32

    th = torch.from_numpy(h).double().requires_grad_(True)
    ts = torch.from_numpy(s_src).double().requires_grad_(True)
    td = torch.from_numpy(s_dst).double().requires_grad_(True)
    # the slope is a float32 argument of the kernels, and of the references
    ty = _torch_layer(g, th, ts, td, heads, float(np.float32(SLOPE)))
    ty.backward(torch.from_numpy(grad_y).double())
    for name, got, ref in (("y", y, ty.detach()), ("grad_h", grad_h, th.grad),
                           ("g_src", g_src, ts.grad), ("g_dst", g_dst, td.grad)):
        np.testing.assert_allclose(got, ref.numpy(), rtol=1e-10, atol=1e-12,
                                   err_msg=name)
