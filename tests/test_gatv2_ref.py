"""Pins tests/gatv2_ref.py, the yardstick of tests/test_gpu_gatv2.py (CPU).

The reference layer (forward and all three gradients) against a dense-index
torch float64 autograd implementation of the four GATv2 formulas, to 1e-10
relative; and the score at K = 1, C = 1, att = 1, slope = 1, where it is the
sum of the two edge scatters of tests/edge_ref.py.

The reference forms t = x_l[src] + x_r[dst] in float32 and torch forms it in
float64; so that both hold the same t, the inputs here are multiples of 2^-3
in [-2, 2], whose sums float32 represents exactly.  That grid also makes t
exactly 0 on some edges, and one x_r row is the negative of an in-edge's x_l
row; there both sides take the slope (torch's leaky_relu
has the derivative `slope` at 0).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import gatv2_ref as V  # noqa: E402

SLOPE = float(np.float32(0.2))   # the C-ABI takes a float: both sides use its value
GRAPHS = {"small": R.small_graph, "tiny": R.tiny_graph}


def _grid(rng, shape):
    """float32 multiples of 2^-3 in [-2, 2]"""
    return (rng.integers(-16, 17, shape) / 8.0).astype(np.float32)


def torch_gatv2(x_l, x_r, att, src_of_edge, dst_of_edge, n_dst, heads, slope):
    """Dense-index GATv2 layer under torch autograd, in the dtype of x_l:
    returns (y, score, alpha)."""
    e = len(src_of_edge)
    t = x_l[src_of_edge] + x_r[dst_of_edge]
    a = torch.nn.functional.leaky_relu(t, slope).view(e, heads, -1)
    score = (a * att.unsqueeze(0)).sum(-1)
    top = torch.full((n_dst, heads), -torch.inf, dtype=x_l.dtype).scatter_reduce(
        0, dst_of_edge.unsqueeze(1).expand(e, heads), score.detach(), "amax")
    ex = torch.exp(score - top[dst_of_edge])
    den = torch.zeros(n_dst, heads, dtype=x_l.dtype).index_add_(
        0, dst_of_edge, ex)
    alpha = ex / den[dst_of_edge]
    msg = alpha.unsqueeze(2) * x_l[src_of_edge].view(e, heads, -1)
    y = torch.zeros(n_dst, heads, msg.shape[2], dtype=x_l.dtype).index_add_(
        0, dst_of_edge, msg)
    return y.view(n_dst, -1), score, alpha


def _close(got, ref, name):
    ref = ref.detach().numpy() if isinstance(ref, torch.Tensor) else ref
    err = np.abs(np.asarray(got, dtype=np.float64) - ref)
    scale = np.abs(ref).max()
    assert scale > 0, name
    assert err.max() <= 1e-10 * scale, f"{name}: {err.max():.3e} of {scale:.3e}"


@pytest.mark.parametrize("heads,c_per", [(1, 1), (1, 5), (2, 4), (3, 7)])
@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_layer_against_torch_autograd(graph, heads, c_per):
    g = GRAPHS[graph]()
    f = heads * c_per
    rng = np.random.default_rng([31, heads, c_per, graph == "tiny"])
    x_l, x_r = _grid(rng, (g.v_src, f)), _grid(rng, (g.batch, f))
    d = int(np.flatnonzero(g.deg > 0)[0])
    x_r[d] = -x_l[int(g.row_indices[g.column_offset[d]]) - g.src_start]
    att = (rng.normal(size=(heads, c_per)) / np.sqrt(c_per)).astype(np.float32)
    gy = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)

    y, mag, sc, alpha = V.layer_forward(g, x_l, x_r, att, heads, SLOPE)
    (gxl, gxr, gatt), mags = V.layer_backward(g, x_l, x_r, att, alpha, gy,
                                              heads, SLOPE)
    assert (np.abs(y) <= mag + 1e-12).all()
    for grad, m in zip((gxl, gxr, gatt), mags):
        assert grad.shape == m.shape and (np.abs(grad) <= m + 1e-12).all()

    src = torch.from_numpy(g.row_indices.astype(np.int64) - g.src_start)
    dst = torch.from_numpy(np.array(g.dst_of_edge, dtype=np.int64))
    t32 = x_l[src.numpy()] + x_r[dst.numpy()]
    assert (t32 == 0).all(axis=1).any(), "no edge with t == 0 on its whole row"
    tl, tr, ta = (torch.from_numpy(a).double().requires_grad_(True)
                  for a in (x_l, x_r, att))
    ty, tsc, talpha = torch_gatv2(tl, tr, ta, src, dst, g.batch, heads, SLOPE)
    assert (t32.astype(np.float64)
            == (tl[src] + tr[dst]).detach().numpy()).all()
    ty.backward(torch.from_numpy(gy).double())
    tag = f"{graph} K={heads} C={c_per}"
    _close(sc, tsc, "score " + tag)
    _close(alpha, talpha, "alpha " + tag)
    _close(y, ty, "y " + tag)
    _close(gxl, tl.grad, "grad x_l " + tag)
    _close(gxr, tr.grad, "grad x_r " + tag)
    _close(gatt, ta.grad, "grad att " + tag)


@pytest.mark.parametrize("graph", sorted(GRAPHS))
def test_score_degenerates_to_the_two_scatters(graph):
    """K = 1, C = 1, att = 1, slope = 1: lrelu is the identity and the score
    is scatter_src_to_msg + scatter_dst_to_msg (exact on the grid inputs), its
    mag the absolute value."""
    g = GRAPHS[graph]()
    rng = np.random.default_rng([32, graph == "tiny"])
    x_l, x_r = _grid(rng, (g.v_src, 1)), _grid(rng, (g.batch, 1))
    sc, mag = V.score(g.column_offset, g.row_indices, g.src_start, x_r, x_l,
                      np.ones((1, 1), dtype=np.float32), 1.0, 1)
    full = np.zeros((g.src_start + g.v_src, 1), dtype=np.float32)
    full[g.src_start:] = x_l
    ident = np.arange(g.src_start + g.v_src, dtype=np.uint32)
    want = (R.scatter_src_to_msg(g.column_offset, g.row_indices, ident, full)
            + R.scatter_dst_to_msg(g.column_offset, g.row_indices, x_r))
    assert sc.shape == (g.edges, 1)
    assert (sc == want).all()
    assert (mag == np.abs(want)).all()


def test_backward_walks_add_onto_their_prefill():
    """backward() over the CSC with prefills equals the prefills plus the
    same walk from zero, and mag grows by |prefill|."""
    g = R.small_graph()
    heads, c_per = 2, 3
    f = heads * c_per
    rng = np.random.default_rng(33)
    x_l, x_r = _grid(rng, (g.v_src, f)), _grid(rng, (g.batch, f))
    att = rng.normal(size=(heads, c_per)).astype(np.float32)
    gs = rng.normal(size=(g.edges, heads)).astype(np.float32)
    po, pa = rng.normal(size=(g.batch, f)), rng.normal(size=f)
    args = (g.column_offset, g.row_indices, g.src_start, gs, x_r, x_l, att,
            SLOPE, heads)
    o0, m0, a0, n0 = V.backward(*args, np.zeros((g.batch, f)))
    o1, m1, a1, n1 = V.backward(*args, po, pa)
    for got, want in ((o1, o0 + po), (m1, m0 + np.abs(po)), (a1, a0 + pa),
                      (n1, n0 + np.abs(pa))):
        assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
