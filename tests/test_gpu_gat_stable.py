"""gat.GATLayer(..., stable=True) under gat.attend with attention logits out
to +-150, against an independent dense-index float64 torch-autograd layer
(marked gpu), and the same inputs through the default layer, which must come
back non-finite: that is why the mode exists.

The chunk is small (300 vertices, about 2,800 edges) and has one destination
of more than 256 in-edges, so the layer also runs the merge of several work
items' maxima and sums.

Tolerance: RTOL, ATOL of tests/test_gpu_gat_heads.py (1e-4*|ref| + 2e-5),
which that file holds for h, grad_y in [-1, 1] and per-head sums of at most
128 terms.  The magnitudes here: h and grad_y are again uniform in [-1, 1]
and a head has C = 8 or 32 columns, so the per-head dots have at most 32
terms; y is a convex combination of h rows, |y| <= 1, whatever the logits;
the softmax weights are in [0, 1] and sum to 1, and a weight s = exp(x)/S
carries an absolute error of about 1.2e-7*|x|*exp(x) <= 5e-8 (x <= 0, S >= 1),
far below the 2e-5 floor after the at most 300-term sums of the backward.
float64 exp is safe to 700, so the reference needs no max subtraction.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2e-5   # of tests/test_gpu_gat_heads.py
SLOPE = 0.2
SCALE = 75.0              # scalars in [-75, 75]: logits in [-150, 150]


def _assert_close(got, ref, name):
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = ref.detach().cpu().numpy().astype(np.float64)
    assert np.isfinite(got).all(), f"{name}: non-finite"
    err = np.abs(got - ref)
    bound = RTOL * np.abs(ref) + ATOL
    print(f"{name}: worst {float((err / bound).max()):.3e} of the tolerance")
    bad = err > bound
    assert not bad.any(), (f"{name}: {bad.sum()}/{bad.size} out of tol, "
                           f"worst {err.max():.3e}")


@functools.lru_cache(maxsize=None)
def _chunk():
    from neutronstarlite_amd import graph as G
    v = 300
    hub = np.stack([np.arange(v), np.full(v, 5)], axis=1).astype(np.uint32)
    edges = np.concatenate([G.rmat_edges(v, 2200, seed=21), hub])
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    ch = G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]
    assert np.diff(ch.column_offset.astype(np.int64)).max() > 256
    return v, ch


def torch_reference(h, s_src, s_dst, dst_of_edge, src_of_edge, v, heads,
                    slope):
    """Dense-index K-head attention aggregation in the dtype of h."""
    h3 = h.view(v, heads, -1)
    e = torch.nn.functional.leaky_relu(
        s_src.view(v, heads)[src_of_edge] + s_dst.view(v, heads)[dst_of_edge],
        slope)
    ex = torch.exp(e)
    den = torch.zeros(v, heads, dtype=h.dtype, device=h.device).index_add_(
        0, dst_of_edge, ex)
    s = ex / den[dst_of_edge]
    y = torch.zeros_like(h3).index_add_(
        0, dst_of_edge, s.unsqueeze(2) * h3[src_of_edge])
    return y.view(v, -1)


def _inputs(heads, dev):
    v, _ = _chunk()
    f = 32
    rng = np.random.default_rng([7, heads])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    shape = (v,) if heads == 1 else (v, heads)
    return (up(rng.uniform(-1, 1, size=(v, f))),
            up(rng.uniform(-SCALE, SCALE, size=shape)),
            up(rng.uniform(-SCALE, SCALE, size=shape)),
            up(rng.uniform(-1, 1, size=(v, f))))


@pytest.mark.parametrize("heads", [1, 4])
def test_stable_layer_attend_autograd(heads):
    """y, grad h, grad s_src and grad s_dst of gat.attend on a stable layer,
    single-head path (heads = 1) and heads path (heads = 4)."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _chunk()
    h0, src0, dst0, gy = _inputs(heads, dev)
    layer = gat.GATLayer(ch, v, dev, heads=heads, stable=True)
    assert layer.stable is True
    h, s_src, s_dst = (t.clone().requires_grad_(True)
                       for t in (h0, src0, dst0))
    y = gat.attend(h, s_src, s_dst, layer, SLOPE)
    y.backward(gy)
    assert layer.stream.edge_softmax_stable_last() == 1

    hr, sr, dr = (t.double().requires_grad_(True) for t in (h0, src0, dst0))
    logits = (sr.detach().view(v, heads)[layer.src_of_edge]
              + dr.detach().view(v, heads)[layer.dst_of_edge])
    assert float(logits.max()) > 120 and float(logits.min()) < -120
    y_ref = torch_reference(hr, sr, dr, layer.dst_of_edge, layer.src_of_edge,
                            v, heads, SLOPE)
    assert bool(torch.isfinite(y_ref).all())
    y_ref.backward(gy.double())
    tag = f"stable K={heads}"
    _assert_close(y, y_ref, f"attend y {tag}")
    _assert_close(h.grad, hr.grad, f"attend grad h {tag}")
    _assert_close(s_src.grad, sr.grad, f"attend grad s_src {tag}")
    _assert_close(s_dst.grad, dr.grad, f"attend grad s_dst {tag}")


@pytest.mark.parametrize("heads", [1, 4])
def test_default_layer_is_not_finite_there(heads):
    """The same inputs through stable=False: exp overflows past a logit of
    about 88.7 and the destination's row is NaN."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _chunk()
    h0, src0, dst0, _ = _inputs(heads, dev)
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    assert layer.stable is False
    y, _ = layer.forward(h0, src0, dst0, SLOPE)
    torch.cuda.synchronize()
    assert layer.stream.edge_softmax_stable_last() == 0
    assert not bool(torch.isfinite(y).all())


def test_stable_must_be_a_bool():
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _chunk()
    for bad in (1, 0, "yes", None):
        with pytest.raises(ValueError):
            gat.GATLayer(ch, v, dev, stable=bad)
