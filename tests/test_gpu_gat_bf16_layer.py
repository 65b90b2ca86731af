"""gat.GATLayer / gat.GATv2Layer and gat.attend / gat.attend_v2 with bfloat16
feature rows, on the GPU (marked gpu).

Forward: a bf16 value is widened exactly and every f-wide pass then runs the
fp32 arithmetic of its twin, so a layer given bf16 rows is compared with the
same layer given those rows widened to float32, bit for bit on destinations
of at most 256 in-edges (one work item: nothing depends on the order of
atomics) and at RTOL, ATOL of tests/test_gpu_gat_heads.py on the rest.

Autograd: against the dense-index float64 torch layers of the fp32 tests on
the widened values, at their tolerance, for y and every float32 gradient; the
row gradients come back in bfloat16, the float32 gradient of the kernels
rounded once, which on a graph where nothing is split is checked bit for bit
against layer.backward.

The chunk is the RMAT one of tests/test_gpu_gat_heads.py (V = 1200,
E = 20000, seed 13); the unsplit one is built as the `bounded` fixture of
tests/test_gpu_gather_bf16.py (V = 2000, degrees at most 200 both ways)."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
from test_gpu_gat_heads import (_assert_close, _layer_chunk,  # noqa: E402
                                torch_heads_reference)
from test_gpu_gatv2 import torch_gatv2_reference  # noqa: E402

pytestmark = pytest.mark.gpu

SLOPE = 0.2
SHAPES = [(1, 32), (4, 8), (8, 16), (3, 11)]
# (K, C, layer arguments, forward arguments)
MODES = ([(k, c, {}, {}) for k, c in SHAPES]
         + [(8, 16, {"stable": True}, {"dropout": 0.6, "seed": 1234})])
SPECIAL = [0x0000, -0x8000, 0x0001, 0x007f, -0x8000 + 0x0040]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _rows(rng, shape, dev):
    """U(-1, 1) rounded to bf16, with zeros, -0.0 and subnormals planted."""
    x = torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)).to(
        dev).to(torch.bfloat16)
    flat = x.view(-1)
    where = torch.from_numpy(rng.choice(flat.numel(), 8 * len(SPECIAL),
                                        replace=False)).to(dev)
    flat[where] = torch.tensor(SPECIAL, dtype=torch.int16, device=dev).view(
        torch.bfloat16).repeat(8)
    return x


def _f32(rng, shape, dev, scale=1.0):
    return torch.from_numpy(
        (scale * rng.uniform(-1, 1, shape)).astype(np.float32)).to(dev)


def _unsplit_dst(ch, dev):
    one = np.diff(ch.column_offset.astype(np.int64)) <= R.SPLIT
    assert one.any()
    return torch.from_numpy(one).to(dev)


def _assert_forward_twin(y16, y32, one, name):
    torch.cuda.synchronize()
    assert y16.dtype == torch.float32 and y16.shape == y32.shape
    assert torch.equal(y16[one].view(torch.int32), y32[one].view(torch.int32)), (
        f"{name}: unsplit destinations not bit-equal")
    _assert_close(y16, y32.double(), name)


@pytest.mark.parametrize("heads,c_per,largs,fargs", MODES)
def test_gat_forward_equals_widened_rows(dev, heads, c_per, largs, fargs):
    """GATLayer.forward(h_bf16, ...) against GATLayer.forward(h_bf16.float(),
    ...) with the same float32 scalars.  At K = 1 the bf16 layer runs the
    heads chain and the fp32 one the fused path: the same values."""
    from neutronstarlite_amd import gat
    v, ch = _layer_chunk()
    f = heads * c_per
    rng = np.random.default_rng([31000, heads, c_per])
    h = _rows(rng, (v, f), dev)
    shape = (v,) if heads == 1 else (v, heads)
    s_src, s_dst = _f32(rng, shape, dev), _f32(rng, shape, dev)
    layer = gat.GATLayer(ch, v, dev, heads=heads, **largs)
    y16, saved = layer.forward(h, s_src, s_dst, SLOPE, **fargs)
    assert saved["h"].dtype == torch.bfloat16
    y32, _ = layer.forward(h.float(), s_src, s_dst, SLOPE, **fargs)
    _assert_forward_twin(y16, y32, _unsplit_dst(ch, dev),
                         f"GAT forward K={heads} C={c_per} {largs} {fargs}")


@pytest.mark.parametrize("heads,c_per,largs,fargs", MODES)
def test_gatv2_forward_equals_widened_rows(dev, heads, c_per, largs, fargs):
    from neutronstarlite_amd import gat
    v, ch = _layer_chunk()
    f = heads * c_per
    rng = np.random.default_rng([32000, heads, c_per])
    x_l, x_r = _rows(rng, (v, f), dev), _rows(rng, (v, f), dev)
    att = _f32(rng, (heads, c_per), dev, 1.0 / np.sqrt(c_per))
    layer = gat.GATv2Layer(ch, v, dev, heads=heads, **largs)
    y16, _ = layer.forward(x_l, x_r, att, SLOPE, **fargs)
    y32, _ = layer.forward(x_l.float(), x_r.float(), att, SLOPE, **fargs)
    _assert_forward_twin(y16, y32, _unsplit_dst(ch, dev),
                         f"GATv2 forward K={heads} C={c_per} {largs} {fargs}")


@pytest.mark.parametrize("heads,c_per", SHAPES)
def test_attend_autograd_bf16(dev, heads, c_per):
    """gat.attend with a bf16 h, the scalars formed from h.float(), against
    the float64 dense-index layer on the widened values: y, grad a_src and
    grad a_dst at the fp32 test's tolerance; h.grad is bfloat16."""
    from neutronstarlite_amd import gat
    v, ch = _layer_chunk()
    f = heads * c_per
    rng = np.random.default_rng([33000, heads, c_per])
    h0 = _rows(rng, (v, f), dev)
    a_src0, a_dst0 = (_f32(rng, (heads, c_per), dev) for _ in range(2))
    gy = _f32(rng, (v, f), dev)

    layer = gat.GATLayer(ch, v, dev, heads=heads)
    h, a_src, a_dst = (t.clone().requires_grad_(True)
                       for t in (h0, a_src0, a_dst0))
    h3 = h.float().view(v, heads, c_per)
    y = gat.attend(h, (h3 * a_src).sum(-1), (h3 * a_dst).sum(-1), layer, SLOPE)
    assert y.shape == (v, f) and y.dtype == torch.float32
    y.backward(gy)
    assert h.grad.dtype == torch.bfloat16 and h.grad.shape == (v, f)
    assert bool(torch.isfinite(h.grad.float()).all())

    hr, ar, dr = (t.double().requires_grad_(True)
                  for t in (h0, a_src0, a_dst0))
    y_ref = torch_heads_reference(hr, ar, dr, layer.dst_of_edge,
                                  layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    tag = f"bf16 K={heads} C={c_per}"
    _assert_close(y, y_ref, f"attend y {tag}")
    _assert_close(a_src.grad, ar.grad, f"attend grad a_src {tag}")
    _assert_close(a_dst.grad, dr.grad, f"attend grad a_dst {tag}")


@pytest.mark.parametrize("heads,c_per", SHAPES)
def test_attend_v2_autograd_bf16(dev, heads, c_per):
    """gat.attend_v2 with bf16 x_l, x_r against the float64 dense-index layer
    on the widened values: y and grad att at the fp32 test's tolerance; the
    row gradients are bfloat16."""
    from neutronstarlite_amd import gat
    v, ch = _layer_chunk()
    f = heads * c_per
    rng = np.random.default_rng([34000, heads, c_per])
    xl0, xr0 = _rows(rng, (v, f), dev), _rows(rng, (v, f), dev)
    att0 = _f32(rng, (heads, c_per), dev, 1.0 / np.sqrt(c_per))
    gy = _f32(rng, (v, f), dev)

    layer = gat.GATv2Layer(ch, v, dev, heads=heads)
    x_l, x_r, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    y = gat.attend_v2(x_l, x_r, att, layer, SLOPE)
    assert y.shape == (v, f) and y.dtype == torch.float32
    y.backward(gy)
    for g in (x_l.grad, x_r.grad):
        assert g.dtype == torch.bfloat16 and g.shape == (v, f)
        assert bool(torch.isfinite(g.float()).all())
    assert att.grad.dtype == torch.float32

    lr, rr, ar = (t.double().requires_grad_(True) for t in (xl0, xr0, att0))
    y_ref, _ = torch_gatv2_reference(lr, rr, ar, layer.dst_of_edge,
                                     layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    tag = f"bf16 K={heads} C={c_per}"
    _assert_close(y, y_ref, f"attend_v2 y {tag}")
    _assert_close(att.grad, ar.grad, f"attend_v2 grad att {tag}")


@functools.lru_cache(maxsize=None)
def _bounded_chunk():
    """V = 2000, per-destination degree uniform in [0, 200], sources uniform:
    no vertex reaches the work-item split in either direction, so no atomics
    merge rows and every per-row result is deterministic to the bit."""
    from neutronstarlite_amd import graph as G
    v = 2000
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 201, size=v)
    deg[:3] = 0
    dst = np.repeat(np.arange(v, dtype=np.uint32), deg)
    src = rng.integers(0, v, size=dst.size).astype(np.uint32)
    assert np.bincount(dst, minlength=v).max() <= R.SPLIT
    assert np.bincount(src, minlength=v).max() <= R.SPLIT
    w = rng.uniform(0.1, 1.0, size=dst.size).astype(np.float32)
    return v, G.build_chunks(np.stack([src, dst], axis=1), w,
                             np.array([0, v], dtype=np.uint32), 0)[0]


def _same_bits(a, b):
    return a.dtype == b.dtype and torch.equal(a.view(torch.int16),
                                              b.view(torch.int16))


@pytest.mark.parametrize("heads,c_per", [(1, 32), (8, 16)])
def test_attend_row_gradient_is_the_fp32_one_rounded(dev, heads, c_per):
    """Nothing is split: layer.backward is deterministic, and h.grad of
    attend (scalars given as leaves of their own) is its float32 gradient
    .to(torch.bfloat16), bit for bit; the scalar gradients are the same
    float32 values."""
    from neutronstarlite_amd import gat
    v, ch = _bounded_chunk()
    f = heads * c_per
    rng = np.random.default_rng([35000, heads, c_per])
    h0 = _rows(rng, (v, f), dev)
    s0, d0 = (_f32(rng, (v, heads), dev) for _ in range(2))
    gy = _f32(rng, (v, f), dev)
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    h, s_src, s_dst = (t.clone().requires_grad_(True) for t in (h0, s0, d0))
    gat.attend(h, s_src, s_dst, layer, SLOPE).backward(gy)
    y, saved = layer.forward(h0, s0, d0, SLOPE)
    grad_h, g_src, g_dst = layer.backward(gy, saved, SLOPE)
    assert grad_h.dtype == torch.float32
    assert _same_bits(h.grad, grad_h.to(torch.bfloat16))
    assert torch.equal(s_src.grad, g_src.reshape(v, heads))
    assert torch.equal(s_dst.grad, g_dst.reshape(v, heads))


@pytest.mark.parametrize("heads,c_per", [(1, 32), (8, 16)])
def test_attend_v2_row_gradients_are_the_fp32_ones_rounded(dev, heads, c_per):
    """The same for attend_v2: x_l.grad and x_r.grad.  grad_att is summed by
    atomics in an order that is not fixed and is not compared here."""
    from neutronstarlite_amd import gat
    v, ch = _bounded_chunk()
    f = heads * c_per
    rng = np.random.default_rng([36000, heads, c_per])
    xl0, xr0 = _rows(rng, (v, f), dev), _rows(rng, (v, f), dev)
    att0 = _f32(rng, (heads, c_per), dev, 1.0 / np.sqrt(c_per))
    gy = _f32(rng, (v, f), dev)
    layer = gat.GATv2Layer(ch, v, dev, heads=heads)
    x_l, x_r, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    gat.attend_v2(x_l, x_r, att, layer, SLOPE).backward(gy)
    y, saved = layer.forward(xl0, xr0, att0, SLOPE)
    grad_xl, grad_xr, grad_att = layer.backward(gy, saved, SLOPE)
    assert grad_xl.dtype == grad_xr.dtype == grad_att.dtype == torch.float32
    assert _same_bits(x_l.grad, grad_xl.to(torch.bfloat16))
    assert _same_bits(x_r.grad, grad_xr.to(torch.bfloat16))


def test_rejected_inputs_raise_before_a_launch(dev):
    from neutronstarlite_amd import gat
    v, ch = _layer_chunk()
    heads, f = 4, 32
    bf = torch.bfloat16
    x = torch.zeros(v, f, device=dev)
    att = torch.zeros(heads, f // heads, device=dev)
    s = torch.zeros(v, heads, device=dev)

    v2 = gat.GATv2Layer(ch, v, dev, heads=heads)
    for call in (v2.forward, lambda *a: gat.attend_v2(*a, v2)):
        with pytest.raises(TypeError):           # the two rows differ
            call(x.to(bf), x, att)
        with pytest.raises(TypeError):
            call(x, x.to(bf), att)
        with pytest.raises(TypeError):           # att stays float32
            call(x.to(bf), x.to(bf), att.to(bf))
        with pytest.raises(TypeError):           # fp16 is not taken
            call(x.half(), x.half(), att)
    y, saved = v2.forward(x.to(bf), x.to(bf), att)
    with pytest.raises(TypeError):               # grad_y stays float32
        v2.backward(torch.zeros(v, f, device=dev, dtype=bf), saved)

    for layer, sc in ((gat.GATLayer(ch, v, dev, heads=heads), s),
                      (gat.GATLayer(ch, v, dev), torch.zeros(v, device=dev))):
        for call in (layer.forward, lambda *a: gat.attend(*a, layer)):
            with pytest.raises(TypeError):       # fp16 h
                call(x.half(), sc, sc)
            with pytest.raises(TypeError):       # the scalars stay float32
                call(x.to(bf), sc.to(bf), sc)
            with pytest.raises(TypeError):
                call(x.to(bf), sc, sc.to(bf))
        y, saved = layer.forward(x.to(bf), sc, sc)
        with pytest.raises(TypeError):
            layer.backward(torch.zeros(v, f, device=dev, dtype=bf), saved)
