"""The GAT training backward that recomputes the attention weights (marked
gpu): Stream.gat_backward_fused[_bf16] against the float64 layer of
tests/heads_ref.py, bit-equality of grad_h with the cached chain, and
GATLayer.forward_recompute / gat.attend(recompute=True) under autograd.
The entry cases run on one graph with split and unsplit vertices on both sides
(`_graph`).  Bounds are RTOL, ATOL of test_gpu_gat_heads.py (1e-4, 2e-5), what
the cached backward is held to; both softmax modes share the float64
reference (inputs far from overflow).
"""
import functools
import gc
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402
from test_gpu_gat_bf16 import Inp16, round_bf16, widen  # noqa: E402
from test_gpu_gat_heads import (ATOL, RTOL, SLOPE, Buf, Inp,  # noqa: E402
                                _assert_bits, _assert_bound, _assert_close,
                                _layer_chunk, _up32, torch_heads_reference)
from test_gpu_gat_infer import _layer_inputs  # noqa: E402

pytestmark = pytest.mark.gpu

IN_DEGREES = (0, 1, 3, 4, 5, 64, 65, 256, 257, 1000)
HUB_OUT, FULL_OUT = 600, 256     # forced out-degrees: 2 items + 88, one item
FAST = [(8, 16), (2, 2), (16, 1), (1, 64)]     # R = 4, 2, 1, 4
GENERAL = [(3, 7), (1, 33)]


@functools.lru_cache(maxsize=None)
def _graph():
    """In-degrees IN_DEGREES plus 100 of degree 0..8; source `a` forced to
    out-degree 600 and `b` to exactly 256, mostly inside the degree-1000
    destination (few other sources then meet it), 40 / 26 edges elsewhere."""
    rng = np.random.default_rng(31000)
    deg = np.concatenate([IN_DEGREES, rng.integers(0, 9, 100)])
    deg = deg[rng.permutation(len(deg))]
    v_src, src_start, seed = 3000, 500, 31001
    free = np.setdiff1d(np.arange(src_start, src_start + v_src),
                        R.build_graph(deg, v_src, src_start, seed).uniq)
    a, b = int(free[0]), int(free[len(free) // 2])
    off = np.concatenate([[0], np.cumsum(deg)])
    hub = int(np.flatnonzero(deg == 1000)[0])
    inside = np.arange(off[hub], off[hub + 1])
    outside = rng.permutation(np.setdiff1d(np.arange(off[-1]), inside))[:66]
    forced = ([(s, a) for s in inside[:HUB_OUT - 40]] +
              [(s, a) for s in outside[:40]] +
              [(s, b) for s in inside[-(FULL_OUT - 26):]] +
              [(s, b) for s in outside[40:]])
    g = R.build_graph(deg, v_src, src_start, seed, forced=forced)
    g.a, g.b = a - src_start, b - src_start
    perm, _ = R.csc_to_csr(g.row_indices)
    g.row_offset = R.csr_offsets(g.row_indices, src_start, v_src)
    g.column_indices = (src_start + g.dst_of_edge[perm]).astype(np.uint32)
    g.out_deg = np.diff(g.row_offset.astype(np.int64))
    worst_in = np.zeros(v_src, dtype=np.int64)
    np.maximum.at(worst_in, g.row_indices.astype(np.int64) - src_start,
                  g.deg[g.dst_of_edge])
    # one-item sources all of whose destinations are one item
    g.exact = (g.out_deg > 0) & (g.out_deg <= R.SPLIT) & (worst_in <= R.SPLIT)
    return g


def test_graph_properties():
    g = _graph()
    for d in IN_DEGREES:
        assert (g.deg == d).sum() >= 1, d
    assert g.out_deg[g.a] == HUB_OUT == 2 * R.SPLIT + 88
    assert g.out_deg[g.b] == FULL_OUT == R.SPLIT
    assert (g.out_deg == 0).sum() > 100 and g.src_start != 0
    assert 2 * g.exact.sum() >= (g.out_deg > 0).sum()
    assert not g.exact[g.a] and not g.exact[g.b]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    g = _graph()
    env = {"dev": dev, "shim": shim,
           "topo": [_up32(dev, a) for a in (g.row_indices, g.column_offset,
                                            g.row_offset, g.column_indices)]}
    for stable in (False, True):
        for general in (False, True):
            st = env[stable, general] = shim.Stream.wrap_torch_current()
            st.edge_softmax_stable(int(stable))
            st.heads_dbg_general(int(general))
    yield env
    for key in [k for k in env if isinstance(k, tuple)]:
        env[key].destroy()


@functools.lru_cache(maxsize=None)
def _case(heads, c_per, bf16):
    """Inputs, non-zero prefills and the float64 reference (prefill
    included) of one shape; h is rounded to bf16 first when bf16."""
    g = _graph()
    f = heads * c_per
    rng = np.random.default_rng([32000, heads, c_per])
    h = rng.uniform(-1, 1, (g.v_src, f)).astype(np.float32)
    bits = round_bf16(h)
    if bf16:
        h = widen(bits)
    s_src = rng.uniform(-1, 1, (g.v_src, heads)).astype(np.float32)
    s_dst = rng.uniform(-1, 1, (g.batch, heads)).astype(np.float32)
    gy = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    pre = [(rng.normal(size=s) + 3).astype(np.float32)
           for s in ((g.v_src, f), (g.v_src, heads), (g.batch, heads))]
    _, m, s = H.layer_forward(g, h, s_src, s_dst, heads, SLOPE)
    ref = [p + r for p, r in zip(pre, H.layer_backward(g, h, s, m, gy, heads,
                                                       SLOPE))]
    return h, bits, s_src, s_dst, gy, pre, ref


def _run(gpu, st, heads, c_per, bf16, shift=0):
    """The fused forward's y, then the fused backward onto the case's
    prefills; shift moves h, grad_y and grad_h that many elements."""
    g, dev = _graph(), gpu["dev"]
    f = heads * c_per
    h, bits, s_src, s_dst, gy, case_pre, _ = _case(heads, c_per, bf16)
    d_h = Inp16(dev, bits, shift) if bf16 else Inp(dev, h, shift)
    d_src, d_dst, d_gy = Inp(dev, s_src), Inp(dev, s_dst), Inp(dev, gy, shift)
    rows, coff, roff, cidx = (t.data_ptr() for t in gpu["topo"])
    span = (g.src_start, g.src_start + g.v_src, g.src_start,
            g.src_start + g.batch)
    y = torch.zeros(g.batch, f, device=dev)
    # the forward indexes s_src by the global source id
    (st.gat_forward_fused_bf16 if bf16 else st.gat_forward_fused)(
        d_h.ptr, y.data_ptr(), d_src.ptr - 4 * g.src_start * heads, d_dst.ptr,
        rows, None, SLOPE, coff, *span, g.edges, g.batch, f, heads)
    outs = [Buf(dev, p.shape, p, shift if i == 0 else 0)
            for i, p in enumerate(case_pre)]
    ran = (st.gat_backward_fused_bf16 if bf16 else st.gat_backward_fused)(
        d_h.ptr, y.data_ptr(), d_gy.ptr, *(o.ptr for o in outs), d_src.ptr,
        d_dst.ptr, SLOPE, rows, coff, roff, cidx, *span, g.edges, f, heads)
    assert ran == 1
    return [o.read(n) for o, n in zip(outs, ("grad_h", "g_src", "g_dst"))]


ENTRY_CASES = ([(k, c, gen, 0) for k, c in FAST for gen in (False, True)] +
               [(k, c, False, 0) for k, c in GENERAL] + [(8, 16, False, 1)])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,c_per,general,shift", ENTRY_CASES)
def test_backward_fused(gpu, heads, c_per, general, shift, stable, bf16):
    """grad_h, grad_s_src, grad_s_dst onto non-zero prefills between guard
    bands, within RTOL * |ref| + ATOL of the float64 layer backward; vertices
    without edges keep their prefill bit for bit; the plan reports the form
    and the lane width of the header's rule."""
    g = _graph()
    f = heads * c_per
    pow2 = c_per & (c_per - 1) == 0
    align = 256 if not shift else 2 if bf16 else 4
    plan = gpu["shim"].gat_backward_fused_plan(
        f, heads, 2 if bf16 else 4, align, 4 if shift else 256, g.v_src,
        g.batch, g.edges, general)
    want = next(r for r in (4, 2, 1) if c_per % r == 0 and not (shift and r > 1))
    assert (plan["form"], plan["cols_per_lane"]) == (
        (1, want) if pow2 and not general else (2, 1)), plan
    st = gpu[stable, general]
    got = _run(gpu, st, heads, c_per, bf16, shift)
    assert st.edge_softmax_stable_last() == int(stable)
    _, _, _, _, _, pre, ref = _case(heads, c_per, bf16)
    tag = f"K={heads} C={c_per} general={general} stable={stable} bf16={bf16}"
    empty = (g.out_deg == 0, g.out_deg == 0, g.deg == 0)
    for name, a, r, p, z in zip(("grad_h", "g_src", "g_dst"), got, ref, pre,
                                empty):
        _assert_bound(a, r, RTOL * np.abs(r) + ATOL, f"{name} {tag}")
        _assert_bits(a[z], p[z], f"{name} {tag}, vertices without edges")


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (3, 7)])
def test_layer_on_offset_chunk_and_cached_bits(gpu, heads, c_per, stable):
    """GATLayer on a chunk with src_s = 500 (s_src by global source id):
    forward_recompute + backward within RTOL, ATOL of the float64 backward;
    on sources of one work item whose destinations are each one work item
    grad_h is _backward_heads' bit for bit (same weight, same fmaf chain)."""
    from neutronstarlite_amd import gat
    from neutronstarlite_amd.graph import Chunk
    g, dev = _graph(), gpu["dev"]
    h, _, s_src, s_dst, gy, pre, ref = _case(heads, c_per, False)
    w = np.ones(g.edges, dtype=np.float32)
    lo = g.src_start
    ch = Chunk(lo, lo + g.v_src, lo, lo + g.batch, g.column_offset.copy(),
               g.row_indices.copy(), w, g.row_offset, g.column_indices, w)
    layer = gat.GATLayer(ch, lo + g.v_src, dev, heads=heads, stable=stable,
                         _heads_path=True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    full = np.zeros((lo + g.v_src, heads), dtype=np.float32)
    full[lo:] = s_src
    args = (up(h), up(full), up(s_dst), SLOPE)
    want = layer.backward(up(gy), layer.forward(*args)[1], SLOPE)
    got = layer.backward(up(gy), layer.forward_recompute(*args)[1], SLOPE)
    got, want = ([t.cpu().numpy() for t in ts] for ts in (got, want))
    for name, a, r, p in zip(("grad_h", "g_src", "g_dst"), got, ref, pre):
        _assert_bound(a, r - p, RTOL * np.abs(r - p) + ATOL,
                      f"layer {name} K={heads} C={c_per} stable={stable}")
    _assert_bits(got[0][g.exact], want[0][g.exact], f"grad_h K={heads}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_attend_recompute_autograd(heads, stable, bf16):
    """gat.attend(..., recompute=True) with h, s_src and s_dst as leaves
    against the float64 dense-index layer: y and the three gradients within
    RTOL, ATOL.  The reference gets per-vertex copies of a_src, a_dst:
    d/da[v, k, :] = g_s[v, k] * h[v, k, :] gives the scalar gradients g_s, and
    h's gradient less g_s * a is the aggregation's.  A bfloat16 h.grad is the
    float32 one rounded once: 2^-8 * |ref| more (8 significand bits)."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    h0, s_src0, s_dst0, a_src0, a_dst0, h32 = _layer_inputs(heads, 32 // heads,
                                                            dev, bf16)
    gy = torch.from_numpy(np.random.default_rng([33000, heads]).uniform(
        -1, 1, (v, 32)).astype(np.float32)).to(dev)
    layer = gat.GATLayer(ch, v, dev, heads=heads, stable=stable)
    h, s_src, s_dst = (t.clone().requires_grad_(True)
                       for t in (h0, s_src0, s_dst0))
    y = gat.attend(h, s_src, s_dst, layer, SLOPE, recompute=True)
    y.backward(gy)
    assert h.grad.dtype == h.dtype and s_src.grad.shape == s_src0.shape

    hr = h32.double().requires_grad_(True)
    ar, dr = (a.double().expand(v, heads, -1).clone().requires_grad_(True)
              for a in (a_src0, a_dst0))
    y_ref = torch_heads_reference(hr, ar, dr, layer.dst_of_edge,
                                  layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    h3 = hr.detach().view(v, heads, -1)
    g_src, g_dst = ((a.grad * h3).sum(-1) / (h3 * h3).sum(-1)
                    for a in (ar, dr))
    g_h = hr.grad - (g_src[..., None] * ar + g_dst[..., None] * dr).view(v, -1)
    tag = f"K={heads} stable={stable} bf16={bf16}"
    _assert_close(y, y_ref, f"recompute y {tag}")
    _assert_close(s_src.grad.view(v, heads), g_src, f"recompute g_src {tag}")
    _assert_close(s_dst.grad.view(v, heads), g_dst, f"recompute g_dst {tag}")
    if not bf16:
        _assert_close(h.grad, g_h, f"recompute grad h {tag}")
    else:
        err = (h.grad.double() - g_h.detach()).abs()
        bound = (RTOL + 2.0 ** -8) * g_h.detach().abs() + ATOL
        assert bool((err <= bound).all()), f"recompute grad h {tag}"


def test_attend_recompute_arguments():
    """recompute=True with dropout raises before a launch; recompute=False
    keeps the training path's `saved`; y changed in place raises in backward."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    h, s_src, s_dst, _, _, _ = _layer_inputs(4, 8, dev, False)
    layer = gat.GATLayer(ch, v, dev, heads=4)
    with pytest.raises(ValueError):
        gat.attend(h, s_src, s_dst, layer, SLOPE, 0.5, recompute=True)
    assert "recompute" not in layer.forward(h, s_src, s_dst, SLOPE)[1]
    _, saved = layer.forward_recompute(h, s_src, s_dst, SLOPE)
    assert sorted(saved) == ["h", "recompute", "s_dst", "s_src", "y"]
    with pytest.raises(ValueError):          # grad_y of another width
        layer.backward(torch.zeros(v, 16, device=dev), saved, SLOPE)
    y = gat.attend(h.clone().requires_grad_(True), s_src, s_dst, layer, SLOPE,
                   recompute=True)
    with pytest.raises(RuntimeError):        # D = grad_y . y needs y intact
        y.add_(1).sum().backward()


def test_recompute_step_allocates_nothing_edge_sized():
    """K = 8, C = 4: forward_recompute + backward raise torch's peak by less
    than one [E, K] float32 array (678 400 B; y, grad_h and the two scalar
    gradients are 384 KB), the cached pair by at least three."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    h, s_src, s_dst, _, _, _ = _layer_inputs(8, 4, dev, False)
    gy = torch.ones(v, 32, device=dev)
    layer = gat.GATLayer(ch, v, dev, heads=8)
    edge_bytes = ch.edge_size * 8 * 4
    assert edge_bytes == 678400

    def step(forward):
        y, saved = forward(h, s_src, s_dst, SLOPE)
        return layer.backward(gy, saved, SLOPE)

    def peak_of(fn):      # the pattern of test_gpu_gat_infer.py
        fn()
        gc.collect()
        gc.disable()
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            assert before == torch.cuda.memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - before
            del out
        finally:
            gc.enable()
        return rise

    rise = peak_of(lambda: step(layer.forward_recompute))
    rise_cached = peak_of(lambda: step(layer.forward))
    print(f"peak rise: recompute {rise}, cached {rise_cached} bytes")
    assert rise < edge_bytes and rise_cached >= 3 * edge_bytes


@pytest.mark.parametrize("stable", [False, True])
def test_empty_batch_writes_nothing(gpu, stable):
    """No edges: nothing launched, prefills bit-unchanged, 1 returned."""
    g = R.empty_graph()
    assert g.edges == 0 and g.batch == 7
    dev, st = gpu["dev"], gpu[stable, False]
    rng = np.random.default_rng(34000)
    heads, f = 4, 8
    coff = _up32(dev, g.column_offset)
    roff = _up32(dev, np.zeros(g.v_src + 1, dtype=np.uint32))
    idx = _up32(dev, np.zeros(4, dtype=np.uint32))
    x = Inp(dev, rng.normal(size=(g.v_src, f)))
    x16 = Inp16(dev, np.zeros((g.v_src, f), dtype=np.uint16))
    lo = g.src_start
    for entry, src in ((st.gat_backward_fused, x),
                       (st.gat_backward_fused_bf16, x16)):
        outs = [Buf(dev, s, rng.normal(size=s) + 1)
                for s in ((g.v_src, f), (g.v_src, heads), (g.batch, heads))]
        assert entry(src.ptr, x.ptr, x.ptr, *(o.ptr for o in outs), x.ptr,
                     x.ptr, SLOPE, idx.data_ptr(), coff.data_ptr(),
                     roff.data_ptr(), idx.data_ptr(), lo, lo + g.v_src, lo,
                     lo + g.batch, 0, f, heads) == 1
        for o in outs:
            o.assert_untouched("fused backward, no edges")
