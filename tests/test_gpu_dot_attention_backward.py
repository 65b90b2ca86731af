"""The dot-product attention backward that recomputes the weights (marked
gpu): Stream.dot_attention_forward_fused_stats[_bf16] and
Stream.dot_attention_backward_fused[_bf16] against the float64 chain of
DotAttentionLayer.backward (edge dot, softmax, softmax backward, four heads
gathers) on the graph of test_gpu_gat_backward_fused.py (split and unsplit
vertices on both sides), and DotAttentionLayer.forward_recompute /
gat.attend_dot(recompute=True) under autograd.  Inputs are uniform in (-1, 1),
scale = C ** -0.5; both softmax modes share the float64 reference (scores far
from overflow).

Bounds, from the inputs and the reference only:
  grad_q, grad_k, grad_v   RTOL*|ref| + 1e-4*mag + ATOL, the rule of
             test_gpu_gatv2_backward_fused.py (mag = the gather's sum of
             absolute terms plus |prefill|); the expm1(2*delta) term was not
             needed.
  M, S       delta[d, k] of test_gpu_dot_attention.py's dot_ref bounds a
             score's error.  M is one of the fp32 scores: |M - max score| <=
             delta.  A term exp(score - M) moves by a factor within
             exp(+-2 delta), and 2e-4 of S covers the fp32 exp, the sum and a
             split destination's merge (test_gpu_gatv2_backward_fused.py's).
"""
import functools
import gc
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402
from test_gpu_dot_attention import (_layer, dot_ref,  # noqa: E402
                                    torch_dot_reference)
from test_gpu_gat_backward_fused import FAST, GENERAL, _graph  # noqa: E402
from test_gpu_gat_bf16 import Inp16, round_bf16, widen  # noqa: E402
from test_gpu_gat_heads import (ATOL, RTOL, Buf, Inp, _assert_bits,  # noqa: E402
                                _assert_bound, _assert_close, _up32)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "NTS_DOT_BWD_CHILD"    # set in the child of the last test
NAMES = ("grad_q", "grad_k", "grad_v")


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
    """Inputs, non-zero prefills and the float64 backward (prefill included)
    with its mags; rows rounded to bf16 first when bf16.  Read-only."""
    g = _graph()
    f = heads * c_per
    rng = np.random.default_rng([38000, heads, c_per])
    q = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    k, v = (rng.uniform(-1, 1, (g.v_src, f)).astype(np.float32) for _ in "kv")
    if bf16:
        q, k, v = (widen(round_bf16(a)) for a in (q, k, v))
    gy = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    scale = float(np.float32(c_per ** -0.5))
    pre = [(rng.normal(size=a.shape) + 3).astype(np.float32) for a in (q, k, v)]
    q64, k64, v64, gy64 = (a.astype(np.float64) for a in (q, k, v, gy))
    csc = (g.column_offset, g.row_indices, g.src_start)
    csr = (g.row_offset, g.column_indices, g.src_start)
    perm, _ = R.csc_to_csr(g.row_indices)
    score = scale * H.edge_dot(*csc, q64, k64, heads)[0]
    alpha = R.softmax_forward(g.column_offset, score)
    galpha, _ = H.edge_dot(*csc, gy64, v64, heads)
    gscore, _ = R.softmax_backward(g.column_offset, galpha, alpha)
    zq, zk = np.zeros(q.shape), np.zeros(k.shape)
    raw = (H.gather(*csc, k64, gscore, heads, zq),
           H.gather(*csr, q64, gscore[perm], heads, zk))
    ref = [p + scale * r for p, (r, _) in zip(pre, raw)]
    mags = [np.abs(p) + scale * m for p, (_, m) in zip(pre, raw)]
    gv, mv = H.gather(*csr, gy64, alpha[perm], heads, pre[2])
    return q, k, v, gy, scale, pre, ref + [gv], mags + [mv]


def _rows(dev, a, bf16, shift=0):
    return Inp16(dev, round_bf16(a), shift) if bf16 else Inp(dev, a, shift)


def _forward(gpu, st, heads, c_per, bf16, stats, shift=0):
    """(y, ms) of the stats entry, or (y, None) of the plain fused forward."""
    g, dev, f = _graph(), gpu["dev"], heads * c_per
    q, k, v, _, scale = _case(heads, c_per, bf16)[:5]
    d_q, d_k, d_v = (_rows(dev, a, bf16, shift) for a in (q, k, v))
    y = torch.zeros(g.batch, f, device=dev)
    ms = torch.full((g.batch, heads, 2), np.nan, device=dev)
    name = "dot_attention_forward_fused" + ("_stats" if stats else "") + (
        "_bf16" if bf16 else "")
    ran = getattr(st, name)(d_q.ptr, d_k.ptr, d_v.ptr, y.data_ptr(), scale,
                            gpu["topo"][0].data_ptr(),
                            gpu["topo"][1].data_ptr(), g.src_start, g.batch,
                            g.edges, f, heads,
                            *([ms.data_ptr()] if stats else []))
    assert ran == 1
    return y, ms if stats else None


def _run(gpu, st, heads, c_per, bf16, shift=0):
    """The stats forward, then the fused backward onto the case's prefills;
    shift moves q, k, v, grad_y and the three gradients that many elements."""
    g, dev = _graph(), gpu["dev"]
    q, k, v, gy, scale, pre = _case(heads, c_per, bf16)[:6]
    y, ms = _forward(gpu, st, heads, c_per, bf16, True, shift)
    d_q, d_k, d_v = (_rows(dev, a, bf16, shift) for a in (q, k, v))
    d_gy = Inp(dev, gy, shift)
    outs = [Buf(dev, p.shape, p, shift) for p in pre]
    lo = g.src_start
    ran = (st.dot_attention_backward_fused_bf16 if bf16
           else st.dot_attention_backward_fused)(
        d_q.ptr, d_k.ptr, d_v.ptr, scale, y.data_ptr(), ms.data_ptr(),
        d_gy.ptr, *(o.ptr for o in outs),
        *(t.data_ptr() for t in gpu["topo"]), lo, lo + g.v_src, lo,
        lo + g.batch, g.edges, heads * c_per, heads)
    assert ran == 1
    return [o.read(n) for o, n in zip(outs, NAMES)]


# general form: (3, 7), (1, 33) run four edges in flight, (1, 129) two,
# (1, 257) one; (8, 16) with every pointer one element off alignment
ENTRY_CASES = ([(k, c, gen, 0) for k, c in FAST for gen in (False, True)] +
               [(k, c, False, 0) for k, c in GENERAL] +
               [(1, 129, False, 0), (1, 257, False, 0), (8, 16, False, 1)])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,c_per,general,shift", ENTRY_CASES)
def test_backward_fused(gpu, heads, c_per, general, shift, stable, bf16):
    """grad_q, grad_k, grad_v onto non-zero prefills between guard bands,
    within RTOL*|ref| + 1e-4*mag + ATOL of the float64 chain; vertices without
    edges keep their prefill bit for bit; the plan reports the form and the
    lane width of the header's rule."""
    g = _graph()
    f = heads * c_per
    pow2 = c_per & (c_per - 1) == 0
    align = 256 if not shift else 2 if bf16 else 4
    plan = gpu["shim"].dot_attention_backward_fused_plan(
        f, heads, 2 if bf16 else 4, align, 4 if shift else 256, g.v_src,
        g.batch, g.edges, general)
    want = next(r for r in (4, 2, 1) if c_per % r == 0 and not (shift and r > 1))
    assert (plan["form"], plan["cols_per_lane"]) == (
        (1, want) if pow2 and not general else (2, 1)), plan
    st = gpu[stable, general]
    got = _run(gpu, st, heads, c_per, bf16, shift)
    assert st.edge_softmax_stable_last() == int(stable)
    pre, ref, mags = _case(heads, c_per, bf16)[5:]
    tag = f"K={heads} C={c_per} general={general} stable={stable} bf16={bf16}"
    idle = (g.deg == 0, g.out_deg == 0, g.out_deg == 0)
    for name, a, r, m, p, z in zip(NAMES, got, ref, mags, pre, idle):
        _assert_bound(a, r, RTOL * np.abs(r) + 1e-4 * m + ATOL,
                      f"{name} {tag}")
        _assert_bits(a[z], p[z], f"{name} {tag}, vertices without edges")


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (3, 7)])
def test_stats_forward(gpu, heads, c_per, stable):
    """y of the stats entry is the plain fused forward's bit for bit; on
    destinations with edges (M, S) match max(score) and sum exp(score - M) of
    the float64 scores within the bounds above; M == 0 in the default mode."""
    g = _graph()
    q, k, v, _, scale = _case(heads, c_per, False)[:5]
    st = gpu[stable, False]
    y, ms = _forward(gpu, st, heads, c_per, False, True)
    y0, _ = _forward(gpu, st, heads, c_per, False, False)
    tag = f"stats K={heads} C={c_per} stable={stable}"
    _assert_bits(y.cpu().numpy(), y0.cpu().numpy(), f"y {tag}")
    _, _, sc, delta = dot_ref(g.column_offset, g.row_indices, g.src_start, q,
                              k, v, heads, scale)
    live = g.deg > 0
    delta = delta[live]
    top = np.maximum.reduceat(
        sc, g.column_offset.astype(np.int64)[:-1][live], axis=0)
    m_ref = top if stable else np.zeros_like(top)
    s_ref = R.segment_sum(np.exp(sc - np.repeat(
        m_ref, g.deg[live], axis=0)), g.column_offset)[live]
    got = ms.cpu().numpy()[live]
    if stable:
        _assert_bound(got[..., 0], m_ref, delta, f"M {tag}")
    else:
        assert (got[..., 0] == 0).all(), tag
    _assert_bound(got[..., 1], s_ref, s_ref * (np.expm1(2 * delta) + 2e-4),
                  f"S {tag}")


@pytest.mark.parametrize("heads,c_per,general", [(8, 16, False), (3, 7, False),
                                                 (8, 16, True)])
def test_one_item_vertices_reproducible(gpu, heads, c_per, general):
    """A vertex that is one work item ends with a plain read-add-write: two
    launches are bit-equal on grad_q of unsplit destinations and on grad_k,
    grad_v of unsplit sources."""
    g = _graph()
    a, b = (_run(gpu, gpu[True, general], heads, c_per, False) for _ in "ab")
    one = (g.deg <= R.SPLIT, g.out_deg <= R.SPLIT, g.out_deg <= R.SPLIT)
    for name, x, y, rows in zip(NAMES, a, b, one):
        assert rows.sum() > 100
        _assert_bits(x[rows], y[rows], f"{name} twice K={heads} C={c_per}")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_attend_dot_recompute_autograd(heads, stable, bf16):
    """gat.attend_dot(..., recompute=True) with q, k and v as leaves against
    the dense-index layer in float64: y and the float32 gradients of
    DotAttentionLayer.backward at RTOL, ATOL.  A bfloat16 leaf's gradient is
    that float32 gradient rounded once to 8 significant bits: 2^-8 * |ref|
    more, the format's own precision."""
    gat, layer, q0, k0, v0, gy = _layer(heads, stable, bf16)
    leaves = [t.clone().requires_grad_(True) for t in (q0, k0, v0)]
    y = gat.attend_dot(*leaves, layer, recompute=True)
    y.backward(gy)
    refs = [t.double().requires_grad_(True) for t in (q0, k0, v0)]
    y_ref = torch_dot_reference(*refs, layer.dst_of_edge, layer.src_of_edge,
                                layer.v, heads, (32 // heads) ** -0.5)
    y_ref.backward(gy.double())
    tag = f"K={heads} stable={stable} bf16={bf16}"
    _assert_close(y, y_ref, f"recompute y {tag}")
    _, saved = layer.forward_recompute(q0, k0, v0)
    for name, leaf, g32, r in zip("qkv", leaves, layer.backward(gy, saved),
                                  refs):
        assert leaf.grad.dtype == leaf.dtype and g32.dtype == torch.float32
        _assert_close(g32, r.grad, f"recompute backward grad_{name} {tag}")
        err = (leaf.grad.double() - r.grad).abs()
        bound = (RTOL + (2.0 ** -8 if bf16 else 0)) * r.grad.abs() + ATOL
        assert bool((err <= bound).all()), (
            f"recompute grad_{name} {tag}: worst "
            f"{float((err / bound).max()):.3e} of the bound")


def test_attend_dot_recompute_arguments():
    """recompute=True with dropout raises before a launch; the `saved` keys;
    y changed in place raises in the backward."""
    gat, layer, q, k, v, _ = _layer(4)
    with pytest.raises(ValueError):
        gat.attend_dot(q, k, v, layer, None, 0.5, recompute=True)
    assert "recompute" not in layer.forward(q, k, v)[1]
    _, saved = layer.forward_recompute(q, k, v)
    assert sorted(saved) == ["k", "ms", "q", "recompute", "scale", "v", "y"]
    y = gat.attend_dot(q.clone().requires_grad_(True), k, v, layer,
                       recompute=True)
    with pytest.raises(RuntimeError):        # D = grad_y . y needs y intact
        y.add_(1).sum().backward()


def test_recompute_step_allocates_nothing_edge_sized():
    """K = 8, C = 4: forward_recompute + backward raise torch's peak by less
    than one [E, K] float32 array, the cached pair by at least three.  What a
    step returns or must keep is y, ms and three row gradients, 4*f*4 + 2*K*4
    = 576 bytes per vertex, against 32 per edge of one [E, K] array: the
    property can hold only past 18 edges per vertex (_layer_chunk has 17.7),
    hence 1200 vertices with 40000 edges and the self loops."""
    from neutronstarlite_amd import gat, graph as G
    dev, n = torch.device("cuda:0"), 1200
    edges = G.rmat_edges(n, 40000, seed=14)
    w = G.norm_weights(edges[:, 0], edges[:, 1], *G.degrees(edges, n))
    ch = G.build_chunks(edges, w, np.array([0, n], dtype=np.uint32), 0)[0]
    layer = gat.DotAttentionLayer(ch, n, dev, heads=8)
    q, k, v, gy = (torch.rand(n, 32, device=dev) * 2 - 1 for _ in range(4))
    edge_bytes = layer.E * 8 * 4
    assert layer.E > 18 * n

    def step(forward):
        y, saved = forward(q, k, v)
        return layer.backward(gy, saved)

    def peak_of(fn):      # the pattern of test_gpu_gat_backward_fused.py
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
    rng = np.random.default_rng(39000)
    heads, f = 4, 8
    coff = _up32(dev, g.column_offset)
    roff = _up32(dev, np.zeros(g.v_src + 1, dtype=np.uint32))
    idx = _up32(dev, np.zeros(4, dtype=np.uint32))
    x = Inp(dev, rng.normal(size=(g.v_src, f)))
    x16 = Inp16(dev, np.zeros((g.v_src, f), dtype=np.uint16))
    lo = g.src_start
    for entry, src in ((st.dot_attention_backward_fused, x),
                       (st.dot_attention_backward_fused_bf16, x16)):
        outs = [Buf(dev, s, rng.normal(size=s) + 1)
                for s in ((g.batch, f), (g.v_src, f), (g.v_src, f))]
        assert entry(src.ptr, src.ptr, src.ptr, 0.5, x.ptr, x.ptr, x.ptr,
                     *(o.ptr for o in outs), idx.data_ptr(), coff.data_ptr(),
                     roff.data_ptr(), idx.data_ptr(), lo, lo + g.v_src, lo,
                     lo + g.batch, 0, f, heads) == 1
        for o in outs:
            o.assert_untouched("fused dot-product backward, no edges")


# sized as the child of test_gpu_gatv2_backward_fused.py: a few seconds of
# work, the rest for a cold import of torch on a fresh machine
CHILD_TIMEOUT = 30


@pytest.mark.skipif(CHILD in os.environ, reason="this is the child")
def test_grid_stride_and_split_in_a_fresh_child():
    """NTS_SPLIT and NTS_MAX_BLOCKS latch per process: test_backward_fused
    again in one fresh child at a split of 8 (most vertices on both sides are
    several work items that merge by atomics) under a cap of one workgroup
    (every lane group walks many items).  Last in the file: nothing follows a
    child that died."""
    env = {k: v for k, v in os.environ.items() if not k.startswith("NTS_")}
    env.update({"NTS_SPLIT": "8", "NTS_MAX_BLOCKS": "1", CHILD: "1"})
    t0 = time.time()
    p = subprocess.run(
        [sys.executable, "-m", "pytest", "-q", "-x", "-m", "gpu",
         os.path.abspath(__file__), "-k", "test_backward_fused"],
        cwd=REPO, env=env, capture_output=True, text=True,
        timeout=CHILD_TIMEOUT)
    print(f"child: {time.time() - t0:.1f} s, exit {p.returncode}")
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-2000:]
