"""The GATv2 training backward that recomputes the attention weights (marked
gpu): Stream.gatv2_forward_fused_stats[_bf16] and
Stream.gatv2_backward_fused[_bf16] against the float64 chain of
tests/gatv2_ref.py on the graph of test_gpu_gat_backward_fused.py (split and
unsplit vertices on both sides), and GATv2Layer.forward_recompute /
gat.attend_v2(recompute=True) under autograd.  Inputs are uniform in (-1, 1);
both softmax modes share the float64 reference (scores far from overflow).

Bounds, from the inputs and the reference only:
  grad_x_l, grad_x_r   1e-4*|ref| + 1e-4*mag + 2e-5: the signed-sum rule of
             test_gpu_gatv2.py plus the layer ATOL of test_gpu_gat_heads.py
  grad_att   ((E + 2)*2^-24 + 1e-4)*mag_att: an fp32 sum of E terms in any
             order (test_gpu_gatv2.py), and 1e-4 for each term's fp32 gs
  M, S       delta[d, k] = max over d's edges of (C + 2)*2^-24*mag_score is
             the score bound of test_gpu_gatv2_fused.py.  M is one of the
             fp32 scores: |M - max score| <= delta.  A term exp(score - M)
             moves by a factor within exp(+-2 delta), and 2e-4 of S covers the
             fp32 exp, the sum and a split destination's merge (that file's).
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
import gatv2_ref as V  # noqa: E402
from test_gpu_gat_backward_fused import FAST, GENERAL, _graph  # noqa: E402
from test_gpu_gat_bf16 import Inp16, round_bf16, widen  # noqa: E402
from test_gpu_gat_heads import (ATOL, RTOL, Buf, Inp, _assert_bits,  # noqa: E402
                                _assert_bound, _assert_close, _layer_chunk,
                                _up32)
from test_gpu_gatv2 import (SLOPE, _layer_inputs,  # noqa: E402
                            torch_gatv2_reference)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = "NTS_GATV2_BWD_CHILD"    # set in the child of the last test
NAMES = ("grad_x_l", "grad_x_r", "grad_att")


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    env = {"dev": dev, "shim": shim}
    for stable in (False, True):
        for general in (False, True):
            st = env[stable, general] = shim.Stream.wrap_torch_current()
            st.edge_softmax_stable(int(stable))
            st.heads_dbg_general(int(general))
    yield env
    for key in [k for k in env if isinstance(k, tuple)]:
        env[key].destroy()


def _topo(dev, g):
    return [_up32(dev, a) for a in (g.row_indices, g.column_offset,
                                    g.row_offset, g.column_indices)]


@functools.lru_cache(maxsize=None)
def _case(heads, c_per, bf16):
    """Inputs, non-zero prefills, the float64 forward (score, its mag) and
    backward (prefill included) with its mags; rows rounded to bf16 first
    when bf16.  Read-only."""
    g = _graph()
    f = heads * c_per
    rng = np.random.default_rng([35000, heads, c_per])
    x_l = rng.uniform(-1, 1, (g.v_src, f)).astype(np.float32)
    x_r = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    if bf16:
        x_l, x_r = widen(round_bf16(x_l)), widen(round_bf16(x_r))
    att = rng.uniform(-1, 1, (heads, c_per)).astype(np.float32)
    gy = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    pre = [(rng.normal(size=s) + 3).astype(np.float32)
           for s in ((g.v_src, f), (g.batch, f), (heads, c_per))]
    _, _, sc, alpha = V.layer_forward(g, x_l, x_r, att, heads, SLOPE)
    _, mag_sc = V.score(g.column_offset, g.row_indices, g.src_start, x_r, x_l,
                        att, SLOPE, heads)
    grads, mags = V.layer_backward(g, x_l, x_r, att, alpha, gy, heads, SLOPE)
    ref = [p + r for p, r in zip(pre, grads)]
    return x_l, x_r, att, gy, pre, ref, mags, sc, mag_sc


def _rows(dev, a, bf16, shift=0):
    return Inp16(dev, round_bf16(a), shift) if bf16 else Inp(dev, a, shift)


def _forward(gpu, st, g, topo, x_l, x_r, att, heads, bf16, stats, shift=0):
    """(y, ms) of the stats entry, or (y, None) of the plain fused forward."""
    dev, f = gpu["dev"], x_l.shape[1]
    d_l, d_r, d_a = _rows(dev, x_l, bf16, shift), _rows(dev, x_r, bf16, shift), \
        Inp(dev, att)
    y = torch.zeros(g.batch, f, device=dev)
    ms = torch.full((g.batch, heads, 2), np.nan, device=dev)
    rows, coff = topo[0].data_ptr(), topo[1].data_ptr()
    name = "gatv2_forward_fused" + ("_stats" if stats else "") + (
        "_bf16" if bf16 else "")
    ran = getattr(st, name)(d_l.ptr, d_r.ptr, y.data_ptr(), d_a.ptr, SLOPE,
                            rows, coff, g.src_start, g.batch, g.edges, f,
                            heads, *([ms.data_ptr()] if stats else []))
    assert ran == 1
    return y, ms if stats else None


def _run(gpu, st, heads, c_per, bf16, shift=0):
    """The stats forward, then the fused backward onto the case's prefills;
    shift moves x_l, x_r, grad_y and grad_x_l that many elements."""
    g, dev = _graph(), gpu["dev"]
    x_l, x_r, att, gy, pre, _, _, _, _ = _case(heads, c_per, bf16)
    topo = _topo(dev, g)
    y, ms = _forward(gpu, st, g, topo, x_l, x_r, att, heads, bf16, True, shift)
    d_l, d_r = _rows(dev, x_l, bf16, shift), _rows(dev, x_r, bf16, shift)
    d_a, d_gy = Inp(dev, att), Inp(dev, gy, shift)
    outs = [Buf(dev, p.shape, p, shift if i == 0 else 0)
            for i, p in enumerate(pre)]
    lo = g.src_start
    ran = (st.gatv2_backward_fused_bf16 if bf16 else st.gatv2_backward_fused)(
        d_l.ptr, d_r.ptr, d_a.ptr, y.data_ptr(), ms.data_ptr(), d_gy.ptr,
        *(o.ptr for o in outs), SLOPE, *(t.data_ptr() for t in topo), lo,
        lo + g.v_src, lo, lo + g.batch, g.edges, heads * c_per, heads)
    assert ran == 1
    return [o.read(n) for o, n in zip(outs, NAMES)]


ENTRY_CASES = ([(k, c, gen, 0) for k, c in FAST for gen in (False, True)] +
               [(k, c, False, 0) for k, c in GENERAL] +
               [(2, 128, True, 0), (8, 16, False, 1)])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,c_per,general,shift", ENTRY_CASES)
def test_backward_fused(gpu, heads, c_per, general, shift, stable, bf16):
    """grad_x_l, grad_x_r, grad_att onto non-zero prefills between guard
    bands, within the bounds above of the float64 chain; vertices without
    edges keep their prefill bit for bit; the plan reports the form and the
    lane width of the header's rule."""
    g = _graph()
    f = heads * c_per
    pow2 = c_per & (c_per - 1) == 0
    align = 256 if not shift else 2 if bf16 else 4
    plan = gpu["shim"].gatv2_backward_fused_plan(
        f, heads, 2 if bf16 else 4, align, 4 if shift else 256, g.v_src,
        g.batch, g.edges, general)
    want = next(r for r in (4, 2, 1) if c_per % r == 0 and not (shift and r > 1))
    assert (plan["form"], plan["cols_per_lane"]) == (
        (1, want) if pow2 and not general else (2, 1)), plan
    st = gpu[stable, general]
    got = _run(gpu, st, heads, c_per, bf16, shift)
    assert st.edge_softmax_stable_last() == int(stable)
    _, _, _, _, pre, ref, mags, _, _ = _case(heads, c_per, bf16)
    tag = f"K={heads} C={c_per} general={general} stable={stable} bf16={bf16}"
    for name, a, r, m, p, z in zip(NAMES[:2], got, ref, mags, pre,
                                   (g.out_deg == 0, g.deg == 0)):
        _assert_bound(a, r, RTOL * np.abs(r) + 1e-4 * m + ATOL,
                      f"{name} {tag}")
        _assert_bits(a[z], p[z], f"{name} {tag}, vertices without edges")
    _assert_bound(got[2], ref[2],
                  ((g.edges + 2) * 2.0 ** -24 + 1e-4) * mags[2],
                  f"grad_att {tag}")


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (3, 7)])
def test_stats_forward(gpu, heads, c_per, stable):
    """y of the stats entry is the plain fused forward's bit for bit; on
    destinations with edges (M, S) match max(score) and sum exp(score - M) of
    the float64 scores within the bounds above; M == 0 in the default mode."""
    g = _graph()
    x_l, x_r, att, _, _, _, _, sc, mag_sc = _case(heads, c_per, False)
    st, topo = gpu[stable, False], _topo(gpu["dev"], g)
    y, ms = _forward(gpu, st, g, topo, x_l, x_r, att, heads, False, True)
    y0, _ = _forward(gpu, st, g, topo, x_l, x_r, att, heads, False, False)
    tag = f"stats K={heads} C={c_per} stable={stable}"
    _assert_bits(y.cpu().numpy(), y0.cpu().numpy(), f"y {tag}")
    live = g.deg > 0
    first = g.column_offset.astype(np.int64)[:-1][live]
    top = np.maximum.reduceat(sc, first, axis=0)
    delta = (c_per + 2) * 2.0 ** -24 * np.maximum.reduceat(mag_sc, first,
                                                           axis=0)
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


@pytest.mark.parametrize("heads,c_per,general", [
    (8, 16, False), (8, 16, True), (3, 7, False), (2, 128, False)])
def test_grad_att_exact_on_a_grid(gpu, heads, c_per, general):
    """No workgroup partial lost or doubled.  att = 0 makes every score 0, so
    with in-degrees 1, 2, 4 and 8 alpha is exactly 1/deg, while grad_att does
    not depend on att.  Rows that are multiples of 2^-2 in [-1, 1], grad_y
    integers in [-1, 1], slope 0.5 and y, ms = (0, deg) from the host make gs
    a multiple of 2^-8 and every term gs*lrelu(t) one of 2^-11; their
    absolute sum stays below 2^13, so fp32 adds them exactly in any order and
    grad_att through registers, LDS and atomics is the float64 reference bit
    for bit.  grad_x_r = att * (...) leaves its prefill untouched."""
    f = heads * c_per
    rng = np.random.default_rng([36000, heads, c_per])
    g = R.build_graph(2 ** rng.integers(0, 4, 600), 500, 300, 36001)
    g.row_offset = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    g.column_indices = (g.src_start + g.dst_of_edge[
        R.csc_to_csr(g.row_indices)[0]]).astype(np.uint32)
    x_l = (rng.integers(-4, 5, (g.v_src, f)) / 4.0).astype(np.float32)
    x_r = (rng.integers(-4, 5, (g.batch, f)) / 4.0).astype(np.float32)
    gy = rng.integers(-1, 2, (g.batch, f)).astype(np.float32)
    att = np.zeros((heads, c_per), dtype=np.float32)
    pre = [rng.integers(1, 9, s).astype(np.float32)
           for s in ((g.v_src, f), (g.batch, f), (heads, c_per))]
    y, _, _, alpha = V.layer_forward(g, x_l, x_r, att, heads, 0.5)
    (_, _, ref_att), (_, _, mag_att) = V.layer_backward(
        g, x_l, x_r, att, alpha, gy, heads, 0.5)
    ref_att = ref_att + pre[2]
    assert (mag_att + pre[2]).max() < 2.0 ** 13
    assert (ref_att.astype(np.float32) == ref_att).all()
    ms = np.stack([np.zeros((g.batch, heads)),
                   np.repeat(g.deg[:, None], heads, axis=1)], axis=2)
    dev, st = gpu["dev"], gpu[False, general]
    ins = [Inp(dev, a) for a in (x_l, x_r, att, y, ms, gy)]
    outs = [Buf(dev, p.shape, p) for p in pre]
    lo = g.src_start
    assert st.gatv2_backward_fused(
        *(i.ptr for i in ins), *(o.ptr for o in outs), 0.5,
        *(t.data_ptr() for t in _topo(dev, g)), lo, lo + g.v_src, lo,
        lo + g.batch, g.edges, f, heads) == 1
    name = f"grid K={heads} C={c_per} general={general}"
    _assert_bits(outs[2].read(name), ref_att.astype(np.float32),
                 name + " grad_att")
    outs[1].assert_untouched(name + " grad_x_r")


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_attend_v2_recompute_autograd(heads, stable, bf16):
    """gat.attend_v2(..., recompute=True) with x_l, x_r and att as leaves
    against the dense-index layer in float64 at RTOL, ATOL.  A bfloat16 row
    gradient is the float32 one rounded once: 2^-8 * |ref| more."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    xl0, xr0, att0, gy = _layer_inputs(heads, 32 // heads, dev)
    if bf16:
        xl0, xr0 = xl0.to(torch.bfloat16), xr0.to(torch.bfloat16)
    layer = gat.GATv2Layer(ch, v, dev, heads=heads, stable=stable)
    x_l, x_r, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    y = gat.attend_v2(x_l, x_r, att, layer, SLOPE, recompute=True)
    y.backward(gy)
    assert x_l.grad.dtype == x_l.dtype and x_r.grad.dtype == x_r.dtype
    lr, rr, ar = (t.double().requires_grad_(True) for t in (xl0, xr0, att0))
    y_ref, _ = torch_gatv2_reference(lr, rr, ar, layer.dst_of_edge,
                                     layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    tag = f"K={heads} stable={stable} bf16={bf16}"
    _assert_close(y, y_ref, f"recompute y {tag}")
    _assert_close(att.grad, ar.grad, f"recompute grad att {tag}")
    for name, a, r in (("x_l", x_l.grad, lr.grad), ("x_r", x_r.grad, rr.grad)):
        err = (a.double() - r).abs()
        bound = (RTOL + (2.0 ** -8 if bf16 else 0)) * r.abs() + ATOL
        assert bool((err <= bound).all()), (
            f"recompute grad {name} {tag}: worst "
            f"{float((err / bound).max()):.3e} of the bound")


def test_attend_v2_recompute_arguments():
    """recompute=True with dropout raises before a launch; the `saved` keys;
    y changed in place raises in the backward."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    x_l, x_r, att, _ = _layer_inputs(4, 8, dev)
    layer = gat.GATv2Layer(ch, v, dev, heads=4)
    with pytest.raises(ValueError):
        gat.attend_v2(x_l, x_r, att, layer, SLOPE, 0.5, recompute=True)
    assert "recompute" not in layer.forward(x_l, x_r, att, SLOPE)[1]
    _, saved = layer.forward_recompute(x_l, x_r, att, SLOPE)
    assert sorted(saved) == ["att", "ms", "recompute", "x_l", "x_r", "y"]
    y = gat.attend_v2(x_l.clone().requires_grad_(True), x_r, att, layer, SLOPE,
                      recompute=True)
    with pytest.raises(RuntimeError):        # D = grad_y . y needs y intact
        y.add_(1).sum().backward()


def test_recompute_step_allocates_nothing_edge_sized():
    """K = 8, C = 4: forward_recompute + backward raise torch's peak by less
    than one [E, K] float32 array, the cached pair by at least three."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    x_l, x_r, att, gy = _layer_inputs(8, 4, dev)
    layer = gat.GATv2Layer(ch, v, dev, heads=8)
    edge_bytes = ch.edge_size * 8 * 4

    def step(forward):
        y, saved = forward(x_l, x_r, att, SLOPE)
        return layer.backward(gy, saved, SLOPE)

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
    rng = np.random.default_rng(37000)
    heads, f = 4, 8
    coff = _up32(dev, g.column_offset)
    roff = _up32(dev, np.zeros(g.v_src + 1, dtype=np.uint32))
    idx = _up32(dev, np.zeros(4, dtype=np.uint32))
    x = Inp(dev, rng.normal(size=(g.v_src, f)))
    x16 = Inp16(dev, np.zeros((g.v_src, f), dtype=np.uint16))
    lo = g.src_start
    for entry, src in ((st.gatv2_backward_fused, x),
                       (st.gatv2_backward_fused_bf16, x16)):
        outs = [Buf(dev, s, rng.normal(size=s) + 1)
                for s in ((g.v_src, f), (g.batch, f), (heads, f // heads))]
        assert entry(src.ptr, src.ptr, x.ptr, x.ptr, x.ptr, x.ptr,
                     *(o.ptr for o in outs), SLOPE, idx.data_ptr(),
                     coff.data_ptr(), roff.data_ptr(), idx.data_ptr(), lo,
                     lo + g.v_src, lo, lo + g.batch, 0, f, heads) == 1
        for o in outs:
            o.assert_untouched("fused GATv2 backward, no edges")


# the child takes 2.7 s on an MI355X with torch warm in the page cache (48
# cases, import, context creation and the float64 references included); the
# rest allows for a cold import of torch on a fresh machine, as the 30 s of
# test_gpu_grid_cap.py do
CHILD_TIMEOUT = 30


@pytest.mark.skipif(CHILD in os.environ, reason="this is the child")
def test_grid_stride_and_split_in_a_fresh_child():
    """NTS_SPLIT and NTS_MAX_BLOCKS latch per process: test_backward_fused
    again in one fresh child at a split of 8 (most vertices on both sides are
    several work items that merge by atomics) under a cap of one workgroup
    (every lane group walks many items, grad_att's LDS meeting sees them all).
    Last in the file: nothing follows a child that died."""
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
