"""The fused GAT inference forward on the GPU (marked gpu):
Stream.gat_forward_fused[_bf16] against the float64 references of
tests/heads_ref.py and tests/softmax_stable_ref.py and against today's
two-entry chain (edge_attention_forward_heads, then
gather_by_dst_from_src_heads), and GATLayer.infer / gat.attend under
torch.no_grad() against GATLayer.forward.

The kernel cases run on edge_ref.edge_case_graph (about 22k edges; degrees on
both sides of 64 and 256 and their multiples, a degree-5000 hub, zero degrees
at both ends and in the middle, src_start = 1000, a shuffled mirror map); the
split is assumed to be the default of 256.  Buffers are those of
tests/test_gpu_gat_heads.py: the output sits between guard bands that must
come back bit-unchanged and starts from random non-zero values that the
reference includes.

Bounds, none taken from what the kernels give.  The output is held to
  1e-4*|ref| + 2e-4*mag,   mag = |prefill| + sum_e |w[e] * x[e]|,
the sum of the two bounds the project holds the fused passes to one by one:
every softmax weight within 1e-4*|w| (test_gpu_gat_heads.py), which moves the
sum by at most 1e-4 * sum_e |w x| <= 1e-4*mag, and the heads gather within
1e-4*|ref| + 1e-4*mag.  In the out-of-range regimes of softmax_stable_ref the
weight term is instead the per-weight bound of test_gpu_softmax_stable.py
(1e-4*w where w >= 1e-30, else 2e-30), summed against |x|.  A destination
that is one work item is in addition bit-equal to the chain: its denominator
is reduced in the same order, a weight is the normalize pass's expression, and
an output element is one lane's fmaf chain in edge order.
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
import softmax_stable_ref as S  # noqa: E402
from test_gpu_gat_bf16 import (Inp16, alignment_of, lane_rule,  # noqa: E402
                               make_rows)
from test_gpu_gat_bf16 import GATHER_CASES as BF16_CASES  # noqa: E402
from test_gpu_gat_heads import (ATOL, GATHER_CASES, RTOL, Buf, Inp,  # noqa: E402
                                _assert_bits, _assert_bound, _attention_case,
                                _layer_chunk, _up32, torch_heads_reference)

pytestmark = pytest.mark.gpu

SLOPE = 0.2
TINY = 1e-30   # of tests/test_gpu_softmax_stable.py


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    g = R.edge_case_graph()
    mk = shim.Stream.wrap_torch_current
    env = {"dev": dev, "shim": shim,
           "auto": mk(), "general": mk(), "stable": mk(),
           "stable_general": mk(),
           "coff": _up32(dev, g.column_offset),
           "rows": _up32(dev, g.row_indices),
           "mi": _up32(dev, g.mirror_index)}
    env["general"].heads_dbg_general(1)
    env["stable"].edge_softmax_stable(1)
    env["stable_general"].edge_softmax_stable(1)
    env["stable_general"].heads_dbg_general(1)
    yield env
    for k in ("auto", "general", "stable", "stable_general"):
        env[k].destroy()


def _unsplit():
    g = R.edge_case_graph()
    one = g.deg <= R.SPLIT
    assert one.any() and (~one).any()
    return one


def _empty():
    g = R.edge_case_graph()
    empty = g.deg == 0
    assert empty.any()
    return empty


def _bound(ref, mag):
    return 1e-4 * np.abs(ref) + 2e-4 * mag


# --------------------------------------------------------------------------
# inputs and references, computed once
# --------------------------------------------------------------------------
def _scalars(heads):
    """(s_src by global source id, s_src by mirror row, s_dst, float64
    softmax (E, K)): test_attention_forward_heads' inputs, per head those of
    edge_ref.attention_inputs(seed = head)."""
    full, s_dst, _, s_ref = _attention_case(heads, False)
    mirror = _attention_case(heads, True)[0]
    return full, mirror, s_dst, s_ref


@functools.lru_cache(maxsize=None)
def _rows(heads, c_per):
    """(x uniform in [-1, 1], non-zero prefill)"""
    g = R.edge_case_graph()
    rng = np.random.default_rng([9100, heads, c_per])
    x = rng.uniform(-1, 1, (g.v_src, heads * c_per)).astype(np.float32)
    pre = (rng.normal(size=(g.batch, heads * c_per)) + 3).astype(np.float32)
    assert (pre != 0).all()
    x.setflags(write=False)
    pre.setflags(write=False)
    return x, pre


@functools.lru_cache(maxsize=None)
def _case(heads, c_per):
    g = R.edge_case_graph()
    x, pre = _rows(heads, c_per)
    s_ref = _scalars(heads)[3]
    ref, mag = H.gather(g.column_offset, g.row_indices, g.src_start, x, s_ref,
                        heads, pre)
    ref.setflags(write=False)
    mag.setflags(write=False)
    return x, pre, ref, mag


def _topo_args(gpu, with_mirror, edges=None, batch=None):
    g = R.edge_case_graph()
    return (gpu["rows"].data_ptr(),
            gpu["mi"].data_ptr() if with_mirror else None, SLOPE,
            gpu["coff"].data_ptr(), g.src_start, g.src_start + g.v_src,
            g.src_start, g.src_start + g.batch,
            g.edges if edges is None else edges,
            g.batch if batch is None else batch)


def _run_fused(gpu, st, x, pre, s_src, s_dst, with_mirror, heads, shift=0,
               name="fused", bits=None, offset=0):
    """One launch onto `pre`; with `bits` the bf16 entry on those rows."""
    dev = gpu["dev"]
    f = pre.shape[1]
    d_src, d_dst = Inp(dev, s_src), Inp(dev, s_dst)
    out = Buf(dev, pre.shape, pre, shift)
    if bits is None:
        d_x = Inp(dev, x, shift)
        entry = st.gat_forward_fused
    else:
        d_x = Inp16(dev, bits, offset)
        entry = st.gat_forward_fused_bf16
    entry(d_x.ptr, out.ptr, d_src.ptr, d_dst.ptr,
          *_topo_args(gpu, with_mirror), f, heads)
    return out.read(name)


def _run_chain(gpu, st, x, pre, s_src, s_dst, with_mirror, heads, name):
    """Today's forward: the attention entry, then the heads gather."""
    g = R.edge_case_graph()
    dev = gpu["dev"]
    f = pre.shape[1]
    d_src, d_dst, d_x = Inp(dev, s_src), Inp(dev, s_dst), Inp(dev, x)
    w, msum = Buf(dev, (g.edges, heads)), Buf(dev, (g.edges, heads))
    out = Buf(dev, pre.shape, pre)
    st.edge_attention_forward_heads(
        w.ptr, None, None, msum.ptr, d_src.ptr, d_dst.ptr,
        gpu["rows"].data_ptr(), gpu["mi"].data_ptr() if with_mirror else None,
        SLOPE, gpu["coff"].data_ptr(), g.batch, g.edges, heads)
    st.gather_by_dst_from_src_heads(
        d_x.ptr, out.ptr, w.ptr, gpu["rows"].data_ptr(),
        gpu["coff"].data_ptr(), g.src_start, g.src_start + g.v_src,
        g.src_start, g.src_start + g.batch, g.edges, g.batch, f, heads)
    return out.read(name)


def test_graph_coverage():
    R.assert_coverage(R.edge_case_graph())


# --------------------------------------------------------------------------
# 1. against the float64 reference
# --------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "general"])
@pytest.mark.parametrize("with_mirror", [True, False])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("heads,c_per", GATHER_CASES)
def test_fused_forward(gpu, heads, c_per, shift, with_mirror, form):
    """heads_ref.attention_forward followed by heads_ref.gather.  shift = 1
    moves the row and output pointers one float off, which leaves the strided
    lanes; rows without edges stay bit-unchanged."""
    assert (1, 33) in GATHER_CASES and (16, 1) in GATHER_CASES
    g = R.edge_case_graph()
    x, pre, ref, mag = _case(heads, c_per)
    full, mirror, s_dst, _ = _scalars(heads)
    name = (f"fused K={heads} C={c_per} shift={shift} mirror={with_mirror} "
            f"{form}")
    want = 1 if shift else (4 if c_per % 4 == 0 else 2 if c_per % 2 == 0 else 1)
    plan = gpu["shim"].gather_plan_heads(heads * c_per, heads,
                                         4 if shift else 256, g.batch, g.edges)
    assert plan["vector_width"] == want, plan
    st = gpu[form]
    got = _run_fused(gpu, st, x, pre, mirror if with_mirror else full, s_dst,
                     with_mirror, heads, shift, name)
    assert st.edge_softmax_stable_last() == 0
    _assert_bound(got, ref, _bound(ref, mag), name)
    _assert_bits(got[_empty()], pre[_empty()], name + ", rows without edges")


# --------------------------------------------------------------------------
# 2. bit equality with today's chain
# --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "stable"])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (4, 6), (3, 7), (1, 33)])
def test_fused_forward_equals_chain(gpu, heads, c_per, mode):
    """On the same prefill the fused entry and the two-entry chain agree bit
    for bit on every destination of at most SPLIT edges, in both softmax
    modes; split destinations merge by atomics and are held to the bound."""
    x, pre, ref, mag = _case(heads, c_per)
    _, mirror, s_dst, _ = _scalars(heads)
    name = f"fused vs chain K={heads} C={c_per} {mode}"
    st = gpu[mode]
    got = _run_fused(gpu, st, x, pre, mirror, s_dst, True, heads, name=name)
    assert st.edge_softmax_stable_last() == int(mode == "stable")
    base = _run_chain(gpu, st, x, pre, mirror, s_dst, True, heads, name)
    one = _unsplit()
    _assert_bits(got[one], base[one], name + ", unsplit destinations")
    _assert_bound(got, ref, _bound(ref, mag), name)
    _assert_bound(base, ref, _bound(ref, mag), name + " (chain)")


# --------------------------------------------------------------------------
# 3. stable mode, out-of-range scores
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stable_case(regime, heads, c_per):
    g = R.edge_case_graph()
    x, pre = _rows(heads, c_per)
    full, mirror, s_dst = S.attention_inputs(regime, g, heads)
    m_ref, s_ref = S.attention_forward(g.column_offset, g.row_indices, full,
                                       s_dst, None, SLOPE)
    ref, mag = H.gather(g.column_offset, g.row_indices, g.src_start, x, s_ref,
                        heads, pre)
    # the softmax term of the bound: test_gpu_softmax_stable's per-weight one
    wb = np.where(s_ref >= TINY, 1e-4 * s_ref, 2 * TINY)
    soft, _ = H.gather(g.column_offset, g.row_indices, g.src_start, np.abs(x),
                       wb, heads, np.zeros_like(pre))
    bound = 1e-4 * np.abs(ref) + 1e-4 * mag + soft
    return x, pre, full, mirror, s_dst, m_ref, ref, bound


@pytest.mark.parametrize("regime", S.REGIMES)
@pytest.mark.parametrize("heads,c_per", [(8, 16), (3, 7), (1, 33)])
def test_fused_forward_stable(gpu, heads, c_per, regime):
    """Scalars whose sums reach +-200, about +-1000 or 500, or are -inf on a
    strict subset of a destination's edges: the output is finite and within
    the bound, and the call is reported as stable.  masked: the weight of an
    edge with a -inf score is exactly +0.0f, so the rows behind such edges can
    take any finite value without changing a bit of an unsplit destination."""
    x, pre, full, mirror, s_dst, m_ref, ref, bound = _stable_case(
        regime, heads, c_per)
    st = gpu["stable"]
    name = f"fused stable K={heads} C={c_per} {regime}"
    got = _run_fused(gpu, st, x, pre, mirror, s_dst, True, heads, name=name)
    assert st.edge_softmax_stable_last() == 1
    _assert_bound(got, ref, bound, name)
    _assert_bits(got[_empty()], pre[_empty()], name + ", rows without edges")
    got_g = _run_fused(gpu, gpu["stable_general"], x, pre, full, s_dst, False,
                       heads, name=name + " general")
    _assert_bound(got_g, ref, bound, name + " general")
    if regime == "masked":
        g = R.edge_case_graph()
        dead_src = np.isneginf(full[g.src_start:])          # (v_src, K)
        assert dead_src.any() and np.isneginf(m_ref).any()
        x2 = x.copy()
        x2[np.repeat(dead_src, c_per, axis=1)] = 1e30
        assert (x2 != x).any()
        got2 = _run_fused(gpu, st, x2, pre, mirror, s_dst, True, heads,
                          name=name + ", other rows behind masked edges")
        one = _unsplit()
        _assert_bits(got2[one], got[one], name + ": masked edges contribute")
        _assert_bound(got2, ref, bound, name + ", other rows")


@pytest.mark.parametrize("heads,c_per", [(8, 16), (1, 33)])
def test_fused_forward_default_keeps_its_nans(gpu, heads, c_per):
    """Default mode on the `huge` regime: no max subtraction, so exp
    overflows; on unsplit destinations the non-finite positions are those of
    the chain."""
    x, pre, full, mirror, s_dst, _, _, _ = _stable_case("huge", heads, c_per)
    st = gpu["auto"]
    name = f"fused default on huge K={heads} C={c_per}"
    got = _run_fused(gpu, st, x, pre, mirror, s_dst, True, heads, name=name)
    assert st.edge_softmax_stable_last() == 0
    base = _run_chain(gpu, st, x, pre, mirror, s_dst, True, heads, name)
    one = _unsplit()
    assert not np.isfinite(base[one]).all()
    assert (np.isfinite(got[one]) == np.isfinite(base[one])).all(), name


# --------------------------------------------------------------------------
# 4. bf16 rows
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _bf16_case(heads, c_per):
    g = R.edge_case_graph()
    rng = np.random.default_rng([9200, heads, c_per])
    bits, x = make_rows((g.v_src, heads * c_per), rng)
    _, pre = _rows(heads, c_per)
    ref, mag = H.gather(g.column_offset, g.row_indices, g.src_start, x,
                        _scalars(heads)[3], heads, pre)
    return bits, x, pre, ref, mag


_fp32_twin = {}


def _twin(gpu, heads, c_per, mode):
    """The fp32 entry on the widened rows, once per case and mode."""
    key = (heads, c_per, mode)
    if key not in _fp32_twin:
        _, x, pre, _, _ = _bf16_case(heads, c_per)
        _, mirror, s_dst, _ = _scalars(heads)
        _fp32_twin[key] = _run_fused(gpu, gpu[mode], x, pre, mirror, s_dst,
                                     True, heads, name="fp32 twin")
    return _fp32_twin[key]


@pytest.mark.parametrize("mode", ["auto", "stable"])
@pytest.mark.parametrize("offset", [0, 1, 2, 4])
@pytest.mark.parametrize("heads,c_per", BF16_CASES)
def test_fused_forward_bf16(gpu, heads, c_per, offset, mode):
    """bf16 rows `offset` elements off their alignment (lanes of 8 / 4 / 2 / 1
    elements by C and the alignment): within the bound, and on unsplit
    destinations bit-equal to the fp32 entry on the widened rows."""
    g = R.edge_case_graph()
    bits, x, pre, ref, mag = _bf16_case(heads, c_per)
    _, mirror, s_dst, _ = _scalars(heads)
    name = f"fused bf16 K={heads} C={c_per} offset={offset} {mode}"
    align = alignment_of(offset)
    want = lane_rule(c_per, align)
    plan = gpu["shim"].gather_plan_heads_bf16(heads * c_per, heads, align,
                                              g.batch, g.edges)
    assert plan["vector_width"] == want, plan
    if offset == 0:
        assert want == {16: 8, 4: 4, 6: 2, 64: 8}.get(c_per, 1)
    got = _run_fused(gpu, gpu[mode], None, pre, mirror, s_dst, True, heads,
                     name=name, bits=bits, offset=offset)
    _assert_bound(got, ref, _bound(ref, mag), name)
    _assert_bits(got[_empty()], pre[_empty()], name + ", rows without edges")
    one = _unsplit()
    _assert_bits(got[one], _twin(gpu, heads, c_per, mode)[one],
                 name + ", unsplit destinations vs fp32 entry")


# --------------------------------------------------------------------------
# 5. nothing to do
# --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["auto", "stable"])
def test_empty_batch_writes_nothing(gpu, mode):
    """edge_ref.empty_graph(): batch_size = 0, and a batch whose destinations
    all have degree 0 (edges = 0), leave the prefilled output bit-unchanged."""
    g = R.empty_graph()
    assert g.edges == 0 and g.batch == 7
    dev, st = gpu["dev"], gpu[mode]
    rng = np.random.default_rng(9300)
    heads, f = 4, 8
    coff = _up32(dev, g.column_offset)
    rows = _up32(dev, np.zeros(4, dtype=np.uint32))
    x = Inp(dev, rng.normal(size=(g.v_src, f)))
    x16 = Inp16(dev, np.zeros((g.v_src, f), dtype=np.uint16))
    s = Inp(dev, rng.normal(size=(g.src_start + g.v_src, heads)))
    for batch in (0, g.batch):
        for entry, src in ((st.gat_forward_fused, x),
                           (st.gat_forward_fused_bf16, x16)):
            out = Buf(dev, (g.batch, f), rng.normal(size=(g.batch, f)) + 1)
            entry(src.ptr, out.ptr, s.ptr, s.ptr, rows.data_ptr(), None,
                  SLOPE, coff.data_ptr(), g.src_start, g.src_start + g.v_src,
                  g.src_start, g.src_start + g.batch, 0, batch, f, heads)
            out.assert_untouched(f"fused forward, batch={batch}")
            assert st.edge_softmax_stable_last() == int(mode == "stable")
    with pytest.raises(ValueError):          # checked by the binding
        st.gat_forward_fused(0, 0, 0, 0, 0, None, SLOPE, 0, 0, 1, 0, 1, 1, 1,
                             32, 5)


# --------------------------------------------------------------------------
# the layer
# --------------------------------------------------------------------------
def _layer_one():
    """Unsplit destinations of the layer tests' graph (bool [V])."""
    v, ch = _layer_chunk()
    deg = np.diff(ch.column_offset.astype(np.int64))
    assert ch.edge_size == 21200 and deg.max() == 1035
    one = deg <= R.SPLIT
    assert int((~one).sum()) == 12 and int(one.sum()) == 1188
    return one


def _layer_inputs(heads, c_per, dev, bf16):
    """(h, s_src, s_dst, a_src, a_dst, h as float32): rows uniform in
    [-1, 1] (rounded to bf16 first when bf16), scalars the projections of the
    float32 rows; [V] scalars for one head."""
    v, _ = _layer_chunk()
    rng = np.random.default_rng([9400, heads, c_per])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    h32 = up(rng.uniform(-1, 1, size=(v, heads * c_per)))
    h = h32.to(torch.bfloat16) if bf16 else h32
    h32 = h.float()
    a_src, a_dst = (up(rng.uniform(-1, 1, size=(heads, c_per)))
                    for _ in range(2))
    h3 = h32.view(v, heads, c_per)
    s_src, s_dst = ((h3 * a).sum(-1).contiguous() for a in (a_src, a_dst))
    if heads == 1:
        s_src, s_dst = s_src[:, 0].contiguous(), s_dst[:, 0].contiguous()
    return h, s_src, s_dst, a_src, a_dst, h32


def _eq_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32),
                       b.contiguous().view(torch.int32))


def _assert_close(got, ref, name):
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = ref.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    bound = RTOL * np.abs(ref) + ATOL
    print(f"{name}: worst {float((err / bound).max()):.3e} of the tolerance")
    assert not (err > bound).any(), f"{name}: worst {err.max():.3e}"


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_layer_infer(heads, stable, bf16):
    """GATLayer.infer against forward(...)[0]: bit-equal on unsplit
    destinations; against the float64 dense-index layer at the layer tests'
    tolerance (RTOL, ATOL = 1e-4, 2e-5) everywhere."""
    from neutronstarlite_amd import gat
    assert (RTOL, ATOL) == (1e-4, 2e-5)
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    c_per = 32 // heads
    h, s_src, s_dst, a_src, a_dst, h32 = _layer_inputs(heads, c_per, dev, bf16)
    layer = gat.GATLayer(ch, v, dev, heads=heads, stable=stable)
    y = layer.infer(h, s_src, s_dst, SLOPE)
    assert isinstance(y, torch.Tensor) and y.dtype == torch.float32
    assert y.shape == (v, 32)
    assert layer.stream.edge_softmax_stable_last() == int(stable)
    y_fwd = layer.forward(h, s_src, s_dst, SLOPE)[0]
    torch.cuda.synchronize()
    one = torch.from_numpy(_layer_one()).to(dev)
    tag = f"infer K={heads} stable={stable} bf16={bf16}"
    assert _eq_bits(y[one], y_fwd[one]), tag + ": unsplit destinations"
    y_ref = torch_heads_reference(h32.double(), a_src.double(), a_dst.double(),
                                  layer.dst_of_edge, layer.src_of_edge, v,
                                  heads, SLOPE)
    _assert_close(y, y_ref, tag)


def test_attend_routes_to_infer_without_grad():
    """gat.attend under torch.no_grad() with dropout == 0 is layer.infer;
    with grad enabled, or with dropout, it takes the training path."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads = 4
    h, s_src, s_dst, _, _, _ = _layer_inputs(heads, 8, dev, False)
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    calls = []
    infer = layer.infer

    def counted(*a, **kw):
        calls.append(1)
        return infer(*a, **kw)

    layer.infer = counted
    one = torch.from_numpy(_layer_one()).to(dev)
    with torch.no_grad():
        y = gat.attend(h, s_src, s_dst, layer, SLOPE)
        assert len(calls) == 1
        y_drop = gat.attend(h, s_src, s_dst, layer, SLOPE, dropout=0.5, seed=3)
        assert len(calls) == 1 and y_drop.shape == y.shape
    assert not y.requires_grad
    assert _eq_bits(y[one], infer(h, s_src, s_dst, SLOPE)[one])
    hg = h.clone().requires_grad_(True)
    y_train = gat.attend(hg, s_src, s_dst, layer, SLOPE)
    assert len(calls) == 1 and y_train.requires_grad
    y_plain = gat.attend(h, s_src, s_dst, layer, SLOPE)   # grad mode, no leaf
    assert len(calls) == 1
    assert _eq_bits(y_plain[one], y[one]) and _eq_bits(y_train[one], y[one])
    del layer.infer    # the wrapper closes over the layer: leave no cycle


def test_infer_allocates_nothing_edge_sized():
    """K = 8, C = 4: one infer call raises torch's peak allocation by less
    than one [E, K] float32 array (678 KB; y is 154 KB), where forward
    allocates at least three."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads = 8
    h, s_src, s_dst, _, _, _ = _layer_inputs(heads, 4, dev, False)
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    edge_bytes = ch.edge_size * heads * 4
    assert edge_bytes == 678400

    def peak_of(fn):
        """Rise of the peak over one call.  Device tensors that earlier
        tests left in reference cycles are collected first and the collector
        is held off meanwhile: a collection inside the call would free them
        below the baseline and understate the rise."""
        fn()                                  # stream scratch, work items
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

    rise = peak_of(lambda: layer.infer(h, s_src, s_dst, SLOPE))
    print(f"infer: peak +{rise} bytes")
    assert rise < edge_bytes
    rise_fwd = peak_of(lambda: layer.forward(h, s_src, s_dst, SLOPE))
    print(f"forward: peak +{rise_fwd} bytes")
    assert rise_fwd >= 3 * edge_bytes


def test_infer_input_checks():
    """Raised before anything is launched, as for GATLayer.forward."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads = 4
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    h = torch.zeros(v, 32, device=dev)
    s = torch.zeros(v, heads, device=dev)
    with pytest.raises(TypeError):           # wrong dtype
        layer.infer(h.double(), s, s)
    with pytest.raises(TypeError):           # fp16 rows
        layer.infer(h.half(), s, s)
    with pytest.raises(TypeError):           # bf16 scalars
        layer.infer(h, s.to(torch.bfloat16), s)
    with pytest.raises(TypeError):
        layer.infer(h.to(torch.bfloat16), s, s.to(torch.bfloat16))
    with pytest.raises(ValueError):          # wrong shape: f % K != 0
        layer.infer(torch.zeros(v, 30, device=dev), s, s)
    with pytest.raises(ValueError):          # [V] scalars on a 4-head layer
        layer.infer(h, torch.zeros(v, device=dev), s)
    with pytest.raises(ValueError):          # too few heads
        layer.infer(h, s, torch.zeros(v, 2, device=dev))
    with pytest.raises(ValueError):          # too few rows
        layer.infer(torch.zeros(v - 1, 32, device=dev), s, s)
    with pytest.raises(TypeError):           # wrong device
        layer.infer(h.cpu(), s, s)
    with pytest.raises(TypeError):
        layer.infer(h, s.cpu(), s)
    with pytest.raises(ValueError):          # not contiguous
        layer.infer(torch.zeros(32, v, device=dev).t(), s, s)
    with pytest.raises(ValueError):
        layer.infer(h, torch.zeros(heads, v, device=dev).t(), s)
    y = layer.infer(h, s, s)                 # and the valid call goes through
    assert y.shape == (v, 32)
    one_head = gat.GATLayer(ch, v, dev)
    y = one_head.infer(h, torch.zeros(v, device=dev),
                       torch.zeros(v, 1, device=dev))
    assert y.shape == (v, 32)
