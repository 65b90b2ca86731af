"""The fused GATv2 inference forward on the GPU (marked gpu): the entries
against gatv2_ref.layer_forward (float64) on edge_ref.edge_case_graph with the
inputs of test_gpu_gatv2._inputs and the buffers of test_gpu_gat_heads.py, and
GATv2Layer.forward_fused / gat.attend_v2 against the dense-index torch layer.

Bound, from the inputs and the reference only.  A score, an fp32 sum of C
terms in any order, is off by at most delta[d, k] = max over d's edges of
(C + 2) * 2^-24 * mag_score[e, k]; that moves a softmax weight by a factor
within exp(+-2 delta), so |y - ref| <= 1e-4*|ref| + (2e-4 + expm1(2*delta[d,
c // C])) * mag[d, c], the 1e-4 / 2e-4 part being test_gpu_gat_infer.py's.
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
import gatv2_ref as V  # noqa: E402
from test_gpu_gat_bf16 import Inp16, alignment_of, round_bf16, widen  # noqa: E402
from test_gpu_gat_heads import (Buf, Inp, _assert_bits, _assert_bound,  # noqa: E402
                                _assert_close, _layer_chunk, _up32)
from test_gpu_gatv2 import (SLOPE, _inputs, _layer_inputs,  # noqa: E402
                            torch_gatv2_reference)

pytestmark = pytest.mark.gpu

AUTO = [(8, 16), (4, 8), (2, 128), (4, 128), (1, 1), (1, 128), (3, 7), (5, 33),
        (1, 602)]
FORMS = [(k, c, "auto") for k, c in AUTO] + [(8, 16, "general"),
                                             (2, 128, "general")]


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    g = R.edge_case_graph()
    env = {"dev": dev, "shim": shim, "coff": _up32(dev, g.column_offset),
           "rows": _up32(dev, g.row_indices)}
    for form in ("auto", "general"):
        for stable in (0, 1):
            st = env[form, stable] = shim.Stream.wrap_torch_current()
            st.heads_dbg_general(form == "general")
            st.edge_softmax_stable(stable)
    yield env
    for key in [k for k in env if isinstance(k, tuple)]:
        env[key].destroy()


@functools.lru_cache(maxsize=None)
def _case(heads, c_per, scale=1.0, bf16=False):
    """(x_l, x_r, att, prefill, ref, bound, float64 scores), read-only."""
    g = R.edge_case_graph()
    x_l, x_r, att = _inputs(heads, c_per)
    if bf16:
        x_l, x_r = widen(round_bf16(x_l)), widen(round_bf16(x_r))
    att = (att * scale).astype(np.float32)
    rng = np.random.default_rng([16000, heads, c_per])
    pre = (rng.normal(size=x_r.shape) + 3).astype(np.float32)
    y, mag, sc, _ = V.layer_forward(g, x_l, x_r, att, heads, SLOPE)
    _, mag_sc = V.score(g.column_offset, g.row_indices, g.src_start, x_r, x_l,
                        att, SLOPE, heads)
    delta = np.zeros((g.batch, heads))
    live = g.deg > 0
    delta[live] = (c_per + 2) * 2.0 ** -24 * np.maximum.reduceat(
        mag_sc, g.column_offset.astype(np.int64)[:-1][live], axis=0)
    ref = y + pre
    bound = 1e-4 * np.abs(ref) + (2e-4 + np.repeat(
        np.expm1(2 * delta), c_per, axis=1)) * (mag + np.abs(pre))
    return x_l, x_r, att, pre, ref, bound, sc


def _run(gpu, st, heads, c_per, d_l, d_r, att, pre, shift=0, bf16=False):
    g = R.edge_case_graph()
    d_a = Inp(gpu["dev"], att, shift)
    out = Buf(gpu["dev"], pre.shape, pre, shift)
    ran = (st.gatv2_forward_fused_bf16 if bf16 else st.gatv2_forward_fused)(
        d_l.ptr, d_r.ptr, out.ptr, d_a.ptr, SLOPE, gpu["rows"].data_ptr(),
        gpu["coff"].data_ptr(), g.src_start, g.batch, g.edges,
        heads * c_per, heads)
    return out, ran


def _check(gpu, key, heads, c_per, name, scale=1.0, shift=0):
    g = R.edge_case_graph()
    x_l, x_r, att, pre, ref, bound, _ = _case(heads, c_per, scale)
    st = gpu[key]
    out, ran = _run(gpu, st, heads, c_per, Inp(gpu["dev"], x_l, shift),
                    Inp(gpu["dev"], x_r, shift), att, pre, shift)
    got = out.read(name)
    assert ran == 1 and st.edge_softmax_stable_last() == key[1]
    _assert_bound(got, ref, bound, name)
    _assert_bits(got[g.deg == 0], pre[g.deg == 0], name + ", rows without edges")
    return got


@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("heads,c_per,form", FORMS)
def test_fused(gpu, heads, c_per, form, shift, stable):
    """Every form and lane width, pointers on and one float off alignment."""
    _check(gpu, (form, stable), heads, c_per,
           f"fused K={heads} C={c_per} {form} shift={shift} stable={stable}",
           shift=shift)


@pytest.mark.parametrize("heads,c_per", [(4, 8), (3, 7)])
def test_fused_large_scores(gpu, heads, c_per):
    """att * 60, scores past 100: the stable mode stays finite and within the
    bound; the default mode is not asserted on."""
    assert _case(heads, c_per, 60.0)[6].max() > 100
    _check(gpu, ("auto", 1), heads, c_per,
           f"fused large scores K={heads} C={c_per}", scale=60.0)


@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (3, 7)])
def test_fused_reproducible(gpu, heads, c_per, stable):
    """No atomics: two launches are bit-equal on every row, the hub's too."""
    name = f"fused twice K={heads} C={c_per} stable={stable}"
    a, b = (_check(gpu, ("auto", stable), heads, c_per, name) for _ in "ab")
    _assert_bits(a, b, name)


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (4, 6), (3, 7)])
def test_fused_bf16(gpu, heads, c_per, offset):
    """Within the bound on the widened rows, and bit-equal to the fp32 entry
    on them where both run the same form and lane width."""
    dev, f = gpu["dev"], heads * c_per
    x_l, x_r, att, pre, ref, bound, _ = _case(heads, c_per, bf16=True)
    name = f"fused bf16 K={heads} C={c_per} offset={offset}"
    for stable in (0, 1):
        st = gpu["auto", stable]
        out, ran = _run(gpu, st, heads, c_per,
                        Inp16(dev, round_bf16(x_l), offset),
                        Inp16(dev, round_bf16(x_r), offset), att, pre,
                        bf16=True)
        got = out.read(name)
        _assert_bound(got, ref, bound, name)
        plan = gpu["shim"].gatv2_forward_fused_plan
        lanes = [(p["form"], p["cols_per_lane"]) for p in (
            plan(f, heads, 2, alignment_of(offset), 256, 1, 1),
            plan(f, heads, 4, 256, 256, 1, 1))]
        if lanes[0] == lanes[1]:
            twin, _ = _run(gpu, st, heads, c_per, Inp(dev, x_l), Inp(dev, x_r),
                           att, pre)
            _assert_bits(got, twin.read(name), name + " vs fp32 entry")


def test_fused_nothing_to_do(gpu):
    dev, st = gpu["dev"], gpu["auto", 0]
    rng = np.random.default_rng(16100)
    for g, f, batch, edges, want in (
            (R.empty_graph(), 12, 7, 0, 1), (R.empty_graph(), 12, 0, 0, 1),
            (R.edge_case_graph(), 12, 0, 5, 1), (R.tiny_graph(), 2048, 10, 0, 1),
            (R.tiny_graph(), 2048, 10, R.tiny_graph().edges, 0)):
        rows = Inp(dev, rng.normal(size=(g.v_src, f)))
        out = Buf(dev, (g.batch, f), rng.normal(size=(g.batch, f)) + 1)
        ran = st.gatv2_forward_fused(
            rows.ptr, rows.ptr, out.ptr, rows.ptr, SLOPE,
            _up32(dev, g.row_indices).data_ptr(),
            _up32(dev, g.column_offset).data_ptr(), g.src_start, batch, edges,
            f, f // 2048 or 4)
        assert ran == want
        out.assert_untouched(f"gatv2_forward_fused f={f} {batch} {edges}")
    for fn in (st.gatv2_forward_fused, st.gatv2_forward_fused_bf16):
        for f, heads in ((32, 5), (4, 8), (32, 0)):
            with pytest.raises(ValueError):
                fn(0, 0, 0, 0, SLOPE, 0, 0, 0, 1, 1, f, heads)


def _layer(heads, stable=False):
    """(gat, v, layer, x_l, x_r, att) at f = 32 on _layer_chunk()."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    return (gat, v, gat.GATv2Layer(ch, v, dev, heads=heads, stable=stable),
            *_layer_inputs(heads, 32 // heads, dev)[:3])


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_layer_forward_fused(heads, stable, bf16):
    """Against the dense-index layer in float64 at RTOL, ATOL = 1e-4, 2e-5."""
    gat, v, layer, x_l, x_r, att = _layer(heads, stable)
    if bf16:
        x_l, x_r = x_l.to(torch.bfloat16), x_r.to(torch.bfloat16)
    y = layer.forward_fused(x_l, x_r, att, SLOPE)
    assert y.dtype == torch.float32 and y.shape == (v, 32)
    assert layer.stream.edge_softmax_stable_last() == int(stable)
    y_ref, _ = torch_gatv2_reference(
        x_l.double(), x_r.double(), att.double(), layer.dst_of_edge,
        layer.src_of_edge, v, heads, SLOPE)
    _assert_close(y, y_ref, f"forward_fused K={heads} {stable} bf16={bf16}")


def test_attend_v2_routes_without_grad():
    """no_grad and dropout == 0: forward_fused; else the training path."""
    gat, v, layer, x_l, x_r, att = _layer(4)
    calls, fused = [], layer.forward_fused

    def counted(*a, **kw):
        calls.append(1)
        return fused(*a, **kw)

    layer.forward_fused = counted
    with torch.no_grad():
        y = gat.attend_v2(x_l, x_r, att, layer, SLOPE)
        assert len(calls) == 1 and not y.requires_grad
        gat.attend_v2(x_l, x_r, att, layer, SLOPE, dropout=0.5, seed=3)
    y_train = gat.attend_v2(x_l.clone().requires_grad_(True), x_r, att, layer,
                            SLOPE)
    assert len(calls) == 1 and y_train.requires_grad
    _assert_close(y, y_train.double(), "attend_v2 no_grad vs training")
    del layer.forward_fused    # the wrapper closes over the layer


def test_forward_fused_allocates_nothing_edge_sized():
    """K = 8, C = 4: the peak rises by less than one [E, K] float32 array,
    forward's by at least three; the input checks raise before a launch."""
    gat, v, layer, x_l, x_r, att = _layer(8)
    edge_bytes = layer.E * 8 * 4

    def peak_of(fn):
        fn()                                  # stream scratch, work items
        gc.collect()
        gc.disable()
        try:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            before = torch.cuda.max_memory_allocated()
            out = fn()
            torch.cuda.synchronize()
            rise = torch.cuda.max_memory_allocated() - before
            del out
        finally:
            gc.enable()
        return rise

    rise = peak_of(lambda: layer.forward_fused(x_l, x_r, att, SLOPE))
    rise_fwd = peak_of(lambda: layer.forward(x_l, x_r, att, SLOPE))
    assert rise < edge_bytes and rise_fwd >= 3 * edge_bytes
    with pytest.raises(ValueError):              # f % K != 0
        layer.forward_fused(x_l[:, :30].contiguous(), x_r, att)
    with pytest.raises(TypeError):               # mixed row dtypes
        layer.forward_fused(x_l.to(torch.bfloat16), x_r, att)
    with pytest.raises(TypeError):               # not on the device
        layer.forward_fused(x_l, x_r, att.cpu())
