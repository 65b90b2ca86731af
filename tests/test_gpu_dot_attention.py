"""Dot-product graph attention on the GPU (marked gpu): the fused forward
against dot_ref (float64) on edge_ref.edge_case_graph, gat.DotAttentionLayer
and gat.attend_dot against a dense-index torch layer at test_gpu_gatv2.py's
RTOL, ATOL = 1e-4, 2e-5.  Bound of the fused forward, from inputs and
reference only: a score (one multiply for qs, C products, their fp32 sum in
any order) is off by at most delta[d, k] = max over d's edges of (C + 3) *
2^-24 * scale * sum_j |q*k|, so |y - ref| <= 1e-4*|ref| + (2e-4 + expm1(2*
delta[d, c // C])) * mag[d, c], mag = sum_e alpha*|v| + |prefill|; 1e-4 / 2e-4
are test_gpu_gat_infer.py's."""
import functools
import gc
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
from test_gpu_gat_bf16 import Inp16, round_bf16, widen  # noqa: E402
from test_gpu_gat_heads import (Buf, Inp, _assert_bits, _assert_bound,  # noqa: E402
                                _assert_close, _layer_chunk, _up32)

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_FLAG = "NTS_TEST_DOT_ATTENTION_CHILD"
AUTO = [(8, 16), (4, 8), (2, 128), (1, 128), (1, 1), (3, 7), (5, 33), (1, 602)]
FORMS = [(k, c, "auto") for k, c in AUTO] + [(8, 16, "general"),
                                             (2, 128, "general")]


def dot_ref(coff, rows, src_start, q, k, v, heads, scale):
    """float64 (y, mag, score [E, K], delta [batch, K])."""
    off = np.asarray(coff, dtype=np.int64)
    deg = np.diff(off)
    dst, src = np.repeat(np.arange(len(deg)), deg), rows.astype(np.int64) - src_start
    q, k, v = (np.asarray(a, dtype=np.float64) for a in (q, k, v))
    e, c_per = len(dst), q.shape[1] // heads
    prod = scale * (q[dst] * k[src]).reshape(e, heads, c_per)
    score, live = prod.sum(-1), deg > 0
    top = np.zeros((len(deg), heads))
    delta = np.zeros((len(deg), heads))
    top[live] = np.maximum.reduceat(score, off[:-1][live], axis=0)
    delta[live] = (c_per + 3) * 2.0 ** -24 * np.maximum.reduceat(
        np.abs(prod).sum(-1), off[:-1][live], axis=0)
    ex = np.exp(score - top[dst])
    alpha = ex / R.segment_sum(ex, off)[dst]
    w = np.repeat(alpha, c_per, axis=1)
    return (R.segment_sum(w * v[src], off), R.segment_sum(w * np.abs(v[src]), off),
            score, delta)


def _bound(ref, mag, delta, pre, c_per):
    return 1e-4 * np.abs(ref) + (2e-4 + np.repeat(
        np.expm1(2 * delta), c_per, axis=1)) * (mag + np.abs(pre))


def _env():
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
    return env


@pytest.fixture(scope="module")
def gpu():
    env = _env()
    yield env
    for key in [k for k in env if isinstance(k, tuple)]:
        env[key].destroy()


@functools.lru_cache(maxsize=None)
def _case(heads, c_per, mult=1.0, bf16=False):
    """(q, k, v, scale, prefill, ref, bound, float64 scores), read-only."""
    g = R.edge_case_graph()
    f = heads * c_per
    rng = np.random.default_rng([17000, heads, c_per])
    q = rng.uniform(-2, 2, (g.batch, f)).astype(np.float32)
    k, v = (rng.uniform(-2, 2, (g.v_src, f)).astype(np.float32) for _ in "kv")
    if bf16:
        q, k, v = (widen(round_bf16(a)) for a in (q, k, v))
    scale = float(np.float32(mult * c_per ** -0.5))
    pre = (rng.normal(size=q.shape) + 3).astype(np.float32)
    y, mag, score, delta = dot_ref(g.column_offset, g.row_indices, g.src_start,
                                   q, k, v, heads, scale)
    ref = y + pre
    return q, k, v, scale, pre, ref, _bound(ref, mag, delta, pre, c_per), score


def _run(gpu, st, heads, c_per, d_q, d_k, d_v, scale, pre, shift=0, bf16=False):
    g = R.edge_case_graph()
    out = Buf(gpu["dev"], pre.shape, pre, shift)
    ran = (st.dot_attention_forward_fused_bf16 if bf16
           else st.dot_attention_forward_fused)(
        d_q.ptr, d_k.ptr, d_v.ptr, out.ptr, scale, gpu["rows"].data_ptr(),
        gpu["coff"].data_ptr(), g.src_start, g.batch, g.edges, heads * c_per,
        heads)
    return out, ran


def _check(gpu, key, heads, c_per, name, mult=1.0, shift=0):
    g = R.edge_case_graph()
    q, k, v, scale, pre, ref, bound, _ = _case(heads, c_per, mult)
    st = gpu[key]
    out, ran = _run(gpu, st, heads, c_per, *(Inp(gpu["dev"], a, shift)
                                             for a in (q, k, v)),
                    scale, pre, shift)
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
           f"dot fused K={heads} C={c_per} {form} shift={shift} stable={stable}",
           shift=shift)


@pytest.mark.parametrize("heads,c_per", [(4, 8), (3, 7)])
def test_fused_large_scores(gpu, heads, c_per):
    """scale * 60, scores past 100: the stable mode stays within the bound."""
    assert _case(heads, c_per, 60.0)[7].max() > 100
    _check(gpu, ("auto", 1), heads, c_per,
           f"dot fused large scores K={heads} C={c_per}", mult=60.0)


@pytest.mark.parametrize("stable", [0, 1])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (3, 7)])
def test_fused_reproducible(gpu, heads, c_per, stable):
    """No atomics: two launches are bit-equal on every row, the hub's too."""
    name = f"dot fused twice K={heads} C={c_per} stable={stable}"
    a, b = (_check(gpu, ("auto", stable), heads, c_per, name) for _ in "ab")
    _assert_bits(a, b, name)


@pytest.mark.parametrize("offset", [0, 1, 2])
@pytest.mark.parametrize("heads,c_per", [(8, 16), (4, 6), (3, 7)])
def test_fused_bf16(gpu, heads, c_per, offset):
    """Within the bound on the widened rows; bit-equal to the fp32 entry on
    them when every pointer is aligned (same form and lane width)."""
    dev = gpu["dev"]
    q, k, v, scale, pre, ref, bound, _ = _case(heads, c_per, bf16=True)
    name = f"dot fused bf16 K={heads} C={c_per} offset={offset}"
    for stable in (0, 1):
        st = gpu["auto", stable]
        out, _ = _run(gpu, st, heads, c_per, *(
            Inp16(dev, round_bf16(a), offset) for a in (q, k, v)), scale, pre,
            bf16=True)
        got = out.read(name)
        _assert_bound(got, ref, bound, name)
        if offset == 0:
            rows = (Inp(dev, a) for a in (q, k, v))
            twin, _ = _run(gpu, st, heads, c_per, *rows, scale, pre)
            _assert_bits(got, twin.read(name), name + " vs fp32 entry")


def test_fused_nothing_to_do(gpu):
    dev, st, rng = gpu["dev"], gpu["auto", 0], np.random.default_rng(17100)
    for g, f, batch, edges, want in (
            (R.empty_graph(), 12, 7, 0, 1), (R.empty_graph(), 12, 0, 0, 1),
            (R.edge_case_graph(), 12, 0, 5, 1), (R.tiny_graph(), 2048, 10, 0, 1),
            (R.tiny_graph(), 2048, 10, R.tiny_graph().edges, 0)):
        rows = Inp(dev, rng.normal(size=(g.v_src, f)))
        out = Buf(dev, (g.batch, f), rng.normal(size=(g.batch, f)) + 1)
        ran = st.dot_attention_forward_fused(
            rows.ptr, rows.ptr, rows.ptr, out.ptr, 0.5,
            _up32(dev, g.row_indices).data_ptr(),
            _up32(dev, g.column_offset).data_ptr(), g.src_start, batch, edges,
            f, f // 2048 or 4)
        assert ran == want
        out.assert_untouched(f"dot_attention_forward_fused f={f} {batch} {edges}")


def test_fused_small_split_capped_grid():
    """test_fused's (8, 16) and (3, 7) automatic cases on one workgroup with
    most destinations split: both are latched per process, hence a child."""
    assert not os.environ.get(CHILD_FLAG), "a child must not start children"
    env = {k: v for k, v in os.environ.items() if not k.startswith("NTS_")}
    env.update({"NTS_SPLIT": "8", "NTS_MAX_BLOCKS": "1", CHILD_FLAG: "1"})
    p = subprocess.run([sys.executable, "-m", "tests.test_gpu_dot_attention"],
                       cwd=REPO, env=env, capture_output=True, text=True,
                       timeout=60)
    assert p.returncode == 0 and "dot attention child ok" in p.stdout, (
        f"status {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")


def torch_dot_reference(q, k, v, dst, src, n, heads, scale, factor=None):
    """Dense-index layer under torch autograd; factor scales the softmax."""
    e = dst.numel()
    score = scale * (q[dst] * k[src]).view(e, heads, -1).sum(-1)
    top = torch.full((n, heads), -torch.inf, dtype=q.dtype, device=q.device)
    top = top.scatter_reduce(0, dst[:, None].expand(-1, heads), score, "amax")
    ex = torch.exp(score - top[dst].detach())
    alpha = ex / torch.zeros_like(top).index_add(0, dst, ex)[dst]
    if factor is not None:
        alpha = alpha * factor
    msg = alpha.unsqueeze(2) * v[src].view(e, heads, -1)
    return torch.zeros(n, heads, msg.shape[2], dtype=q.dtype,
                       device=q.device).index_add(0, dst, msg).view(n, -1)


def _layer(heads, stable=False, bf16=False):
    """(gat, layer, q, k, v, grad_y) at f = 32 on _layer_chunk()."""
    from neutronstarlite_amd import gat
    dev, (n, ch) = torch.device("cuda:0"), _layer_chunk()
    rng = np.random.default_rng([17200, heads])
    rows = [torch.from_numpy(rng.uniform(-1, 1, (n, 32)).astype(np.float32))
            .to(dev) for _ in range(4)]
    if bf16:
        rows[:3] = [t.to(torch.bfloat16) for t in rows[:3]]
    return (gat, gat.DotAttentionLayer(ch, n, dev, heads=heads, stable=stable),
            *rows)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4, 8])
def test_layer(heads, stable, bf16):
    """forward / backward, dropout and forward_fused against float64."""
    gat, layer, q, k, v, gy = _layer(heads, stable, bf16)
    n, tag = layer.v, f"K={heads} stable={stable} bf16={bf16}"
    scale = (32 // heads) ** -0.5
    ref_in = [t.double().requires_grad_(True) for t in (q, k, v)]
    topo = (layer.dst_of_edge, layer.src_of_edge, n, heads, scale)
    y_ref = torch_dot_reference(*ref_in, *topo)
    y_ref.backward(gy.double())
    y, saved = layer.forward(q, k, v)
    assert layer.stream.edge_softmax_stable_last() == int(stable)
    _assert_close(y, y_ref, f"forward {tag}")
    for got, ref, name in zip(layer.backward(gy, saved), ref_in, "qkv"):
        assert got.dtype == torch.float32
        _assert_close(got, ref.grad, f"backward grad_{name} {tag}")
    from neutronstarlite_amd import shim
    factor = torch.from_numpy(shim.edge_dropout_keep(
        5, 0.5, 0, layer.E * heads).reshape(layer.E, heads) / 0.5).to(q.device)
    with torch.no_grad():
        _assert_close(layer.forward(q, k, v, dropout=0.5, seed=5)[0],
                      torch_dot_reference(*ref_in, *topo, factor),
                      f"forward dropout {tag}")
    ch = layer.np_ch
    ref, mag, _, delta = dot_ref(ch.column_offset, ch.row_indices, ch.src_s,
                                 *(t.float().cpu().numpy() for t in (q, k, v)),
                                 heads, float(np.float32(scale)))
    _assert_bound(layer.forward_fused(q, k, v).cpu().numpy(), ref,
                  _bound(ref, mag, delta, 0.0, 32 // heads),
                  f"forward_fused {tag}")


def test_attend_dot_routes_without_grad():
    """no_grad and dropout == 0: forward_fused; else the training path."""
    gat, layer, q, k, v, gy = _layer(4, bf16=True)
    calls, fused = [], layer.forward_fused
    layer.forward_fused = lambda *a: (calls.append(1), fused(*a))[1]
    with torch.no_grad():
        y = gat.attend_dot(q, k, v, layer)
        assert len(calls) == 1 and not y.requires_grad
        gat.attend_dot(q, k, v, layer, dropout=0.5, seed=3)
    leaves = [t.clone().requires_grad_(True) for t in (q, k, v)]
    y_train = gat.attend_dot(*leaves, layer)
    y_train.backward(gy)
    assert len(calls) == 1 and all(t.grad.dtype == q.dtype for t in leaves)
    _assert_close(y, y_train.double(), "attend_dot no_grad vs training")
    del layer.forward_fused    # the wrapper closes over the layer


def test_forward_fused_allocates_nothing_edge_sized():
    """K = 8, C = 4: the peak rises by less than one [E, K] float32 array,
    forward's by at least three."""
    gat, layer, q, k, v, _ = _layer(8)
    edge_bytes = layer.E * 8 * 4

    def peak_of(fn):
        fn()                                  # stream scratch, work items
        gc.collect()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.max_memory_allocated()
        out = fn()                            # held: the peak cannot fall
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before

    rise = peak_of(lambda: layer.forward_fused(q, k, v))
    rise_fwd = peak_of(lambda: layer.forward(q, k, v))
    assert rise < edge_bytes and rise_fwd >= 3 * edge_bytes


if __name__ == "__main__":
    assert os.environ.get(CHILD_FLAG) == "1"
    child_env = _env()
    for (heads, c_per), shift, stable in itertools.product(
            ((8, 16), (3, 7)), (0, 1), (0, 1)):
        _check(child_env, ("auto", stable), heads, c_per, "child", shift=shift)
    print("dot attention child ok")
