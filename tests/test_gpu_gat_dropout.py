"""Attention dropout on the GPU (marked gpu): the three *_drop entries against
the float64 references of tests/dropout_ref.py with its restated mask, and
gat.attend / gat.attend_v2 with dropout against dense-index float64 torch
layers that multiply their softmax by mask * scale.

Graph A is the 300-vertex chunk of tests/test_gpu_gat_stable.py (2,800 edges,
one destination of 326 in-edges, which is split into work items, and dozens of
in-degree 1).  Graph B is the committed Cora fixture: no destination reaches
the split of 256, so nothing is merged by atomics and the softmax is
bit-reproducible.  p = 0.5 wherever bits are compared: the scale is exactly 2.

What is exact: w against np.where(keep, alpha * 2, +0.0) with alpha the array
read back from the same call (one fp32 multiply), the sign bit of every
dropped value, the permuted copies, m_sum (one fp32 add), and at p = 0 every
output against the twin entry's on B.

Tolerance of everything else: RTOL, ATOL of tests/test_gpu_gat_heads.py,
1e-4*|ref| + 2e-5, which that file holds for h, grad_y in [-1, 1] and sums of
at most 128 terms, with the absolute term doubled: a dropped weight is at most
1 / (1 - p) = 2 times the softmax weight it scales, so every bound on y and on
the gradients that pass through w grows by at most that factor.  The inputs
stay in that file's range: h, grad_y, the attention scalars, the scores and
the raw gradients are uniform in [-1, 1], a head has C = 8 or 32 columns.  The
softmax itself (alpha) is held to the same bound; its own error is about
1e-7 relative.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_ref as D  # noqa: E402
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402
from test_gpu_gat_heads import Buf, Inp, _assert_bits, _bits, _up32  # noqa: E402
from test_gpu_gat_stable import _chunk as _chunk_a  # noqa: E402

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 2 * 2e-5   # test_gpu_gat_heads.py's, ATOL times 1/(1-p)
SLOPE = 0.2
P, SEED = 0.5, 11
HERE = os.path.dirname(os.path.abspath(__file__))


def _assert_tol(got, ref, name):
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, f"{name}: {got.shape} against {ref.shape}"
    assert np.isfinite(got).all(), f"{name}: non-finite"
    err = np.abs(got - ref)
    bound = RTOL * np.abs(ref) + ATOL
    print(f"{name}: worst {float((err / bound).max()):.3e} of the tolerance")
    bad = err > bound
    assert not bad.any(), (f"{name}: {bad.sum()}/{bad.size} out of tol, "
                           f"worst {err.max():.3e}")


def _t(x):
    return x.detach().cpu().numpy()


# --------------------------------------------------------------------------
# the two graphs
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _chunk_b():
    from neutronstarlite_amd import graph as G
    edges = np.load(os.path.join(HERE, "golden", "cora.2708.edge.self.npy"))
    v = 2708
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    ch = G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]
    assert np.diff(ch.column_offset.astype(np.int64)).max() < R.SPLIT
    return v, ch


@functools.lru_cache(maxsize=None)
def _graph(which):
    """The chunk's CSC arrays as the references take them."""
    v, ch = _chunk_a() if which == "A" else _chunk_b()
    assert ch.src_s == 0 and ch.dst_s == 0
    coff = np.ascontiguousarray(ch.column_offset, dtype=np.uint32)
    rows = np.ascontiguousarray(ch.row_indices, dtype=np.uint32)
    deg = np.diff(coff.astype(np.int64))
    perm, pos = R.csc_to_csr(rows)
    g = {"v": v, "ch": ch, "coff": coff, "rows": rows, "deg": deg,
         "edges": int(coff[-1]), "batch": len(deg), "pos": pos,
         "doe": np.repeat(np.arange(len(deg)), deg)}
    if which == "A":
        assert g["edges"] == 2800 and deg.max() == 326 and (deg == 1).any()
    return g


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    env = {"dev": dev, "shim": shim, "streams": {}}
    for which in ("A", "B"):
        g = _graph(which)
        env[which] = {"coff": _up32(dev, g["coff"]),
                      "rows": _up32(dev, g["rows"]),
                      "pos": _up32(dev, g["pos"])}
    yield env
    for s in env["streams"].values():
        s.destroy()


def _stream(gpu, stable=False, general=False):
    key = (stable, general)
    if key not in gpu["streams"]:
        s = gpu["shim"].Stream.wrap_torch_current()
        s.edge_softmax_stable(1 if stable else 0)
        s.heads_dbg_general(1 if general else 0)
        gpu["streams"][key] = s
    return gpu["streams"][key]


def _check_dropped(w, w_perm, alpha, keep, pos, name):
    """w is one fp32 multiply of the alpha of the same call, or +0.0."""
    want = np.where(keep, alpha * np.float32(2), np.float32(0)).astype(
        np.float32)
    _assert_bits(w, want, name + " w")
    assert (_bits(w)[~keep] == 0).all(), name + ": a dropped value is not +0.0"
    assert (~keep).any() and keep.any()
    assert np.isfinite(w_perm).all(), name + ": permuted slot not written"
    _assert_bits(w_perm[pos], w, name + " permuted w")


# --------------------------------------------------------------------------
# 1. attention forward
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attention_case(which, heads):
    g = _graph(which)
    rng = np.random.default_rng([21000, heads, int(which == "B")])
    s_src = rng.uniform(-1, 1, (g["v"], heads)).astype(np.float32)
    s_dst = rng.uniform(-1, 1, (g["batch"], heads)).astype(np.float32)
    m_ref, s_ref = H.attention_forward(g["coff"], g["rows"], s_src, s_dst,
                                       None, SLOPE)
    return s_src, s_dst, m_ref, s_ref


def _run_attention(gpu, which, st, heads, p, seed, drop=True):
    g, d = _graph(which), gpu[which]
    dev = gpu["dev"]
    s_src, s_dst, _, _ = _attention_case(which, heads)
    d_src, d_dst = Inp(dev, s_src), Inp(dev, s_dst)
    shape = (g["edges"], heads)
    out, out2, msum = Buf(dev, shape), Buf(dev, shape), Buf(dev, shape)
    args = (out.ptr, out2.ptr, d["pos"].data_ptr(), msum.ptr, d_src.ptr,
            d_dst.ptr, d["rows"].data_ptr(), None, SLOPE,
            d["coff"].data_ptr(), g["batch"], g["edges"], heads)
    if not drop:
        st.edge_attention_forward_heads(*args)
        return [b.read("attention twin") for b in (out, out2, msum)]
    alpha = Buf(dev, shape)
    st.edge_attention_forward_drop(*args, alpha.ptr, p, seed)
    return [b.read("attention drop") for b in (out, out2, msum, alpha)]


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads,form", [(1, "auto"), (3, "auto"), (8, "auto"),
                                        (8, "general")])
def test_attention_forward_drop(gpu, heads, form, stable):
    """alpha_out against the float64 softmax; softmax_out bit-equal to
    where(keep, alpha_out * 2, +0.0); the permuted copy bit-equal through the
    slot map; m_sum_out bit-equal to the one fp32 add.  K = 3 runs the
    general lane layout, (8, general) forces it, K = 1 the one-column one."""
    g = _graph("A")
    st = _stream(gpu, stable, form == "general")
    name = f"attention drop K={heads} {form} stable={stable}"
    w, w_perm, msum, alpha = _run_attention(gpu, "A", st, heads, P, SEED)
    assert st.edge_softmax_stable_last() == int(stable)
    _, _, m_ref, s_ref = _attention_case("A", heads)
    _assert_bits(msum, m_ref, name + " m_sum")
    _assert_tol(alpha, s_ref, name + " alpha")
    keep = D.keep_edges(SEED, P, g["edges"], heads)
    _check_dropped(w, w_perm, alpha, keep, g["pos"], name)


# --------------------------------------------------------------------------
# 2. softmax forward
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _scores(which, f):
    g = _graph(which)
    rng = np.random.default_rng([22000, f, int(which == "B")])
    return rng.uniform(-1, 1, (g["edges"], f)).astype(np.float32)


def _run_softmax(gpu, which, st, f, p, seed, drop=True):
    g, d = _graph(which), gpu[which]
    dev = gpu["dev"]
    x = Inp(dev, _scores(which, f))
    shape = (g["edges"], f)
    out, out2, cached = Buf(dev, shape), Buf(dev, shape), Buf(dev, shape)
    if drop:
        st.edge_softmax_forward_drop(out.ptr, out2.ptr, d["pos"].data_ptr(),
                                     x.ptr, cached.ptr, d["coff"].data_ptr(),
                                     g["batch"], g["edges"], f, p, seed)
    else:
        st.edge_softmax_forward_dual(out.ptr, out2.ptr, d["pos"].data_ptr(),
                                     x.ptr, cached.ptr, d["coff"].data_ptr(),
                                     g["batch"], f)
    return [b.read("softmax") for b in (out, out2, cached)]


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("f", [1, 4])
def test_softmax_forward_drop(gpu, f, stable):
    """The checks of test_attention_forward_drop with feature_size as K:
    msg_cached is the softmax, msg_output and msg_output_perm are w."""
    g = _graph("A")
    st = _stream(gpu, stable)
    name = f"softmax drop f={f} stable={stable}"
    w, w_perm, alpha = _run_softmax(gpu, "A", st, f, P, SEED)
    assert st.edge_softmax_stable_last() == int(stable)
    _assert_tol(alpha, R.softmax_forward(g["coff"], _scores("A", f)),
                name + " alpha")
    keep = D.keep_edges(SEED, P, g["edges"], f)
    _check_dropped(w, w_perm, alpha, keep, g["pos"], name)


# --------------------------------------------------------------------------
# 4. softmax backward (3, the p = 0 twins, follows: it uses these helpers)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backward_case(which, f):
    """(grad_w, alpha, lrelu_in): uniform gradients, a real softmax as the
    cache, leaky-relu inputs of both signs; all float32."""
    g = _graph(which)
    rng = np.random.default_rng([23000, f, int(which == "B")])
    gw = rng.uniform(-1, 1, (g["edges"], f)).astype(np.float32)
    alpha = R.softmax_forward(
        g["coff"], rng.uniform(-1, 1, (g["edges"], f))).astype(np.float32)
    lin = rng.uniform(-1, 1, (g["edges"], f)).astype(np.float32)
    return gw, alpha, lin


def _run_backward(gpu, which, st, f, with_lrelu, p, seed, drop=True):
    """Returns (in_grad, in_grad_perm, dst_sum or None, dst prefill)."""
    g, d = _graph(which), gpu[which]
    dev = gpu["dev"]
    gw, alpha, lin = _backward_case(which, f)
    d_gw, d_alpha, d_lin = Inp(dev, gw), Inp(dev, alpha), Inp(dev, lin)
    shape = (g["edges"], f)
    out, out2 = Buf(dev, shape), Buf(dev, shape)
    pre = np.zeros(g["batch"], dtype=np.float32)
    dsum = Buf(dev, (g["batch"],), pre) if f == 1 else None
    lin_ptr = d_lin.ptr if with_lrelu else None
    dsum_ptr = dsum.ptr if dsum else None
    if drop:
        st.edge_softmax_backward_drop(
            out.ptr, out2.ptr, d["pos"].data_ptr(), d_gw.ptr, d_alpha.ptr,
            lin_ptr, SLOPE, d["coff"].data_ptr(), g["batch"], g["edges"], f,
            p, seed, dst_sum=dsum_ptr)
    else:
        st.edge_softmax_backward_fused(
            out.ptr, out2.ptr, d["pos"].data_ptr(), d_gw.ptr, d_alpha.ptr,
            lin_ptr, SLOPE, d["coff"].data_ptr(), g["batch"], f,
            dst_sum=dsum_ptr)
    return (out.read("backward"), out2.read("backward perm"),
            dsum.read("backward dst_sum") if dsum else None, pre)


@pytest.mark.parametrize("with_lrelu", [False, True])
@pytest.mark.parametrize("f", [1, 4])
def test_softmax_backward_drop(gpu, f, with_lrelu):
    """msg_input_grad against the float64 reference with the restated mask,
    both emission orders bit-equal, dst_sum at one column."""
    g = _graph("A")
    st = _stream(gpu)
    name = f"backward drop f={f} lrelu={with_lrelu}"
    gw, alpha, lin = _backward_case("A", f)
    keep = D.keep_edges(SEED, P, g["edges"], f)
    got, got_perm, dsum, pre = _run_backward(gpu, "A", st, f, with_lrelu, P,
                                             SEED)
    ref = D.softmax_backward(g["coff"], gw, alpha, keep, P,
                             lin if with_lrelu else None, SLOPE,
                             pre if f == 1 else None)
    _assert_tol(got, ref[0], name)
    assert np.isfinite(got_perm).all(), name + ": permuted slot not written"
    _assert_bits(got_perm[g["pos"]], got, name + " permuted")
    if f == 1:
        _assert_tol(dsum, ref[2], name + " dst_sum")
    # the mask matters: without it the result is another one
    plain = R.softmax_backward(g["coff"], gw, alpha,
                               lin if with_lrelu else None, SLOPE)[0]
    assert (np.abs(plain - ref[0]) > 10 * ATOL).any()


# --------------------------------------------------------------------------
# 3. p = 0 is the twin entry, bit for bit (graph B: nothing is split)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_p0_attention_is_the_heads_entry(gpu, heads, stable):
    st = _stream(gpu, stable)
    name = f"p=0 attention K={heads} stable={stable}"
    w, w_perm, msum, alpha = _run_attention(gpu, "B", st, heads, 0.0, SEED)
    s, s_perm, msum0 = _run_attention(gpu, "B", st, heads, 0.0, SEED,
                                      drop=False)
    _assert_bits(alpha, s, name + " alpha")
    _assert_bits(w, s, name + " w")
    _assert_bits(w_perm, s_perm, name + " permuted w")
    _assert_bits(msum, msum0, name + " m_sum")


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("f", [1, 4])
def test_p0_softmax_is_the_dual_entry(gpu, f, stable):
    st = _stream(gpu, stable)
    name = f"p=0 softmax f={f} stable={stable}"
    w, w_perm, alpha = _run_softmax(gpu, "B", st, f, 0.0, SEED)
    s, s_perm, cached = _run_softmax(gpu, "B", st, f, 0.0, SEED, drop=False)
    _assert_bits(alpha, cached, name + " cached")
    _assert_bits(w, s, name + " w")
    _assert_bits(w_perm, s_perm, name + " permuted w")


@pytest.mark.parametrize("f,with_lrelu", [(1, True), (4, True), (4, False)])
def test_p0_backward_is_the_fused_entry(gpu, f, with_lrelu):
    st = _stream(gpu)
    name = f"p=0 backward f={f} lrelu={with_lrelu}"
    a = _run_backward(gpu, "B", st, f, with_lrelu, 0.0, SEED)
    b = _run_backward(gpu, "B", st, f, with_lrelu, 0.0, SEED, drop=False)
    _assert_bits(a[0], b[0], name)
    _assert_bits(a[1], b[1], name + " permuted")
    if f == 1:
        _assert_bits(a[2], b[2], name + " dst_sum")


def test_nothing_to_do_writes_nothing(gpu):
    """edges == 0 (a batch of degree-0 destinations) and batch_size == 0:
    the three entries launch nothing and leave prefilled outputs
    bit-unchanged."""
    g = R.empty_graph()
    dev, st = gpu["dev"], _stream(gpu)
    assert g.edges == 0 and g.batch == 7
    rng = np.random.default_rng(27000)
    coff, rows = _up32(dev, g.column_offset), _up32(dev, np.arange(16))
    inp = Inp(dev, rng.normal(size=(32, 4)))
    mk = lambda: Buf(dev, (8, 4), rng.normal(size=(8, 4)) + 1)
    for batch in (g.batch, 0):
        bufs = [mk() for _ in range(4)]
        st.edge_attention_forward_drop(
            bufs[0].ptr, bufs[1].ptr, rows.data_ptr(), bufs[2].ptr, inp.ptr,
            inp.ptr, rows.data_ptr(), None, SLOPE, coff.data_ptr(), batch,
            0 if batch else 5, 4, bufs[3].ptr, P, SEED)
        for b in bufs:
            b.assert_untouched("edge_attention_forward_drop")
        bufs = [mk() for _ in range(3)]
        st.edge_softmax_forward_drop(
            bufs[0].ptr, bufs[1].ptr, rows.data_ptr(), inp.ptr, bufs[2].ptr,
            coff.data_ptr(), batch, 0 if batch else 5, 4, P, SEED)
        for b in bufs:
            b.assert_untouched("edge_softmax_forward_drop")
        bufs = [mk() for _ in range(2)]
        st.edge_softmax_backward_drop(
            bufs[0].ptr, bufs[1].ptr, rows.data_ptr(), inp.ptr, inp.ptr,
            inp.ptr, SLOPE, coff.data_ptr(), batch, 0 if batch else 5, 4, P,
            SEED)
        for b in bufs:
            b.assert_untouched("edge_softmax_backward_drop")


# --------------------------------------------------------------------------
# 5. the layers on A
# --------------------------------------------------------------------------
def _factor(layer, heads, dev):
    """float64 [E, K] mask * scale, the mask restated and indexed by the CSC
    position, and the (destination, head) pairs that lost every in-edge."""
    g = _graph("A")
    keep = D.keep_edges(SEED, P, layer.E, heads)
    kept = R.segment_sum(keep.astype(np.float64), g["coff"])
    dead = (g["deg"] > 0)[:, None] & (kept == 0)
    return torch.from_numpy(D.factor(keep, P)).to(dev), dead


def _gat_reference(h, s_src, s_dst, factor, doe, soe, v, heads):
    h3 = h.view(v, heads, -1)
    e = torch.nn.functional.leaky_relu(
        s_src.view(v, heads)[soe] + s_dst.view(v, heads)[doe], SLOPE)
    ex = torch.exp(e)
    den = torch.zeros(v, heads, dtype=h.dtype, device=h.device).index_add_(
        0, doe, ex)
    w = ex / den[doe] * factor
    return torch.zeros_like(h3).index_add_(
        0, doe, w.unsqueeze(2) * h3[soe]).view(v, -1)


def _gatv2_reference(x_l, x_r, att, factor, doe, soe, v, heads):
    e = doe.numel()
    a = torch.nn.functional.leaky_relu(x_l[soe] + x_r[doe], SLOPE)
    score = (a.view(e, heads, -1) * att.unsqueeze(0)).sum(-1)
    ex = torch.exp(score)
    den = torch.zeros(v, heads, dtype=x_l.dtype,
                      device=x_l.device).index_add_(0, doe, ex)
    w = ex / den[doe] * factor
    msg = w.unsqueeze(2) * x_l[soe].view(e, heads, -1)
    return torch.zeros(v, heads, msg.shape[2], dtype=x_l.dtype,
                       device=x_l.device).index_add_(0, doe, msg).view(v, -1)


def _assert_dead_rows(y, dead, heads, name):
    """At least one (destination, head) lost every in-edge; its C columns of
    y are exactly 0 and everything is finite."""
    assert dead.any(), name + ": no destination lost all its in-edges"
    print(f"{name}: {int(dead.sum())} (destination, head) pairs all dropped")
    y3 = _t(y).reshape(dead.shape[0], heads, -1)
    assert np.isfinite(y3).all()
    assert (y3[dead] == 0).all(), name + ": a fully dropped row is not zero"


@pytest.mark.parametrize("stable", [False, True])
@pytest.mark.parametrize("heads", [1, 4])
def test_attend_with_dropout(heads, stable):
    """y and the gradients of h, s_src, s_dst under gat.attend(dropout=0.5,
    seed=11): the fused gather-dot path (heads = 1) and the heads path."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _chunk_a()
    f = 32
    rng = np.random.default_rng([24000, heads])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    shape = (v,) if heads == 1 else (v, heads)
    h0, gy = (up(rng.uniform(-1, 1, size=(v, f))) for _ in range(2))
    src0, dst0 = (up(rng.uniform(-1, 1, size=shape)) for _ in range(2))
    layer = gat.GATLayer(ch, v, dev, heads=heads, stable=stable)
    h, s_src, s_dst = (t.clone().requires_grad_(True)
                       for t in (h0, src0, dst0))
    y = gat.attend(h, s_src, s_dst, layer, SLOPE, dropout=P, seed=SEED)
    y.backward(gy)
    assert layer.stream.edge_softmax_stable_last() == int(stable)

    factor, dead = _factor(layer, heads, dev)
    hr, sr, dr = (t.double().requires_grad_(True) for t in (h0, src0, dst0))
    y_ref = _gat_reference(hr, sr, dr, factor, layer.dst_of_edge,
                           layer.src_of_edge, v, heads)
    y_ref.backward(gy.double())
    tag = f"attend dropout K={heads} stable={stable}"
    _assert_tol(_t(y), _t(y_ref), tag + " y")
    _assert_tol(_t(h.grad), _t(hr.grad), tag + " grad h")
    _assert_tol(_t(s_src.grad), _t(sr.grad), tag + " grad s_src")
    _assert_tol(_t(s_dst.grad), _t(dr.grad), tag + " grad s_dst")
    _assert_dead_rows(y, dead, heads, tag)
    for t in (h.grad, s_src.grad, s_dst.grad):
        assert bool(torch.isfinite(t).all())


@pytest.mark.parametrize("heads", [1, 4])
def test_attend_v2_with_dropout(heads):
    """y and the gradients of x_l, x_r, att under gat.attend_v2(dropout=0.5,
    seed=11)."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _chunk_a()
    f = 32
    rng = np.random.default_rng([25000, heads])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    xl0, xr0, gy = (up(rng.uniform(-1, 1, size=(v, f))) for _ in range(3))
    att0 = up(rng.uniform(-1, 1, size=(heads, f // heads))
              / np.sqrt(f // heads))
    layer = gat.GATv2Layer(ch, v, dev, heads=heads)
    x_l, x_r, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    y = gat.attend_v2(x_l, x_r, att, layer, SLOPE, dropout=P, seed=SEED)
    y.backward(gy)

    factor, dead = _factor(layer, heads, dev)
    lr, rr, ar = (t.double().requires_grad_(True) for t in (xl0, xr0, att0))
    y_ref = _gatv2_reference(lr, rr, ar, factor, layer.dst_of_edge,
                             layer.src_of_edge, v, heads)
    y_ref.backward(gy.double())
    tag = f"attend_v2 dropout K={heads}"
    _assert_tol(_t(y), _t(y_ref), tag + " y")
    _assert_tol(_t(x_l.grad), _t(lr.grad), tag + " grad x_l")
    _assert_tol(_t(x_r.grad), _t(rr.grad), tag + " grad x_r")
    _assert_tol(_t(att.grad), _t(ar.grad), tag + " grad att")
    _assert_dead_rows(y, dead, heads, tag)
    for t in (x_l.grad, x_r.grad, att.grad):
        assert bool(torch.isfinite(t).all())


# --------------------------------------------------------------------------
# 6. determinism and launch parity (graph B)
# --------------------------------------------------------------------------
def _layer_b(kind, heads, dev):
    from neutronstarlite_amd import gat
    v, ch = _chunk_b()
    f = 32
    rng = np.random.default_rng([26000, heads])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    if kind == "gat":
        shape = (v,) if heads == 1 else (v, heads)
        return (gat.GATLayer(ch, v, dev, heads=heads),
                (up(rng.uniform(-1, 1, size=(v, f))),
                 up(rng.uniform(-1, 1, size=shape)),
                 up(rng.uniform(-1, 1, size=shape))),
                up(rng.uniform(-1, 1, size=(v, f))))
    return (gat.GATv2Layer(ch, v, dev, heads=heads),
            (up(rng.uniform(-1, 1, size=(v, f))),
             up(rng.uniform(-1, 1, size=(v, f))),
             up(rng.uniform(-1, 1, size=(heads, f // heads)))),
            up(rng.uniform(-1, 1, size=(v, f))))


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32),
                       b.contiguous().view(torch.int32))


@pytest.mark.parametrize("kind,heads", [("gat", 1), ("gat", 4), ("gatv2", 4)])
def test_determinism(kind, heads):
    """The same seed twice gives the same w bits, seeds 11 and 12 different
    masks, and dropout=0.0 the y of a call without the argument, with
    today's saved keys."""
    dev = torch.device("cuda:0")
    layer, inputs, _ = _layer_b(kind, heads, dev)
    y1, s1 = layer.forward(*inputs, SLOPE, dropout=P, seed=11)
    y2, s2 = layer.forward(*inputs, SLOPE, dropout=P, seed=11)
    y3, s3 = layer.forward(*inputs, SLOPE, dropout=P, seed=12)
    for key in ("alpha", "w", "w_csr"):
        assert _same_bits(s1[key], s2[key]), key
    assert _same_bits(y1, y2)
    assert s1["p"] == P and s1["seed"] == 11 and s3["seed"] == 12
    assert not torch.equal(s1["w"] == 0, s3["w"] == 0)
    assert _same_bits(s1["alpha"], s3["alpha"])
    want = D.keep_edges(11, P, layer.E, heads)
    assert (_t(s1["w"] != 0) == want).all()

    y0, saved0 = layer.forward(*inputs, SLOPE)
    y0d, saved0d = layer.forward(*inputs, SLOPE, dropout=0.0)
    assert _same_bits(y0, y0d)
    assert set(saved0) == set(saved0d) and "p" not in saved0d
    assert set(s1) - set(saved0) >= {"w", "w_csr", "p", "seed"}


@pytest.mark.parametrize("kind,heads", [("gat", 4), ("gatv2", 4), ("gat", 1)])
def test_launch_parity(kind, heads):
    """A forward + backward with dropout=0.5 makes as many timed launches
    under NTS_KTAG_EDGE as one with dropout=0.0: no mask pass, no apply
    pass."""
    from neutronstarlite_amd import shim
    dev = torch.device("cuda:0")
    layer, inputs, gy = _layer_b(kind, heads, dev)
    streams = (layer.stream, layer.scalar_stream)
    counts = []
    for p in (0.0, P):
        for st in streams:
            st.timing(True)
            st.timing_reset()
        y, saved = layer.forward(*inputs, SLOPE, dropout=p, seed=SEED)
        layer.backward(gy, saved, SLOPE)
        torch.cuda.synchronize()
        counts.append(sum(st.kernel_launches(shim.KTAG_EDGE)
                          for st in streams))
        for st in streams:
            st.timing(False)
    assert counts[0] == counts[1] and counts[0] > 0, counts


# --------------------------------------------------------------------------
# 7. validation, before any launch
# --------------------------------------------------------------------------
def test_validation():
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _chunk_a()
    bad_p = (-0.1, 1.0, 1.5, "0.5")
    bad_seed = (-1, 2**64, 1.5)
    h = torch.zeros(v, 32, device=dev, requires_grad=True)
    for heads in (1, 4):
        layer = gat.GATLayer(ch, v, dev, heads=heads)
        s = torch.zeros((v,) if heads == 1 else (v, heads), device=dev)
        for p in bad_p:
            with pytest.raises(ValueError):
                layer.forward(h.detach(), s, s, SLOPE, dropout=p)
            with pytest.raises(ValueError):
                gat.attend(h, s, s, layer, SLOPE, dropout=p)
        for seed in bad_seed:
            with pytest.raises(ValueError):
                layer.forward(h.detach(), s, s, SLOPE, dropout=0.5, seed=seed)
            with pytest.raises(ValueError):
                gat.attend(h, s, s, layer, SLOPE, dropout=0.5, seed=seed)
    layer2 = gat.GATv2Layer(ch, v, dev, heads=4)
    att = torch.zeros(4, 8, device=dev)
    for p in bad_p:
        with pytest.raises(ValueError):
            layer2.forward(h.detach(), h.detach(), att, SLOPE, dropout=p)
        with pytest.raises(ValueError):
            gat.attend_v2(h, h, att, layer2, SLOPE, dropout=p)
    for seed in bad_seed:
        with pytest.raises(ValueError):
            gat.attend_v2(h, h, att, layer2, SLOPE, dropout=0.5, seed=seed)
    st = layer2.stream
    for p in bad_p:     # the bindings check too: the library would abort
        with pytest.raises(ValueError):
            st.edge_attention_forward_drop(0, 0, 0, 0, 0, 0, 0, 0, SLOPE, 0,
                                           0, 0, 4, 0, p, 0)
        with pytest.raises(ValueError):
            st.edge_softmax_forward_drop(0, 0, 0, 0, 0, 0, 0, 0, 4, p, 0)
        with pytest.raises(ValueError):
            st.edge_softmax_backward_drop(0, 0, 0, 0, 0, 0, SLOPE, 0, 0, 0, 4,
                                          p, 0)


def test_seed_none_draws_from_the_cpu_generator():
    """seed=None is reproducible under torch.manual_seed and differs from
    draw to draw."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    layer, inputs, _ = _layer_b("gat", 4, dev)
    ys = []
    for reseed in (True, False, True):
        if reseed:
            torch.manual_seed(1234)
        ys.append(gat.attend(*inputs, layer, SLOPE, dropout=P))
    assert _same_bits(ys[0], ys[2])
    assert not _same_bits(ys[0], ys[1])
