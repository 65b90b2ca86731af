"""The item-driven GAT edge kernels against float64 numpy references
(tests/edge_ref.py), on a graph built for their edges (marked gpu).

The graph (edge_ref.edge_case_graph, about 22k edges) has a destination on
each side of every degree at which the kernels change behaviour: the 64-lane
stride, the 256-edge split after which a destination becomes several work
items merged by atomics, multiples of the split, a degree-5000 hub, and zero
degree at both ends and in the middle.  Source ids are global (src_start =
1000) and mirror_index is a shuffled map onto fewer rows than sources.  The
split is assumed to be the default of 256.

Every output buffer sits between two guard bands of 64 sentinel floats that
must come back bit-unchanged.  An output the op must fully write starts as
NaN and must come back finite; an output the op adds to starts from random
non-zero values that the reference includes; rows the op has no business
with must come back bit-unchanged.

Bounds.  None is taken from what the kernels give:
  - copies (the scatters, m_sum, permuted second outputs, cached) are exact;
  - sums of signed terms are held to the project's 1e-4 bar applied to the
    magnitude of the computation, 1e-4*|ref| + 1e-4*mag with mag the sum of
    the absolute terms (prefill included), since an fp32 sum in any order
    errs by at most n*2^-24*mag;
  - softmax outputs are held to a purely relative 1e-4*|ref| (derivation at
    test_softmax_forward): on a hub they are about 1/deg, where an absolute
    term would accept anything;
  - per-edge dots as in test_gpu_gather_dot.py (see test_edge_dot).
Each assertion message carries the worst observed ratio to its bound.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402  (the helper module next to this file)

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = np.float32(-12345.678)
SLOPE = 0.2
EXTRA_ROWS = 5   # mirror rows past the M referenced ones


# --------------------------------------------------------------------------
# buffers and comparisons
# --------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Buf:
    """A float32 device buffer of `shape` between two guard bands; filled
    with NaN, or with `fill`."""

    def __init__(self, dev, shape, fill=None):
        shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.shape, self.n = shape, int(np.prod(shape))
        host = np.full(self.n + 2 * GUARD, SENTINEL, dtype=np.float32)
        body = host[GUARD:GUARD + self.n]
        body[:] = np.nan if fill is None else np.asarray(
            fill, dtype=np.float32).reshape(-1)
        self.before = host
        self.t = torch.from_numpy(host.copy()).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    @property
    def prefill(self):
        return self.before[GUARD:GUARD + self.n].reshape(self.shape)

    def read(self, name):
        torch.cuda.synchronize()
        after = self.t.cpu().numpy()
        for side, sl in (("front", slice(0, GUARD)),
                         ("back", slice(GUARD + self.n, None))):
            assert (_bits(after[sl]) == _bits(self.before[sl])).all(), (
                f"{name}: {side} guard band overwritten")
        return after[GUARD:GUARD + self.n].reshape(self.shape)

    def assert_untouched(self, name):
        got = self.read(name)
        assert (_bits(got) == _bits(self.prefill)).all(), (
            f"{name}: written although there was nothing to do")


def _assert_bound(got, ref, bound, name):
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(err > 0, err / np.where(bound > 0, bound, 1e-300), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{name}: worst {worst:.3e} of the bound")
    bad = err > bound
    assert not bad.any(), (f"{name}: {bad.sum()}/{bad.size} out of bound, "
                           f"worst {worst:.3e} of it")


def _assert_bits(got, want, name):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} not bit-equal"


def _assert_rel(got, ref, name):
    _assert_bound(got, ref, 1e-4 * np.abs(ref), name)


# --------------------------------------------------------------------------
# device state
# --------------------------------------------------------------------------
class DevGraph:
    def __init__(self, g, dev):
        def up32(a):
            return torch.from_numpy(
                np.ascontiguousarray(a).view(np.int32)).to(dev)
        self.g = g
        self.coff = up32(g.column_offset)
        self.rows = up32(g.row_indices)
        self.mi = up32(g.mirror_index)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    env = {"dev": dev, "shim": shim, "s": shim.Stream.wrap_torch_current(),
           "big": DevGraph(R.edge_case_graph(), dev),
           "small": DevGraph(R.small_graph(), dev),
           "tiny": DevGraph(R.tiny_graph(), dev),
           "empty": DevGraph(R.empty_graph(), dev)}
    env["up"] = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    return env


def _up32(gpu, a):
    return gpu["up"](np.ascontiguousarray(a, dtype=np.uint32).view(np.int32))


def test_graph_coverage():
    R.assert_coverage(R.edge_case_graph())


# --------------------------------------------------------------------------
# the five edge ops
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _edge_inputs(f):
    g = R.edge_case_graph()
    rng = np.random.default_rng(1000 + f)
    n = lambda *shape: rng.normal(size=shape).astype(np.float32)
    d = {"mirror": n(g.m + EXTRA_ROWS, f), "dstf": n(g.batch, f),
         "msg": n(g.edges, f), "pre_src": n(g.m + EXTRA_ROWS, f) + 3,
         "pre_dst": n(g.batch, f) + 3, "pre_msg": n(g.edges, f) + 3}
    for a in d.values():
        a.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def _edge_ref(op, f):
    g, x = R.edge_case_graph(), _edge_inputs(f)
    co, ri, mi = g.column_offset, g.row_indices, g.mirror_index
    if op == "scatter_src_to_msg":
        return R.scatter_src_to_msg(co, ri, mi, x["mirror"]), None
    if op == "scatter_dst_to_msg":
        return R.scatter_dst_to_msg(co, ri, x["dstf"]), None
    if op == "gather_msg_to_src":
        return R.gather_msg_to_src(co, ri, mi, x["msg"], x["pre_src"])
    if op == "gather_msg_to_dst":
        return R.gather_msg_to_dst(co, ri, x["msg"], x["pre_dst"])
    return R.scatter_grad_back_to_msg(co, ri, x["dstf"], x["pre_msg"])


@pytest.mark.parametrize("f", [1, 3, 64, 65])
@pytest.mark.parametrize("op", R.OVERWRITE[:2] + R.ACCUMULATE)
def test_edge_op(gpu, op, f):
    """The scatters overwrite a NaN message with a pure copy: bit-exact.  The
    two gathers and scatter_grad_back add onto a non-zero prefill and are held
    to 1e-4*|ref| + 1e-4*mag; vertex rows of zero-degree destinations and
    mirror rows no edge refers to stay bit-unchanged."""
    dg, st, dev = gpu["big"], gpu["s"], gpu["dev"]
    g, x = dg.g, _edge_inputs(f)
    ref, mag = _edge_ref(op, f)
    name = f"{op} f={f}"
    topo = (dg.rows.data_ptr(), dg.coff.data_ptr())
    if op == "scatter_src_to_msg":
        src = gpu["up"](x["mirror"])
        out = Buf(dev, (g.edges, f))
        st.scatter_src_mirror_to_msg(out.ptr, src.data_ptr(), *topo,
                                     dg.mi.data_ptr(), g.batch, f)
    elif op == "scatter_dst_to_msg":
        src = gpu["up"](x["dstf"])
        out = Buf(dev, (g.edges, f))
        st.scatter_dst_to_msg(out.ptr, src.data_ptr(), *topo, g.batch, f)
    elif op == "gather_msg_to_src":
        src = gpu["up"](x["msg"])
        out = Buf(dev, (g.m + EXTRA_ROWS, f), x["pre_src"])
        st.gather_msg_to_src_mirror(out.ptr, src.data_ptr(), *topo,
                                    dg.mi.data_ptr(), g.batch, f)
        untouched = np.arange(g.m, g.m + EXTRA_ROWS)
    elif op == "gather_msg_to_dst":
        src = gpu["up"](x["msg"])
        out = Buf(dev, (g.batch, f), x["pre_dst"])
        st.gather_msg_to_dst(out.ptr, src.data_ptr(), *topo, g.batch, f)
        untouched = np.flatnonzero(g.deg == 0)
    else:
        src = gpu["up"](x["dstf"])
        out = Buf(dev, (g.edges, f), x["pre_msg"])
        st.scatter_grad_back_to_message(src.data_ptr(), out.ptr, *topo,
                                        g.batch, f)
        untouched = np.arange(0)
    got = out.read(name)
    if op in R.OVERWRITE:
        assert np.isfinite(got).all(), f"{name}: an edge slot was not written"
        _assert_bits(got, ref.astype(np.float32), name)
        return
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    assert len(untouched) or op == "scatter_grad_back_to_msg"
    _assert_bits(got[untouched], out.prefill[untouched],
                 f"{name}, rows it must not touch")


# --------------------------------------------------------------------------
# softmax forward
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _softmax_case(regime, f):
    g = R.edge_case_graph()
    x = R.softmax_scores(regime, g.edges, f)
    ref = R.softmax_forward(g.column_offset, x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


@functools.lru_cache(maxsize=None)
def _slot_maps():
    """(the CSC-to-CSR slot of every edge, a random permutation)"""
    g = R.edge_case_graph()
    pos = R.csc_to_csr(g.row_indices)[1]
    rnd = np.random.default_rng(6).permutation(g.edges)
    return pos, rnd


@pytest.mark.parametrize("regime", R.SCORE_REGIMES)
@pytest.mark.parametrize("f", [1, 3, 8])
def test_softmax_forward(gpu, f, regime):
    """Plain and _dual (CSC-to-CSR map and a random permutation as perm_pos;
    msg_cached separate, null, and equal to the output).

    Bound: relative only, |got - ref| <= 1e-4*|ref|.  All terms are positive,
    so nothing cancels; __expf at |x| <= 30 contributes a few 1e-6 (the
    argument scaling x*log2(e) rounds at up to 2^-24 * 43, times ln 2, plus
    the hardware exp2); the longest summation chain, on the degree-5000 hub,
    is about 30 additions (4 per lane, 6 butterfly steps, 20 atomics), each
    at 2^-24; one division.  The expected error is under 1e-5, so the margin
    is about ten.  (Measured on an MI355X: worst 3.3e-6 in the [-30, 30]
    regime, 0.7e-6 in the normal one, so __expf stays in the kernels.)  test_edge_ref.py asserts that every reference value is a
    normal float32.  With all scores equal the reference is exactly 1/deg."""
    dg, st, dev = gpu["big"], gpu["s"], gpu["dev"]
    g = dg.g
    x, ref = _softmax_case(regime, f)
    if regime == "equal":
        assert np.allclose(ref, (1.0 / g.deg[g.dst_of_edge])[:, None],
                           rtol=1e-15, atol=0)
    d_x = gpu["up"](x)
    shape = (g.edges, f)
    tag = f"softmax fwd f={f} {regime}"

    out, cached = Buf(dev, shape), Buf(dev, shape)
    st.edge_softmax_forward(out.ptr, d_x.data_ptr(), cached.ptr,
                            dg.rows.data_ptr(), dg.coff.data_ptr(), g.batch, f)
    plain = out.read(tag)
    _assert_rel(plain, ref, tag)
    _assert_bits(cached.read(tag), plain, tag + " cached")

    for pname, pos in zip(("csr map", "random perm"), _slot_maps()):
        d_pos = _up32(gpu, pos)
        for cmode in ("separate", "null", "output"):
            name = f"{tag} dual, {pname}, cached {cmode}"
            out, out2 = Buf(dev, shape), Buf(dev, shape)
            cached = Buf(dev, shape) if cmode == "separate" else None
            cptr = (cached.ptr if cached is not None
                    else out.ptr if cmode == "output" else None)
            st.edge_softmax_forward_dual(out.ptr, out2.ptr, d_pos.data_ptr(),
                                         d_x.data_ptr(), cptr,
                                         dg.coff.data_ptr(), g.batch, f)
            got = out.read(name)
            _assert_rel(got, ref, name)
            got2 = out2.read(name)
            assert np.isfinite(got2).all(), f"{name}: permuted slot not written"
            _assert_bits(got2[pos], got, name + " permuted output")
            if cached is not None:
                _assert_bits(cached.read(name), got, name + " cached")


# --------------------------------------------------------------------------
# softmax backward
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backward_case(f):
    """(g, cached, lrelu_in, dst prefill) and the references of the plain and
    the masked backward."""
    gr = R.edge_case_graph()
    rng = np.random.default_rng(2000 + f)
    grad = rng.normal(size=(gr.edges, f)).astype(np.float32)
    cached = _softmax_case("normal", f)[1].astype(np.float32)
    lin = rng.normal(size=(gr.edges, f)).astype(np.float32)
    flat = lin.reshape(-1)
    edge_values = np.array([0.0, -0.0, 1e-30, -1e-30, 1e-6, -1e-6],
                           dtype=np.float32)
    flat[::3] = np.resize(edge_values, len(flat[::3]))
    pre = (rng.normal(size=gr.batch) + 2).astype(np.float32)
    plain = R.softmax_backward(gr.column_offset, grad, cached)
    if f == 1:
        masked = R.softmax_backward(gr.column_offset, grad, cached, lin,
                                    SLOPE, pre)
    else:
        masked = R.softmax_backward(gr.column_offset, grad, cached, lin, SLOPE)
    for a in (grad, cached, lin, pre):
        a.setflags(write=False)
    return grad, cached, lin, pre, plain, masked


@pytest.mark.parametrize("f", [1, 3, 8])
def test_softmax_backward(gpu, f):
    """Plain, _fused with nothing optional (must agree with plain's
    reference), and _fused with the leaky-relu mask, the CSR-order second
    output and, at f = 1 only, the per-destination sum onto a non-zero
    prefill.  lrelu_in holds 0.0, -0.0 and both signs next to zero on a third
    of the edges; at zero the factor is the slope.

    Bounds: per edge 1e-4*(|g*s| + s*sum|g*s|), the magnitude of the two
    terms that are subtracted; per destination 1e-4*(|prefill| + sum|v|)."""
    dg, st, dev = gpu["big"], gpu["s"], gpu["dev"]
    gr = dg.g
    grad, cached, lin, pre, plain, masked = _backward_case(f)
    assert (_bits(lin) == 0).any() and (_bits(lin) == np.int32(-2**31)).any()
    d_g, d_c, d_l = gpu["up"](grad), gpu["up"](cached), gpu["up"](lin)
    shape = (gr.edges, f)
    pos = _slot_maps()[0]
    d_pos = _up32(gpu, pos)

    name = f"softmax bwd f={f} plain"
    out = Buf(dev, shape)
    st.edge_softmax_backward(out.ptr, d_g.data_ptr(), d_c.data_ptr(),
                             dg.rows.data_ptr(), dg.coff.data_ptr(),
                             gr.batch, f)
    _assert_bound(out.read(name), plain[0], 1e-4 * plain[1], name)

    name = f"softmax bwd f={f} fused, no extras"
    out = Buf(dev, shape)
    st.edge_softmax_backward_fused(out.ptr, None, None, d_g.data_ptr(),
                                   d_c.data_ptr(), None, 0.0,
                                   dg.coff.data_ptr(), gr.batch, f)
    _assert_bound(out.read(name), plain[0], 1e-4 * plain[1], name)

    name = f"softmax bwd f={f} fused, mask + csr copy"
    out, out2 = Buf(dev, shape), Buf(dev, shape)
    dsum = Buf(dev, (gr.batch,), pre) if f == 1 else None
    st.edge_softmax_backward_fused(out.ptr, out2.ptr, d_pos.data_ptr(),
                                   d_g.data_ptr(), d_c.data_ptr(),
                                   d_l.data_ptr(), SLOPE, dg.coff.data_ptr(),
                                   gr.batch, f,
                                   dst_sum=dsum.ptr if dsum else None)
    got = out.read(name)
    _assert_bound(got, masked[0], 1e-4 * masked[1], name)
    got2 = out2.read(name)
    assert np.isfinite(got2).all(), f"{name}: permuted slot not written"
    _assert_bits(got2[pos], got, name + " permuted output")
    if dsum is not None:
        gd = dsum.read(name)
        _assert_bound(gd, masked[2], 1e-4 * masked[3], name + " dst_sum")
        zero = gr.deg == 0
        _assert_bits(gd[zero], pre[zero], name + " dst_sum at degree 0")


# --------------------------------------------------------------------------
# fused attention forward
# --------------------------------------------------------------------------
@pytest.mark.parametrize("with_perm", [True, False])
@pytest.mark.parametrize("with_mirror", [True, False])
def test_attention_forward(gpu, with_mirror, with_perm):
    """Against the float64 reference, not against other kernels.  m spans
    about [-20, 20] and is exactly 0 on some edges (leaky-relu's corner);
    m_sum_out is one fp32 add, so it is compared bit for bit with numpy
    float32.  The softmax is bounded as in test_softmax_forward
    (|leaky_relu(m)| <= 20 < 30), and so is its CSR-order copy, which must
    also be bit-equal to it under the map.  Without mirror_index, s_src is
    indexed by global source id; without perm_pos there is no second
    output."""
    dg, st, dev = gpu["big"], gpu["s"], gpu["dev"]
    g = dg.g
    full, mirror, s_dst = R.attention_inputs(g)
    s_src = mirror if with_mirror else full
    m_ref, s_ref = R.attention_forward(
        g.column_offset, g.row_indices, s_src, s_dst,
        g.mirror_index if with_mirror else None, SLOPE)
    assert (m_ref == 0).any() and m_ref.min() < -15 and m_ref.max() > 15
    perm, pos = R.csc_to_csr(g.row_indices)
    d_pos = _up32(gpu, pos)
    d_src, d_dst = gpu["up"](s_src), gpu["up"](s_dst)
    name = f"attention fwd mirror={with_mirror} perm={with_perm}"
    out, msum = Buf(dev, (g.edges,)), Buf(dev, (g.edges,))
    out2 = Buf(dev, (g.edges,)) if with_perm else None
    st.edge_attention_forward(
        out.ptr, out2.ptr if out2 else None,
        d_pos.data_ptr() if out2 else None, msum.ptr, d_src.data_ptr(),
        d_dst.data_ptr(), dg.rows.data_ptr(),
        dg.mi.data_ptr() if with_mirror else None, SLOPE,
        dg.coff.data_ptr(), g.batch)
    got_m = msum.read(name)
    assert np.isfinite(got_m).all(), f"{name}: m_sum slot not written"
    _assert_bits(got_m, m_ref, name + " m_sum")
    got = out.read(name)
    _assert_rel(got, s_ref, name + " softmax")
    if out2 is not None:
        got2 = out2.read(name)
        _assert_rel(got2, s_ref[perm], name + " CSR-order copy")
        _assert_bits(got2[pos], got, name + " CSR-order copy")


# --------------------------------------------------------------------------
# weight sum, edge dot, permute
# --------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["csc", "csr"])
def test_weight_sum(gpu, order):
    """out[v] += sum of signed weights over v's edge range, on the CSC
    offsets (split destinations) and on the CSR offsets of the same edges.
    Bound 1e-4*(|prefill| + sum|w|); vertices without edges stay
    bit-unchanged."""
    dg, st, dev = gpu["big"], gpu["s"], gpu["dev"]
    g = dg.g
    if order == "csc":
        off, d_off = g.column_offset, dg.coff
    else:
        off = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
        d_off = _up32(gpu, off)
    n = len(off) - 1
    rng = np.random.default_rng(3000)
    w = rng.normal(size=g.edges).astype(np.float32)
    pre = (rng.normal(size=n) + 2).astype(np.float32)
    ref, mag = R.weight_sum(off, w, pre)
    d_w = gpu["up"](w)
    out = Buf(dev, (n,), pre)
    st.weight_sum(out.ptr, d_w.data_ptr(), d_off.data_ptr(), n)
    name = f"weight_sum {order}"
    got = out.read(name)
    _assert_bound(got, ref, 1e-4 * mag, name)
    zero = np.diff(off.astype(np.int64)) == 0
    assert zero.any()
    _assert_bits(got[zero], pre[zero], name + " at degree 0")


@functools.lru_cache(maxsize=None)
def _dot_case(f):
    g = R.edge_case_graph()
    rng = np.random.default_rng(4000 + f)
    a = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    b = rng.uniform(-1, 1, (g.v_src, f)).astype(np.float32)
    return (a, b) + R.edge_dot(g.column_offset, g.row_indices, g.src_start,
                               a, b)


@pytest.mark.parametrize("f", [1, 63, 64, 65, 130, 602])
def test_edge_dot(gpu, f):
    """out[e] = dst_rows[dst] . src_rows[src - src_start], src_start = 1000.
    Degrees 1 to 3 run the tail loop only, 4 the unrolled body only, 5 both.

    Bound, as in test_gpu_gather_dot.py: 1e-5 + 1e-4*sum_j|a_j b_j|.  The
    fp32 forward error of an f-term dot is at most f*2^-24*sum|a_j b_j| in
    any summation order; at the widest f = 602 that is 3.6e-5*sum|a_j b_j|,
    a margin of 2.8, and above 9 for f <= 130."""
    dg, st, dev = gpu["big"], gpu["s"], gpu["dev"]
    g = dg.g
    a, b, ref, mag = _dot_case(f)
    d_a, d_b = gpu["up"](a), gpu["up"](b)
    out = Buf(dev, (g.edges,))
    st.edge_dot(out.ptr, d_a.data_ptr(), d_b.data_ptr(), dg.rows.data_ptr(),
                dg.coff.data_ptr(), g.src_start, g.batch, f)
    _assert_bound(out.read(f"edge_dot f={f}"), ref, 1e-5 + 1e-4 * mag,
                  f"edge_dot f={f}")


@pytest.mark.parametrize("n", [1, 255, 256, 257, 70001])
def test_permute(gpu, n):
    """out[i] = in[index[i]] with repeats in the index, compared as int32 bit
    patterns; the inputs are random bit patterns, NaN payloads among them."""
    st, dev = gpu["s"], gpu["dev"]
    rng = np.random.default_rng(5000 + n)
    n_in = n // 2 + 1
    bits = rng.integers(-2**31, 2**31, n_in, dtype=np.int64).astype(np.int32)
    bits[::5] = np.int32(0x7fc00000) | rng.integers(
        1, 1 << 22, len(bits[::5])).astype(np.int32)      # quiet NaNs
    bits[1::7] = np.int32(0x7f800000) | rng.integers(
        1, 1 << 22, len(bits[1::7])).astype(np.int32)     # signalling NaNs
    index = rng.integers(0, n_in, n).astype(np.uint32)
    assert n == 1 or len(np.unique(index)) < n
    d_in = gpu["up"](bits)
    d_idx = _up32(gpu, index)
    out = Buf(dev, (n,))
    st.permute_f32(out.ptr, d_in.data_ptr(), d_idx.data_ptr(), n)
    got = out.read(f"permute n={n}")
    bad = got.view(np.int32) != bits[index]
    assert not bad.any(), f"permute n={n}: {bad.sum()}/{n} bit patterns differ"


# --------------------------------------------------------------------------
# state that one stream carries from call to call
# --------------------------------------------------------------------------
def _softmax_on(gpu, st, dg, f, seed):
    """Plain softmax forward of fresh scores on graph dg: (got, ref)."""
    g = dg.g
    x = R.softmax_scores("normal", g.edges, f, seed=seed)
    d_x = gpu["up"](x)
    out = Buf(gpu["dev"], (g.edges, f))
    st.edge_softmax_forward(out.ptr, d_x.data_ptr(), None, dg.rows.data_ptr(),
                            dg.coff.data_ptr(), g.batch, f)
    return (out.read(f"softmax f={f} on {g.batch} vertices"),
            R.softmax_forward(g.column_offset, x))


def test_sums_workspace_across_widths_and_graphs(gpu):
    """The per-destination sums workspace is grown on demand and must start
    from zero on every call: f = 8, then 1, then 8 again on the big graph,
    then a 10-vertex graph, all on one new Stream."""
    st = gpu["shim"].Stream.wrap_torch_current()
    try:
        for step, (key, f) in enumerate([("big", 8), ("big", 1), ("big", 8),
                                         ("tiny", 1), ("tiny", 8)]):
            got, ref = _softmax_on(gpu, st, gpu[key], f, seed=10 + step)
            _assert_rel(got, ref, f"step {step}: softmax f={f} on {key}")
    finally:
        st.destroy()


def test_items_cache_reuse(gpu):
    """With items_reuse(1): graph A, graph B (another, smaller offsets
    tensor), A again (a cache hit), then items_cache_clear() and A once more.
    Every result matches its reference.  On destinations of degree <= 256 it
    is also bit-equal to the run with reuse off: such a destination is one
    work item, its sum is one wave reduction in a fixed order followed by a
    single atomic add onto zero, so nothing depends on scheduling."""
    big, small = gpu["big"], gpu["small"]
    one_item = (big.g.deg <= R.SPLIT)[big.g.dst_of_edge]
    one_item_small = (small.g.deg <= R.SPLIT)[small.g.dst_of_edge]
    assert one_item.any() and not one_item.all()
    st = gpu["shim"].Stream.wrap_torch_current()
    try:
        base_a, ref_a = _softmax_on(gpu, st, big, 1, seed=20)
        base_b, ref_b = _softmax_on(gpu, st, small, 1, seed=21)
        _assert_rel(base_a, ref_a, "reuse off, A")
        _assert_rel(base_b, ref_b, "reuse off, B")
        st.items_reuse(1)
        steps = [("A", big, 20), ("B", small, 21), ("A again", big, 20),
                 ("B again", small, 21)]
        for name, dg, seed in steps:
            got, ref = _softmax_on(gpu, st, dg, 1, seed=seed)
            _assert_rel(got, ref, f"reuse on, {name}")
            base, mask = ((base_a, one_item) if dg is big
                          else (base_b, one_item_small))
            _assert_bits(got[mask], base[mask], f"reuse on, {name}")
        st.items_cache_clear()
        got, ref = _softmax_on(gpu, st, big, 1, seed=20)
        _assert_rel(got, ref, "after items_cache_clear, A")
        _assert_bits(got[one_item], base_a[one_item], "after clear, A")
        # other entry points share the cached items
        w = np.random.default_rng(22).normal(size=big.g.edges).astype(
            np.float32)
        pre = np.full(big.g.batch, 0.5, dtype=np.float32)
        out = Buf(gpu["dev"], (big.g.batch,), pre)
        st.weight_sum(out.ptr, gpu["up"](w).data_ptr(), big.coff.data_ptr(),
                      big.g.batch)
        ref, mag = R.weight_sum(big.g.column_offset, w, pre)
        _assert_bound(out.read("reuse on, weight_sum"), ref, 1e-4 * mag,
                      "reuse on, weight_sum")
        st.items_reuse(0)
    finally:
        st.destroy()


# --------------------------------------------------------------------------
# nothing to do
# --------------------------------------------------------------------------
def test_zero_degree_batch_writes_nothing(gpu):
    """On a batch whose destinations all have degree 0, every entry point
    leaves its prefilled outputs bit-unchanged."""
    dg, st, dev = gpu["empty"], gpu["s"], gpu["dev"]
    g = dg.g
    assert g.edges == 0 and g.batch == 7
    rng = np.random.default_rng(6000)
    rows, coff, mi = dg.rows.data_ptr(), dg.coff.data_ptr(), dg.mi.data_ptr()
    f = 3
    inp = gpu["up"](rng.normal(size=(16, f)).astype(np.float32))
    idx = _up32(gpu, np.arange(16))
    mk = lambda *shape: Buf(dev, shape, rng.normal(size=shape) + 1)
    done = []

    def ran(name, *bufs):
        done.append(name)
        for b in bufs:
            b.assert_untouched(name)

    a = mk(8, f)
    st.scatter_src_mirror_to_msg(a.ptr, inp.data_ptr(), rows, coff, mi,
                                 g.batch, f)
    ran("scatter_src_mirror_to_msg", a)
    a = mk(8, f)
    st.gather_msg_to_src_mirror(a.ptr, inp.data_ptr(), rows, coff, mi,
                                g.batch, f)
    ran("gather_msg_to_src_mirror", a)
    a = mk(8, f)
    st.scatter_dst_to_msg(a.ptr, inp.data_ptr(), rows, coff, g.batch, f)
    ran("scatter_dst_to_msg", a)
    a = mk(g.batch, f)
    st.gather_msg_to_dst(a.ptr, inp.data_ptr(), rows, coff, g.batch, f)
    ran("gather_msg_to_dst", a)
    a = mk(8, f)
    st.scatter_grad_back_to_message(inp.data_ptr(), a.ptr, rows, coff,
                                    g.batch, f)
    ran("scatter_grad_back_to_message", a)
    a, c = mk(8, f), mk(8, f)
    st.edge_softmax_forward(a.ptr, inp.data_ptr(), c.ptr, rows, coff,
                            g.batch, f)
    ran("edge_softmax_forward", a, c)
    a, b, c = mk(8, f), mk(8, f), mk(8, f)
    st.edge_softmax_forward_dual(a.ptr, b.ptr, idx.data_ptr(), inp.data_ptr(),
                                 c.ptr, coff, g.batch, f)
    ran("edge_softmax_forward_dual", a, b, c)
    a = mk(8, f)
    st.edge_softmax_backward(a.ptr, inp.data_ptr(), inp.data_ptr(), rows,
                             coff, g.batch, f)
    ran("edge_softmax_backward", a)
    a, b, c = mk(8, 1), mk(8, 1), mk(g.batch)
    st.edge_softmax_backward_fused(a.ptr, b.ptr, idx.data_ptr(),
                                   inp.data_ptr(), inp.data_ptr(),
                                   inp.data_ptr(), SLOPE, coff, g.batch, 1,
                                   dst_sum=c.ptr)
    ran("edge_softmax_backward_fused", a, b, c)
    a, b, c = mk(8), mk(8), mk(8)
    st.edge_attention_forward(a.ptr, b.ptr, idx.data_ptr(), c.ptr,
                              inp.data_ptr(), inp.data_ptr(), rows, mi, SLOPE,
                              coff, g.batch)
    ran("edge_attention_forward", a, b, c)
    a = mk(g.batch)
    st.weight_sum(a.ptr, inp.data_ptr(), coff, g.batch)
    ran("weight_sum", a)
    a = mk(8)
    st.edge_dot(a.ptr, inp.data_ptr(), inp.data_ptr(), rows, coff,
                g.src_start, g.batch, f)
    ran("edge_dot", a)
    a = mk(8)
    st.permute_f32(a.ptr, inp.data_ptr(), idx.data_ptr(), 0)
    ran("permute_f32", a)
    assert len(done) == 13
