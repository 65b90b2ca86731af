"""The float64 numpy references of tests/edge_ref.py against the C oracle
(CPU only), on the edge-case graph the GPU tests use.

The oracle computes in float32, so each comparison is held to the float32
error of the oracle's own arithmetic, with u = 2^-24:
  - scatters copy: bit-exact;
  - an accumulation of n terms onto a prefill is n sequential fp32 adds, whose
    forward error is at most n*u*mag (mag = sum of |terms|, prefill included;
    Higham, Accuracy and Stability, eq. 4.4): bound (n + 1)*u*mag;
  - softmax forward is expf (< 1 ulp), a double sum rounded once, one fp32
    division: under 3 ulp = 3.6e-7 relative; bound 1e-6*|ref|;
  - softmax backward is two fp32 products and a subtraction around a double
    sum of fp32 products: under 4*u*mag; bound 1e-6*mag.
"""
import os
import sys

import numpy as np
import pytest

import oracle

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402  (the helper module next to this file)

U = 2.0 ** -24
WIDTHS = [1, 3, 65]


@pytest.fixture(scope="module")
def g():
    return R.edge_case_graph()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _worst(err, bound):
    return float((err / np.maximum(bound, 1e-300)).max())


def test_coverage(g):
    R.assert_coverage(g)
    # the other topologies are what their users assume
    assert R.small_graph().deg.max() > R.SPLIT
    assert R.tiny_graph().batch == 10 and R.tiny_graph().deg.max() <= R.SPLIT
    assert R.empty_graph().edges == 0 and R.empty_graph().batch > 0
    assert not (set(R.OVERWRITE) & set(R.ACCUMULATE))


def test_slot_maps(g):
    perm, pos = R.csc_to_csr(g.row_indices)
    src = g.row_indices.astype(np.int64)
    assert (np.diff(src[perm]) >= 0).all()                 # CSR order
    same = np.diff(src[perm]) == 0
    assert (np.diff(perm)[same] > 0).all()                 # stable
    assert (perm[pos] == np.arange(g.edges)).all()         # inverse
    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    assert roff[-1] == g.edges
    seg_src = np.repeat(np.arange(g.v_src), np.diff(roff.astype(np.int64)))
    assert (src[perm] - g.src_start == seg_src).all()


@pytest.mark.parametrize("f", WIDTHS)
def test_scatters_overwrite_bit_exact(g, f):
    """scatter_src_to_msg and scatter_dst_to_msg overwrite a non-zero
    prefilled message with a pure copy."""
    rng = np.random.default_rng(10 + f)
    mirror = rng.normal(size=(g.m, f)).astype(np.float32)
    dstf = rng.normal(size=(g.batch, f)).astype(np.float32)
    prefill = rng.normal(size=(g.edges, f)).astype(np.float32) + 3.0

    msg = prefill.copy()
    oracle.scatter_src_to_msg(msg, mirror, g.row_indices, g.column_offset,
                              g.mirror_index, g.batch, f)
    ref = R.scatter_src_to_msg(g.column_offset, g.row_indices, g.mirror_index,
                               mirror)
    assert (_bits(msg) == _bits(ref)).all()

    msg = prefill.copy()
    oracle.scatter_dst_to_msg(msg, dstf, g.column_offset, g.batch, f)
    ref = R.scatter_dst_to_msg(g.column_offset, g.row_indices, dstf)
    assert (_bits(msg) == _bits(ref)).all()


@pytest.mark.parametrize("f", WIDTHS)
def test_gathers_and_grad_accumulate(g, f):
    """gather_msg_to_src, gather_msg_to_dst and scatter_grad_back_to_msg add
    onto a non-zero prefill; the reference includes it."""
    rng = np.random.default_rng(20 + f)
    msg = rng.normal(size=(g.edges, f)).astype(np.float32)
    grad = rng.normal(size=(g.batch, f)).astype(np.float32)
    pre_src = rng.normal(size=(g.m, f)).astype(np.float32) + 3.0
    pre_dst = rng.normal(size=(g.batch, f)).astype(np.float32) + 3.0
    pre_msg = rng.normal(size=(g.edges, f)).astype(np.float32) + 3.0
    outdeg = np.bincount(g.mirror_index[g.row_indices], minlength=g.m)

    def check(got, ref, mag, n_terms, prefill, name):
        err = np.abs(got.astype(np.float64) - ref)
        bound = (n_terms.reshape(-1, 1) + 1) * U * mag
        assert (err <= bound).all(), f"{name}: worst {_worst(err, bound):.3e}"
        # it accumulated: the prefill is part of the result
        touched = n_terms > 0
        assert (np.abs(ref - prefill)[touched].max() > 0)
        assert (_bits(got[~touched]) == _bits(prefill[~touched])).all()

    got = pre_src.copy()
    oracle.gather_msg_to_src(got, msg, g.row_indices, g.column_offset,
                             g.mirror_index, g.batch, f)
    ref, mag = R.gather_msg_to_src(g.column_offset, g.row_indices,
                                   g.mirror_index, msg, pre_src)
    check(got, ref, mag, outdeg, pre_src, "gather_msg_to_src")

    got = pre_dst.copy()
    oracle.gather_msg_to_dst(got, msg, g.column_offset, g.batch, f)
    ref, mag = R.gather_msg_to_dst(g.column_offset, g.row_indices, msg,
                                   pre_dst)
    check(got, ref, mag, g.deg, pre_dst, "gather_msg_to_dst")

    got = pre_msg.copy()
    oracle.scatter_grad_back_to_msg(grad, got, g.column_offset, g.batch, f)
    ref, mag = R.scatter_grad_back_to_msg(g.column_offset, g.row_indices,
                                          grad, pre_msg)
    check(got, ref, mag, np.ones(g.edges, dtype=np.int64), pre_msg,
          "scatter_grad_back_to_msg")


@pytest.mark.parametrize("regime", R.SCORE_REGIMES)
@pytest.mark.parametrize("f", WIDTHS)
def test_softmax_forward_and_backward(g, f, regime):
    """Both overwrite a non-zero prefill (NaN here: nothing may survive)."""
    x = R.softmax_scores(regime, g.edges, f)
    out = np.full((g.edges, f), np.nan, dtype=np.float32)
    cached = np.full((g.edges, f), np.nan, dtype=np.float32)
    oracle.edge_softmax_forward(out, x, cached, g.column_offset, g.batch, f)
    ref = R.softmax_forward(g.column_offset, x)
    err = np.abs(out.astype(np.float64) - ref)
    assert (err <= 1e-6 * ref).all(), f"fwd worst {_worst(err, 1e-6 * ref):.3e}"
    assert (_bits(cached) == _bits(out)).all()
    if regime == "equal":
        assert np.allclose(ref, (1.0 / g.deg[g.dst_of_edge])[:, None],
                           rtol=1e-15, atol=0)

    grad = np.random.default_rng(30 + f).normal(
        size=(g.edges, f)).astype(np.float32)
    s32 = ref.astype(np.float32)
    gin = np.full((g.edges, f), np.nan, dtype=np.float32)
    oracle.edge_softmax_backward(gin, grad, s32, g.column_offset, g.batch, f)
    v, mag = R.softmax_backward(g.column_offset, grad, s32)
    err = np.abs(gin.astype(np.float64) - v)
    assert (err <= 1e-6 * mag).all(), f"bwd worst {_worst(err, 1e-6 * mag):.3e}"


def test_softmax_reference_stays_normal_in_fp32(g):
    """A purely relative bound means something only while the reference is a
    normal float32: the smallest softmax output of every score regime, and of
    the attention inputs, is far above the float32 denormal range."""
    for regime in R.SCORE_REGIMES:
        for f in (1, 3, 8):
            x = R.softmax_scores(regime, g.edges, f)
            if regime == "wide":
                assert np.abs(x).max() <= 30.0 and np.abs(x).max() > 29.0
            assert R.softmax_forward(g.column_offset, x).min() > 1e-35
    full, mirror, s_dst = R.attention_inputs(g)
    m, s = R.attention_forward(g.column_offset, g.row_indices, mirror, s_dst,
                               g.mirror_index, 0.2)
    assert s.min() > 1e-35
    assert (m == 0).sum() >= 50 and m.min() < -15 and m.max() > 15
    assert np.abs(m).max() <= 20.0
    # indexed by source id, the same scalars give the same m bit for bit
    m2, s2 = R.attention_forward(g.column_offset, g.row_indices, full, s_dst,
                                 None, 0.2)
    assert (_bits(m) == _bits(m2)).all() and (s == s2).all()


def test_softmax_backward_mask_and_dst_sum(g):
    """The optional parts of the backward reference, spelled out per edge on
    a small graph: factor `slope` at lrelu_in <= 0 (both zeros included), and
    the per-destination sum on top of a prefill."""
    t = R.tiny_graph()
    rng = np.random.default_rng(40)
    x = rng.normal(size=(t.edges, 1)).astype(np.float32)
    s = R.softmax_forward(t.column_offset, x).astype(np.float32)
    grad = rng.normal(size=(t.edges, 1)).astype(np.float32)
    lin = rng.normal(size=(t.edges, 1)).astype(np.float32)
    lin[0], lin[1], lin[2], lin[3] = 0.0, -0.0, 1e-30, -1e-30
    pre = rng.normal(size=t.batch).astype(np.float32) + 2.0
    v, mag, dsum, dmag = R.softmax_backward(t.column_offset, grad, s, lin,
                                            0.2, pre)
    off = t.column_offset.astype(np.int64)
    slope = float(np.float32(0.2))
    for d in range(t.batch):
        gs = [float(grad[e, 0]) * float(s[e, 0]) for e in range(off[d], off[d + 1])]
        tot, acc, amag = sum(gs), float(pre[d]), abs(float(pre[d]))
        for k, e in enumerate(range(off[d], off[d + 1])):
            want = (gs[k] - tot * float(s[e, 0])) * (
                1.0 if lin[e, 0] > 0 else slope)
            assert abs(v[e, 0] - want) <= 1e-12 * mag[e, 0]
            acc += want
            amag += abs(want)
        assert abs(dsum[d] - acc) <= 1e-12 * amag
        assert abs(dmag[d] - amag) <= 1e-12 * amag
    assert dsum[0] == pre[0] and dmag[0] == abs(pre[0])  # degree 0: prefill


def test_weight_sum_and_edge_dot_references(g):
    """Against per-item Python loops on the small graph."""
    t = R.small_graph()
    rng = np.random.default_rng(50)
    w = rng.normal(size=t.edges).astype(np.float32)
    pre = rng.normal(size=t.batch).astype(np.float32)
    out, mag = R.weight_sum(t.column_offset, w, pre)
    off = t.column_offset.astype(np.int64)
    for d in range(t.batch):
        seg = w[off[d]:off[d + 1]].astype(np.float64)
        assert abs(out[d] - (pre[d] + seg.sum())) <= 1e-12 * mag[d]
        assert abs(mag[d] - (abs(pre[d]) + np.abs(seg).sum())) <= 1e-12 * mag[d]
    f = 5
    a = rng.normal(size=(t.batch, f)).astype(np.float32)
    b = rng.normal(size=(t.v_src, f)).astype(np.float32)
    dot, dmag = R.edge_dot(t.column_offset, t.row_indices, t.src_start, a, b)
    for e in range(t.edges):
        pa = a[t.dst_of_edge[e]].astype(np.float64)
        pb = b[int(t.row_indices[e]) - t.src_start].astype(np.float64)
        assert abs(dot[e] - (pa * pb).sum()) <= 1e-12 * dmag[e]
        assert abs(dmag[e] - np.abs(pa * pb).sum()) <= 1e-12 * dmag[e]
