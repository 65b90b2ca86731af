"""GATv2 attention on the GPU (marked gpu): nts_edge_gatv2_score and
nts_edge_gatv2_backward against the float64 references of tests/gatv2_ref.py,
and gat.GATv2Layer with gat.attend_v2 against an independent dense-index
torch layer.

The kernel cases run on edge_ref.edge_case_graph (about 22k edges; degrees on
both sides of 64 and 256 and their multiples, a degree-5000 hub that is split
into work items, zero degrees, src_start = 1000); the split is assumed to be
the default of 256.  Buffers follow tests/test_gpu_gat_heads.py, whose Buf and
Inp are used: every output sits between two guard bands that must come back
bit-unchanged, an output the op fully writes starts as NaN, one it adds to
starts from random non-zero values that the reference includes.

Inputs: x ~ U(-2, 2), att ~ N(0, 1)/sqrt(C); on every third destination that
has edges, x_r's row is the negative of the x_l row of its first in-edge's
source (about 1 % of the edges), so t == 0 on whole rows.

Bounds, none taken from what the kernels give:
  score     1e-5 + 1e-4*mag, the rule of test_edge_dot (a head has at most 602
            terms here: 604*2^-24 = 3.6e-5 of mag in any order)
  grad_own  1e-4*|ref| + 1e-4*mag, the project's rule for signed sums
  grad_att  (n + 2)*2^-24*mag with n the number of edges: the worst case of
            an fp32 sum of n terms in ANY order, each term
            carrying two roundings of its own (slope*t and the product)
  mask      grad_score and att small integers, slope = 0.5, integer prefill:
            every term and every partial sum is a multiple of 0.5 below 2^20,
            so fp32 is exact in any order and unsplit vertices are bit-equal
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import gatv2_ref as V  # noqa: E402
from test_gpu_gat_heads import (Buf, Inp, _assert_bits, _assert_bound,  # noqa: E402
                                _assert_close, _csr_topology,
                                _layer_chunk, _up32)

pytestmark = pytest.mark.gpu

SLOPE = 0.2
SHAPES = [(1, 1), (1, 128), (8, 16), (4, 8), (2, 128), (3, 7), (5, 33),
          (1, 602)]
POW2 = [(k, c) for k, c in SHAPES if c & (c - 1) == 0]
# (K, C, form): every shape on the automatic choice, the power-of-two ones
# (which then run a fast form) also on the general forms
FORMS = ([(k, c, "auto") for k, c in SHAPES]
         + [(k, c, "general") for k, c in POW2])


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    g = R.edge_case_graph()
    roff, cidx, _ = _csr_topology()
    env = {"dev": dev, "shim": shim, "s": shim.Stream.wrap_torch_current(),
           "general": shim.Stream.wrap_torch_current(),
           "coff": _up32(dev, g.column_offset), "rows": _up32(dev, g.row_indices),
           "roff": _up32(dev, roff), "cidx": _up32(dev, cidx)}
    env["general"].heads_dbg_general(1)
    yield env
    env["general"].destroy()


def _stream(gpu, form):
    return gpu["general"] if form == "general" else gpu["s"]


@functools.lru_cache(maxsize=None)
def _inputs(heads, c_per):
    """(x_l (v_src, f), x_r (batch, f), att (K, C)), read-only."""
    g = R.edge_case_graph()
    f = heads * c_per
    rng = np.random.default_rng([11000, heads, c_per])
    x_l = rng.uniform(-2, 2, (g.v_src, f)).astype(np.float32)
    x_r = rng.uniform(-2, 2, (g.batch, f)).astype(np.float32)
    att = (rng.normal(size=(heads, c_per)) / np.sqrt(c_per)).astype(np.float32)
    off = g.column_offset.astype(np.int64)
    forced = np.flatnonzero(g.deg > 0)[::3]
    x_r[forced] = -x_l[g.row_indices[off[forced]].astype(np.int64)
                       - g.src_start]
    assert 0.005 * g.edges <= len(forced) <= 0.02 * g.edges
    for a in (x_l, x_r, att):
        a.setflags(write=False)
    return x_l, x_r, att


def _direction(d):
    """(offset, nbr, nbr_start, device offset key, device nbr key) of the
    walk over the CSC or the CSR; destination d is global vertex
    src_start + d, so nbr_start is src_start both ways."""
    g = R.edge_case_graph()
    if d == "csc":
        return g.column_offset, g.row_indices, g.src_start, "coff", "rows"
    roff, cidx, _ = _csr_topology()
    return roff, cidx, g.src_start, "roff", "cidx"


def _own_nbr(d, x_l, x_r):
    return (x_r, x_l) if d == "csc" else (x_l, x_r)


# --------------------------------------------------------------------------
# score
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _score_ref(heads, c_per):
    g = R.edge_case_graph()
    x_l, x_r, att = _inputs(heads, c_per)
    ref, mag = V.score(g.column_offset, g.row_indices, g.src_start, x_r, x_l,
                       att, SLOPE, heads)
    ref.setflags(write=False)
    mag.setflags(write=False)
    return ref, mag


def _run_score(gpu, heads, c_per, form, shifts):
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    x_l, x_r, att = _inputs(heads, c_per)
    d_r, d_l, d_a = (Inp(dev, a, s) for a, s in zip((x_r, x_l, att), shifts))
    out = Buf(dev, (g.edges, heads))
    st.edge_gatv2_score(out.ptr, d_r.ptr, d_l.ptr, d_a.ptr, SLOPE,
                        gpu["rows"].data_ptr(), gpu["coff"].data_ptr(),
                        g.src_start, g.batch, g.edges, heads * c_per, heads)
    return out


@pytest.mark.parametrize("shift_att", [0, 1])
@pytest.mark.parametrize("shift_src", [0, 1])
@pytest.mark.parametrize("shift_dst", [0, 1])
@pytest.mark.parametrize("heads,c_per,form", FORMS)
def test_score(gpu, heads, c_per, form, shift_dst, shift_src, shift_att):
    """score[e, k] = att[k] . lrelu(x_r[dst] + x_l[src]) over head k, every
    slot written; each of the three pointers on and one float off its
    alignment."""
    ref, mag = _score_ref(heads, c_per)
    name = (f"score K={heads} C={c_per} {form} "
            f"shift={shift_dst}{shift_src}{shift_att}")
    out = _run_score(gpu, heads, c_per, form,
                     (shift_dst, shift_src, shift_att))
    _assert_bound(out.read(name), ref, 1e-5 + 1e-4 * mag, name)


def test_score_zero_rows_give_zero(gpu):
    """On the forced edges t == 0 on the whole row: lrelu(0) = 0 and the
    score is exactly +-0 whatever att holds."""
    g = R.edge_case_graph()
    first = g.column_offset.astype(np.int64)[np.flatnonzero(g.deg > 0)[::3]]
    for heads, c_per in ((8, 16), (3, 7)):
        for form in ("auto", "general"):
            got = _run_score(gpu, heads, c_per, form, (0, 0, 0)).read("score")
            assert (got[first] == 0).all(), (heads, c_per, form)


# --------------------------------------------------------------------------
# backward
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _backward_case(heads, c_per, d):
    g = R.edge_case_graph()
    x_l, x_r, att = _inputs(heads, c_per)
    own, nbr_rows = _own_nbr(d, x_l, x_r)
    off, nbr, start, _, _ = _direction(d)
    f = heads * c_per
    rng = np.random.default_rng([12000, heads, c_per, int(d == "csr")])
    gs = rng.normal(size=(g.edges, heads)).astype(np.float32)
    pre = (rng.normal(size=own.shape) + 3).astype(np.float32)
    pre_att = (rng.normal(size=f) + 3).astype(np.float32)
    assert (pre != 0).all() and (pre_att != 0).all()
    res = V.backward(off, nbr, start, gs, own, nbr_rows, att, SLOPE, heads,
                     pre, pre_att if d == "csc" else None)
    for a in (gs, pre, pre_att) + res:
        a.setflags(write=False)
    return (gs, pre, pre_att) + res


def _run_backward(gpu, d, form, heads, own, nbr_rows, att, gs, pre, pre_att,
                  slope, shift, with_att, name):
    """One launch; returns (grad_own, grad_att buffer contents)."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    _, _, start, koff, knbr = _direction(d)
    d_own, d_nbr, d_att = (Inp(dev, a, shift) for a in (own, nbr_rows, att))
    d_gs = Inp(dev, gs)
    out = Buf(dev, own.shape, pre, shift)
    out_att = Buf(dev, (att.size,), pre_att, shift)
    st.edge_gatv2_backward(out.ptr, out_att.ptr if with_att else None,
                           d_gs.ptr, d_own.ptr, d_nbr.ptr, d_att.ptr, slope,
                           gpu[koff].data_ptr(), gpu[knbr].data_ptr(), start,
                           own.shape[0], g.edges, own.shape[1], heads)
    return out.read(name), out_att.read(name + " grad_att")


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("d", ["csc", "csr"])
@pytest.mark.parametrize("heads,c_per,form", FORMS)
def test_backward(gpu, heads, c_per, form, d, shift):
    """CSC walk (own = x_r) with grad_att, CSR walk (own = x_l) with grad_att
    NULL, onto non-zero prefills.  Vertices without edges stay bit-unchanged;
    with grad_att NULL a sentinel grad_att buffer stays bit-unchanged."""
    g = R.edge_case_graph()
    x_l, x_r, att = _inputs(heads, c_per)
    own, nbr_rows = _own_nbr(d, x_l, x_r)
    gs, pre, pre_att, ref, mag, ref_att, mag_att = _backward_case(
        heads, c_per, d)
    name = f"backward {d} K={heads} C={c_per} {form} shift={shift}"
    got, got_att = _run_backward(gpu, d, form, heads, own, nbr_rows, att, gs,
                                 pre, pre_att, SLOPE, shift, d == "csc", name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    empty = np.diff(_direction(d)[0].astype(np.int64)) == 0
    assert empty.any()
    _assert_bits(got[empty], pre[empty], name + ", vertices without edges")
    if d == "csc":
        _assert_bound(got_att, ref_att,
                      (g.edges + 2) * 2.0 ** -24 * mag_att, name + " grad_att")
    else:
        _assert_bits(got_att, pre_att, name + " grad_att with NULL")


@pytest.mark.parametrize("d", ["csc", "csr"])
@pytest.mark.parametrize("heads,c_per,form", [
    (8, 16, "auto"), (8, 16, "general"), (3, 7, "auto"), (1, 128, "auto")])
def test_backward_mask_convention(gpu, heads, c_per, form, d):
    """grad_score and att integers in [-3, 3], slope = 0.5, integer prefill:
    every term gs*att*lrelu' is a multiple of 0.5 and every partial sum stays
    below 2^20, so fp32 is exact and grad_own of a vertex that is one work
    item equals the float64 reference bit for bit: on the rows where t == 0
    too, which take the slope.  (lrelu'(0) = 1 would differ there: the terms
    are non-zero.)"""
    g = R.edge_case_graph()
    x_l, x_r, _ = _inputs(heads, c_per)
    own, nbr_rows = _own_nbr(d, x_l, x_r)
    off, nbr, start, _, _ = _direction(d)
    f = heads * c_per
    rng = np.random.default_rng([13000, heads, c_per, int(d == "csr")])
    att = rng.integers(1, 4, (heads, c_per)).astype(np.float32)
    att *= rng.choice([-1, 1], att.shape)
    gs = rng.integers(-3, 4, (g.edges, heads)).astype(np.float32)
    pre = rng.integers(1, 9, own.shape).astype(np.float32)
    ref, _, _, _ = V.backward(off, nbr, start, gs, own, nbr_rows, att, 0.5,
                              heads, pre)
    name = f"mask {d} K={heads} C={c_per} {form}"
    got, _ = _run_backward(gpu, d, form, heads, own, nbr_rows, att, gs, pre,
                           np.ones(f), 0.5, 0, False, name)
    deg = np.diff(off.astype(np.int64))
    one = deg <= R.SPLIT
    assert one.any() and ((~one).any() or d == "csr")  # no source is split
    assert (ref.astype(np.float32) == ref).all()
    _assert_bits(got[one], ref[one].astype(np.float32), name)
    # the t == 0 rows are among them and the convention matters there
    voe = np.repeat(np.arange(len(deg)), deg)
    rows = nbr.astype(np.int64) - start
    zero_edge = (own[voe] + nbr_rows[rows] == 0).all(axis=1)
    hit = np.unique(voe[zero_edge & (gs != 0).any(axis=1)])
    assert one[hit].sum() > 20


@pytest.mark.parametrize("heads,c_per,form", [
    (8, 16, "auto"), (8, 16, "general"), (3, 7, "auto"), (2, 128, "auto"),
    (1, 602, "auto")])
def test_backward_grad_att_exact_on_a_grid(gpu, heads, c_per, form):
    """The worst-case bound of test_backward is wide enough to hide a lost or
    doubled partial sum, so once with numbers that fp32 adds exactly in any
    order: rows that are multiples of 2^-3 in [-2, 2], grad_score integers in
    [-3, 3], slope = 0.5 and an integer prefill make every term gs*lrelu(t) a
    multiple of 2^-4 of at most 12, and 22k of them stay below 2^19.
    grad_att, the sum over ALL edges through registers, LDS and atomics, is
    then bit-equal to the float64 reference."""
    g = R.edge_case_graph()
    f = heads * c_per
    rng = np.random.default_rng([15000, heads, c_per])
    x_l = (rng.integers(-16, 17, (g.v_src, f)) / 8.0).astype(np.float32)
    x_r = (rng.integers(-16, 17, (g.batch, f)) / 8.0).astype(np.float32)
    att = rng.integers(-3, 4, (heads, c_per)).astype(np.float32)
    gs = rng.integers(-3, 4, (g.edges, heads)).astype(np.float32)
    pre = rng.integers(1, 9, x_r.shape).astype(np.float32)
    pre_att = rng.integers(1, 9, f).astype(np.float32)
    ref, _, ref_att, mag_att = V.backward(
        g.column_offset, g.row_indices, g.src_start, gs, x_r, x_l, att, 0.5,
        heads, pre, pre_att)
    assert mag_att.max() < 2.0 ** 19
    assert (ref_att.astype(np.float32) == ref_att).all()
    name = f"grid csc K={heads} C={c_per} {form}"
    got, got_att = _run_backward(gpu, "csc", form, heads, x_r, x_l, att, gs,
                                 pre, pre_att, 0.5, 0, True, name)
    _assert_bits(got_att, ref_att.astype(np.float32), name + " grad_att")
    _assert_bits(got, ref.astype(np.float32), name + " grad_own")


# --------------------------------------------------------------------------
# nothing to do, invalid heads
# --------------------------------------------------------------------------
def test_nothing_to_do_writes_nothing(gpu):
    """A batch whose destinations all have degree 0, edges = 0 and
    batch_size = 0 leave prefilled outputs bit-unchanged."""
    g = R.empty_graph()
    dev, st = gpu["dev"], gpu["s"]
    assert g.edges == 0 and g.batch == 7
    rng = np.random.default_rng(6200)
    coff, rows = _up32(dev, g.column_offset), _up32(dev, g.row_indices)
    heads, c_per = 4, 3
    f = heads * c_per
    inp = Inp(dev, rng.normal(size=(32, f)))
    mk = lambda *shape: Buf(dev, shape, rng.normal(size=shape) + 1)
    cp, rp = coff.data_ptr(), rows.data_ptr()
    for batch, edges, cp_ in ((g.batch, 0, cp), (0, 0, cp),
                              (0, 5, gpu["coff"].data_ptr())):
        a = mk(8, heads)
        st.edge_gatv2_score(a.ptr, inp.ptr, inp.ptr, inp.ptr, SLOPE, rp, cp_,
                            g.src_start, batch, edges, f, heads)
        a.assert_untouched("edge_gatv2_score")
        a, b = mk(g.batch, f), mk(f)
        st.edge_gatv2_backward(a.ptr, b.ptr, inp.ptr, inp.ptr, inp.ptr,
                               inp.ptr, SLOPE, cp_, rp, g.src_start, batch,
                               edges, f, heads)
        a.assert_untouched("edge_gatv2_backward grad_own")
        b.assert_untouched("edge_gatv2_backward grad_att")


def test_invalid_heads_raise_in_the_binding(gpu):
    st = gpu["s"]
    for f, heads in ((32, 5), (4, 8), (32, 0)):
        with pytest.raises(ValueError):
            st.edge_gatv2_score(0, 0, 0, 0, SLOPE, 0, 0, 0, 1, 1, f, heads)
        with pytest.raises(ValueError):
            st.edge_gatv2_backward(0, 0, 0, 0, 0, 0, SLOPE, 0, 0, 0, 1, 1, f,
                                   heads)


# --------------------------------------------------------------------------
# the layer and autograd
# --------------------------------------------------------------------------
def torch_gatv2_reference(x_l, x_r, att, dst_of_edge, src_of_edge, v, heads,
                          slope):
    """Independent dense-index GATv2 layer under torch autograd, in the dtype
    of x_l; the softmax is torch.softmax over each destination's in-edges,
    laid out as a dense [v, max degree, K] table padded with -inf."""
    e = dst_of_edge.numel()
    t = x_l[src_of_edge] + x_r[dst_of_edge]
    a = torch.nn.functional.leaky_relu(t, slope).view(e, heads, -1)
    score = (a * att.unsqueeze(0)).sum(-1)
    deg = torch.bincount(dst_of_edge, minlength=v)
    first = torch.cumsum(deg, 0) - deg
    slot = torch.arange(e, device=score.device) - first[dst_of_edge]
    table = torch.full((v, int(deg.max()), heads), -torch.inf,
                       dtype=score.dtype, device=score.device)
    table = table.index_put((dst_of_edge, slot), score)
    live = deg > 0
    soft = torch.zeros_like(table)
    soft[live] = torch.softmax(table[live], dim=1)
    alpha = soft[dst_of_edge, slot]
    msg = alpha.unsqueeze(2) * x_l[src_of_edge].view(e, heads, -1)
    y = torch.zeros(v, heads, msg.shape[2], dtype=x_l.dtype,
                    device=x_l.device).index_add_(0, dst_of_edge, msg)
    return y.view(v, -1), score


def _layer_inputs(heads, c_per, dev, att_scale=1.0):
    v, _ = _layer_chunk()
    f = heads * c_per
    rng = np.random.default_rng([14000, heads, c_per])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    return (up(rng.uniform(-1, 1, size=(v, f))),
            up(rng.uniform(-1, 1, size=(v, f))),
            up(att_scale * rng.normal(size=(heads, c_per)) / np.sqrt(c_per)),
            up(rng.uniform(-1, 1, size=(v, f))))


@pytest.mark.parametrize("heads,c_per,stable", [
    (4, 8, False), (8, 16, False), (3, 11, False), (2, 128, False),
    (8, 16, True)])
def test_layer_attend_v2_autograd(heads, c_per, stable):
    """gat.attend_v2 under autograd against the dense-index layer evaluated
    in float64 from the same float32 inputs, as test_layer_attend_autograd
    does and at its tolerance (RTOL 1e-4, ATOL 2e-5: inputs in [-1, 1], a
    head of at most 128 columns): y, grad x_l, grad x_r, grad att.  The
    destinations of the csc-sorted edge list are grouped, which the
    reference's table relies on."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    xl0, xr0, att0, gy = _layer_inputs(heads, c_per, dev)
    layer = gat.GATv2Layer(ch, v, dev, heads=heads, stable=stable)
    x_l, x_r, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    y = gat.attend_v2(x_l, x_r, att, layer, SLOPE)
    assert y.shape == (v, heads * c_per)
    y.backward(gy)
    assert layer.stream.edge_softmax_stable_last() == int(stable)

    lr, rr, ar = (t.double().requires_grad_(True) for t in (xl0, xr0, att0))
    y_ref, _ = torch_gatv2_reference(lr, rr, ar, layer.dst_of_edge,
                                     layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    tag = f"K={heads} C={c_per} stable={stable}"
    _assert_close(y, y_ref, f"attend_v2 y {tag}")
    _assert_close(x_l.grad, lr.grad, f"attend_v2 grad x_l {tag}")
    _assert_close(x_r.grad, rr.grad, f"attend_v2 grad x_r {tag}")
    _assert_close(att.grad, ar.grad, f"attend_v2 grad att {tag}")


def test_layer_shared_weights():
    """x_l is x_r: autograd adds the two gradients; checked against the
    reference called with one tensor in both places."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads, c_per = 4, 8
    x0, _, att0, gy = _layer_inputs(heads, c_per, dev)
    layer = gat.GATv2Layer(ch, v, dev, heads=heads)
    x, att = (t.clone().requires_grad_(True) for t in (x0, att0))
    y = gat.attend_v2(x, x, att, layer, SLOPE)
    y.backward(gy)
    xr, ar = (t.double().requires_grad_(True) for t in (x0, att0))
    y_ref, _ = torch_gatv2_reference(xr, xr, ar, layer.dst_of_edge,
                                     layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    _assert_close(y, y_ref, "shared y")
    _assert_close(x.grad, xr.grad, "shared grad x (sum of both)")
    _assert_close(att.grad, ar.grad, "shared grad att")


def test_layer_stable_large_scores():
    """att scaled so that scores pass 100, where exp overflows in fp32: on a
    stable layer y and the gradients are finite, the stream reports the
    stable form, and y matches the torch.softmax reference.

    Tolerance of y.  A score s is an fp32 sum of C terms whose absolute
    values add up to m <= C*max|att|*max|t|: its error is at most
    d = (C + 2)*2^-24*m in any order.  The softmax moves by at most
    alpha*(2d + O(d^2)) under score errors bounded by d, and y is a sum of
    alpha*x_l with |x_l| <= 1 and sum alpha = 1, so |dy| <= 2.1*d; on top
    comes the tolerance the ordinary case has, 1e-4*|ref| + 2e-5.  d is
    computed from the inputs below, not from the kernel's output.  The same
    inputs with stable=False are not asserted on."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads, c_per = 4, 8
    xl0, xr0, att0, gy = _layer_inputs(heads, c_per, dev, att_scale=60.0)
    layer = gat.GATv2Layer(ch, v, dev, heads=heads, stable=True)
    x_l, x_r, att = (t.clone().requires_grad_(True) for t in (xl0, xr0, att0))
    y = gat.attend_v2(x_l, x_r, att, layer, SLOPE)
    y.backward(gy)
    assert layer.stream.edge_softmax_stable_last() == 1
    for name, t in (("y", y), ("grad x_l", x_l.grad), ("grad x_r", x_r.grad),
                    ("grad att", att.grad)):
        assert bool(torch.isfinite(t).all()), f"{name}: non-finite"

    with torch.no_grad():
        y_ref, score = torch_gatv2_reference(
            xl0.double(), xr0.double(), att0.double(), layer.dst_of_edge,
            layer.src_of_edge, v, heads, SLOPE)
    assert float(score.max()) > 100
    d = (c_per + 2) * 2.0 ** -24 * c_per * float(att0.abs().max()) * 2.0
    got = y.detach().cpu().numpy().astype(np.float64)
    ref = y_ref.cpu().numpy()
    bound = 1e-4 * np.abs(ref) + 2e-5 + 2.1 * d
    err = np.abs(got - ref)
    print(f"stable large scores: worst {float((err / bound).max()):.3e} of "
          f"the bound, d = {d:.3e}")
    assert (err <= bound).all()


def test_layer_input_checks():
    """Raised before anything is launched: the kernels take raw pointers."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads, f = 4, 32
    layer = gat.GATv2Layer(ch, v, dev, heads=heads)
    x = torch.zeros(v, f, device=dev)
    att = torch.zeros(heads, f // heads, device=dev)
    for call in (layer.forward, lambda *a: gat.attend_v2(*a, layer)):
        with pytest.raises(ValueError):          # f % K != 0
            call(torch.zeros(v, 30, device=dev), x, att)
        with pytest.raises(ValueError):          # x_r of another width
            call(x, torch.zeros(v, 16, device=dev), att)
        with pytest.raises(ValueError):          # att flat
            call(x, x, torch.zeros(f, device=dev))
        with pytest.raises(ValueError):          # att with too few heads
            call(x, x, torch.zeros(2, f // heads, device=dev))
        with pytest.raises(ValueError):          # not contiguous
            call(torch.zeros(f, v, device=dev).t(), x, att)
        with pytest.raises(TypeError):           # not float32
            call(x.double(), x, att)
        with pytest.raises(TypeError):
            call(x, x, att.to(torch.bfloat16))
        with pytest.raises(TypeError):           # not on the device
            call(x.cpu(), x, att)
        with pytest.raises(TypeError):
            call(x, x, att.cpu())
    with pytest.raises(ValueError):
        gat.GATv2Layer(ch, v, dev, heads=0)
    with pytest.raises(ValueError):
        gat.GATv2Layer(ch, v, dev, stable=1)
    y, saved = layer.forward(x, x, att)
    with pytest.raises(ValueError):              # grad_y of another width
        layer.backward(torch.zeros(v, 16, device=dev), saved)
