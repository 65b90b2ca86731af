"""bfloat16 feature rows in the attention entries, on the GPU (marked gpu):
nts_gather_by_*_heads_bf16, nts_edge_dot_heads_bf16, nts_edge_gatv2_score_bf16
and nts_edge_gatv2_backward_bf16 against the float64 references of
tests/heads_ref.py and tests/gatv2_ref.py evaluated on the WIDENED rows, and
against their fp32 twins run on the widened rows.

A bf16 value is widened exactly (its bits are the high half of the fp32), so
each entry computes what its fp32 twin computes: the bounds are the ones
tests/test_gpu_gat_heads.py and tests/test_gpu_gatv2.py apply to the fp32
entries, none of them new, and where the lane walks the same columns in the
same order the two results are compared bit for bit.

The cases run on edge_ref.edge_case_graph (about 22k edges, degrees 1...257,
one hub of 5000 that is split into work items, destinations without edges);
the split is assumed to be the default of 256.  Rows are U(-1, 1) rounded to
bf16 with exact zeros, -0.0 and bf16 subnormals planted (make_input of
tests/test_gpu_gather_bf16.py); buffers are the Buf / Inp of
tests/test_gpu_gat_heads.py: guard bands, NaN or non-zero prefill.  A bf16
input sits `offset` ELEMENTS past its allocation's alignment."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import gatv2_ref as V  # noqa: E402
import heads_ref as H  # noqa: E402
from test_gpu_gat_heads import (Buf, Inp, _assert_bits, _assert_bound,  # noqa: E402
                                _csr_topology, _topology, _unsplit_rows,
                                _up32)
from test_gpu_gatv2 import FORMS, _direction, _own_nbr  # noqa: E402

pytestmark = pytest.mark.gpu

SLOPE = 0.2
SPECIAL = np.array([0x0000, 0x8000, 0x0001, 0x007f, 0x8040], dtype=np.uint16)


# --------------------------------------------------------------------------
# bf16 on the host: raw uint16 bits and their exact float32 widening
# --------------------------------------------------------------------------
def widen(bits):
    return (np.ascontiguousarray(bits, dtype=np.uint16).astype(np.uint32)
            << 16).view(np.float32)


def round_bf16(a):
    """float32 -> bf16 bits, round to nearest even (finite inputs)."""
    u = np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def make_rows(shape, rng, lo=-1.0, hi=1.0):
    """(bits, widened float32), read-only: U(lo, hi) rounded to bf16 with
    zeros, -0.0 and subnormals planted, 8 of each."""
    bits = round_bf16(rng.uniform(lo, hi, shape))
    flat = bits.reshape(-1)
    where = rng.choice(flat.size, 8 * len(SPECIAL), replace=flat.size < 64)
    flat[where] = np.tile(SPECIAL, 8)
    x = widen(bits)
    assert np.isfinite(x).all() and (x == 0).any()
    bits.setflags(write=False)
    x.setflags(write=False)
    return bits, x


def test_host_bf16_helpers_agree_with_torch():
    rng = np.random.default_rng(1)
    a = rng.uniform(-3, 3, 4096).astype(np.float32)
    t = torch.from_numpy(a).to(torch.bfloat16)
    assert (t.view(torch.int16).numpy().view(np.uint16) == round_bf16(a)).all()
    assert (t.float().numpy() == widen(round_bf16(a))).all()


class Inp16:
    """bf16 rows on the device whose first element sits `offset` elements
    (2 bytes each) past the allocation's alignment."""

    def __init__(self, dev, bits, offset=0):
        flat = np.ascontiguousarray(bits, dtype=np.uint16).reshape(-1)
        host = np.concatenate([np.zeros(offset, dtype=np.uint16), flat])
        self.t = torch.from_numpy(host.view(np.int16)).to(dev)
        self.ptr = self.t.data_ptr() + 2 * offset
        assert self.t.data_ptr() % 256 == 0


def alignment_of(offset):
    """Alignment in bytes of a pointer `offset` bf16 elements past a 256-byte
    boundary."""
    return 256 if offset == 0 else (2 * offset) & -(2 * offset)


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


# --------------------------------------------------------------------------
# heads gather, both directions
# --------------------------------------------------------------------------
GATHER_CASES = [(8, 16),   # 8-wide lanes
                (4, 4),    # 4-wide lanes
                (4, 6),    # 2-wide lanes
                (3, 7),    # strided, heads change inside a lane
                (5, 33),   # head boundary inside a stride
                (16, 64),  # f = 1024, two slabs at 8 wide
                (16, 1),   # tensor_weight form
                (1, 33)]   # the scalar bf16 entry


def lane_rule(c_per, alignment):
    """The header's rule: the widest of 8 / 4 / 2 elements that divides C
    (hence f) and whose 16- / 8- / 4-byte load the alignment permits."""
    for n in (8, 4, 2):
        if c_per % n == 0 and alignment % (2 * n) == 0:
            return n
    return 1


@functools.lru_cache(maxsize=None)
def _gather_case(heads, c_per, direction):
    g = R.edge_case_graph()
    off, nbr, start, n_in, n_out = _topology(direction)
    f = heads * c_per
    rng = np.random.default_rng([21000, heads, c_per, int(direction == "bwd")])
    bits, x = make_rows((n_in, f), rng)
    w = rng.uniform(-1, 1, (g.edges, heads)).astype(np.float32)
    pre = (rng.normal(size=(n_out, f)) + 3).astype(np.float32)
    assert (pre != 0).all()
    ref, mag = H.gather(off, nbr, start, x, w, heads, pre)
    for a in (w, pre, ref, mag):
        a.setflags(write=False)
    return bits, x, w, pre, ref, mag


def _gather_args(gpu, direction, in_ptr, out_ptr, w_ptr, f):
    g = R.edge_case_graph()
    _, _, start, n_in, n_out = _topology(direction)
    if direction == "fwd":
        return (in_ptr, out_ptr, w_ptr, gpu["rows"].data_ptr(),
                gpu["coff"].data_ptr(), start, start + n_in, start,
                start + n_out, g.edges, n_out, f)
    return (in_ptr, out_ptr, w_ptr, gpu["roff"].data_ptr(),
            gpu["cidx"].data_ptr(), start, start + n_out, start,
            start + n_in, g.edges, n_out, f)


_fp32_gather = {}


def _gather_fp32_twin(gpu, heads, c_per, direction):
    """The fp32 heads entry on the widened rows, once per case."""
    key = (heads, c_per, direction)
    if key not in _fp32_gather:
        _, x, w, pre, _, _ = _gather_case(heads, c_per, direction)
        dev, st = gpu["dev"], gpu["s"]
        d_x, d_w = Inp(dev, x), Inp(dev, w)
        out = Buf(dev, pre.shape, pre)
        entry = (st.gather_by_dst_from_src_heads if direction == "fwd"
                 else st.gather_by_src_from_dst_heads)
        entry(*_gather_args(gpu, direction, d_x.ptr, out.ptr, d_w.ptr,
                            heads * c_per), heads)
        got = out.read("fp32 heads gather")
        got.setflags(write=False)
        _fp32_gather[key] = got
    return _fp32_gather[key]


@pytest.mark.parametrize("offset", [0, 1, 2, 4])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("heads,c_per", GATHER_CASES)
def test_gather_heads_bf16(gpu, heads, c_per, direction, offset):
    """output[v, c] += sum_e w[e, c // C] * widen(input[nbr(e), c]) onto a
    non-zero prefill.  Each output element is one fmaf chain in edge order
    whatever the lane width, so rows of at most 256 edges are bit-equal to
    the fp32 entry on the widened rows at every offset; split rows merge by
    atomics and are held to the fp32 test's bound."""
    bits, x, w, pre, ref, mag = _gather_case(heads, c_per, direction)
    name = f"gather bf16 {direction} K={heads} C={c_per} offset={offset}"
    f = heads * c_per
    off = _topology(direction)[0]
    align = alignment_of(offset)
    want = lane_rule(c_per, align)
    plan = gpu["shim"].gather_plan_heads_bf16(f, heads, align, len(off) - 1,
                                              int(off[-1]))
    assert plan["vector_width"] == want, plan
    if offset == 0:
        assert want == {16: 8, 4: 4, 6: 2, 64: 8}.get(c_per, 1)

    dev, st = gpu["dev"], gpu["s"]
    d_x, d_w = Inp16(dev, bits, offset), Inp(dev, w)
    out = Buf(dev, pre.shape, pre)
    assert out.ptr % 256 == 0
    entry = (st.gather_by_dst_from_src_heads_bf16 if direction == "fwd"
             else st.gather_by_src_from_dst_heads_bf16)
    entry(*_gather_args(gpu, direction, d_x.ptr, out.ptr, d_w.ptr, f), heads)
    got = out.read(name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    empty = np.diff(off.astype(np.int64)) == 0
    assert empty.any()
    _assert_bits(got[empty], pre[empty], name + ", rows without edges")
    one = _unsplit_rows(direction)
    assert one.any()
    twin = _gather_fp32_twin(gpu, heads, c_per, direction)
    _assert_bits(got[one], twin[one], name + ", unsplit rows vs fp32 entry")
    if heads > 1:
        assert st.gather_schedule_last()[0] == 0


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_gather_output_alignment_narrows_the_lane(gpu, direction):
    """The output is accessed in vectors of half the lane's elements: one
    float off its alignment leaves 4 bytes, hence 2 elements per lane."""
    heads, c_per = 8, 16
    bits, x, w, pre, ref, mag = _gather_case(heads, c_per, direction)
    f = heads * c_per
    off = _topology(direction)[0]
    plan = gpu["shim"].gather_plan_heads_bf16(f, heads, 4, len(off) - 1,
                                              int(off[-1]))
    assert plan["vector_width"] == 2
    dev, st = gpu["dev"], gpu["s"]
    d_x, d_w = Inp16(dev, bits, 0), Inp(dev, w)
    out = Buf(dev, pre.shape, pre, shift=1)
    entry = (st.gather_by_dst_from_src_heads_bf16 if direction == "fwd"
             else st.gather_by_src_from_dst_heads_bf16)
    entry(*_gather_args(gpu, direction, d_x.ptr, out.ptr, d_w.ptr, f), heads)
    name = f"gather bf16 {direction}, output one float off"
    got = out.read(name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    one = _unsplit_rows(direction)
    _assert_bits(got[one], _gather_fp32_twin(gpu, heads, c_per, direction)[one],
                 name)


# --------------------------------------------------------------------------
# per-head edge dot: dst_rows fp32, src_rows bf16
# --------------------------------------------------------------------------
# the (K, C) of test_edge_dot_heads, plus (1, 128) and (1, 33) on the row-pair
# forms with one head
DOT_SHAPES = [(8, 16), (2, 64), (2, 128), (3, 16), (8, 64), (16, 2), (16, 1),
              (4, 6), (3, 7), (1, 33), (1, 128)]


@functools.lru_cache(maxsize=None)
def _dot_case(heads, c_per):
    g = R.edge_case_graph()
    f = heads * c_per
    rng = np.random.default_rng([22000, heads, c_per])
    a = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    bits, b = make_rows((g.v_src, f), rng)
    a.setflags(write=False)
    return (a, bits, b) + H.edge_dot(g.column_offset, g.row_indices,
                                     g.src_start, a, b, heads)


def _run_dot(gpu, form, heads, c_per, d_a, d_b, bf16):
    g = R.edge_case_graph()
    st = _stream(gpu, form)
    out = Buf(gpu["dev"], (g.edges, heads))
    (st.edge_dot_heads_bf16 if bf16 else st.edge_dot_heads)(
        out.ptr, d_a.ptr, d_b.ptr, gpu["rows"].data_ptr(),
        gpu["coff"].data_ptr(), g.src_start, g.batch, g.edges, heads * c_per,
        heads)
    return out


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("form", ["auto", "general"])
@pytest.mark.parametrize("heads,c_per", DOT_SHAPES)
def test_edge_dot_heads_bf16(gpu, heads, c_per, form, offset):
    """out[e, k] = dst_rows[dst, head k] . widen(src_rows[src, head k]), the
    bound of test_edge_dot_heads.  With 16-byte aligned pointers and the same
    form the lane holds the same R columns as in the fp32 entry: bit-equal
    (K > 1; at K = 1 the fp32 entry runs another kernel)."""
    dev = gpu["dev"]
    a, bits, b, ref, mag = _dot_case(heads, c_per)
    name = f"edge_dot bf16 K={heads} C={c_per} {form} offset={offset}"
    d_a = Inp(dev, a)
    got = _run_dot(gpu, form, heads, c_per, d_a, Inp16(dev, bits, offset),
                   True).read(name)
    _assert_bound(got, ref, 1e-5 + 1e-4 * mag, name)
    if heads > 1 and offset == 0:
        twin = _run_dot(gpu, form, heads, c_per, d_a, Inp(dev, b),
                        False).read(name + " fp32")
        _assert_bits(got, twin, name + " vs fp32 entry")


@pytest.mark.parametrize("shift", [1, 2])
def test_edge_dot_heads_bf16_fp32_operand_off_alignment(gpu, shift):
    """R follows every pointer by its own element size: dst_rows (fp32) one
    or two floats off its alignment."""
    heads, c_per = 8, 16
    dev = gpu["dev"]
    a, bits, b, ref, mag = _dot_case(heads, c_per)
    name = f"edge_dot bf16 K=8 C=16, dst_rows {shift} floats off"
    got = _run_dot(gpu, "auto", heads, c_per, Inp(dev, a, shift),
                   Inp16(dev, bits, 2 * shift), True).read(name)
    _assert_bound(got, ref, 1e-5 + 1e-4 * mag, name)


# --------------------------------------------------------------------------
# GATv2 score and backward: both row operands bf16
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _v2_inputs(heads, c_per):
    """((bits, widened) of x_l (v_src, f), the same of x_r (batch, f), att
    (K, C)).  On every third destination that has edges x_r's row is the
    negative of the x_l row of its first in-edge's source: bf16 values that
    cancel exactly, t == 0 on whole rows (about 1 % of the edges)."""
    g = R.edge_case_graph()
    f = heads * c_per
    rng = np.random.default_rng([23000, heads, c_per])
    l_bits, _ = make_rows((g.v_src, f), rng)
    r_bits, _ = make_rows((g.batch, f), rng)
    r_bits = r_bits.copy()
    att = (rng.normal(size=(heads, c_per)) / np.sqrt(c_per)).astype(np.float32)
    off = g.column_offset.astype(np.int64)
    forced = np.flatnonzero(g.deg > 0)[::3]
    r_bits[forced] = l_bits[g.row_indices[off[forced]].astype(np.int64)
                            - g.src_start] ^ 0x8000
    x_l, x_r = widen(l_bits), widen(r_bits)
    assert (x_r[forced] == -x_l[g.row_indices[off[forced]].astype(np.int64)
                                - g.src_start]).all()
    for a in (l_bits, r_bits, x_l, x_r, att):
        a.setflags(write=False)
    return (l_bits, x_l), (r_bits, x_r), att


@functools.lru_cache(maxsize=None)
def _score_ref(heads, c_per):
    g = R.edge_case_graph()
    (_, x_l), (_, x_r), att = _v2_inputs(heads, c_per)
    return V.score(g.column_offset, g.row_indices, g.src_start, x_r, x_l, att,
                   SLOPE, heads)


def _run_score(gpu, form, heads, c_per, d_r, d_l, d_a, bf16):
    g = R.edge_case_graph()
    st = _stream(gpu, form)
    out = Buf(gpu["dev"], (g.edges, heads))
    (st.edge_gatv2_score_bf16 if bf16 else st.edge_gatv2_score)(
        out.ptr, d_r.ptr, d_l.ptr, d_a.ptr, SLOPE, gpu["rows"].data_ptr(),
        gpu["coff"].data_ptr(), g.src_start, g.batch, g.edges, heads * c_per,
        heads)
    return out


@pytest.mark.parametrize("offset_src", [0, 1])
@pytest.mark.parametrize("offset_dst", [0, 1])
@pytest.mark.parametrize("heads,c_per,form", FORMS)
def test_score_bf16(gpu, heads, c_per, form, offset_dst, offset_src):
    """score[e, k] = att[k] . lrelu(widen(x_r[dst]) + widen(x_l[src])), the
    bound of test_score; exactly +-0 where the row cancels; bit-equal to the
    fp32 entry on the widened rows with aligned pointers and the same form."""
    g = R.edge_case_graph()
    dev = gpu["dev"]
    (l_bits, x_l), (r_bits, x_r), att = _v2_inputs(heads, c_per)
    ref, mag = _score_ref(heads, c_per)
    name = (f"score bf16 K={heads} C={c_per} {form} "
            f"offset={offset_dst}{offset_src}")
    d_a = Inp(dev, att)
    got = _run_score(gpu, form, heads, c_per, Inp16(dev, r_bits, offset_dst),
                     Inp16(dev, l_bits, offset_src), d_a, True).read(name)
    _assert_bound(got, ref, 1e-5 + 1e-4 * mag, name)
    first = g.column_offset.astype(np.int64)[np.flatnonzero(g.deg > 0)[::3]]
    assert (got[first] == 0).all(), name + ": t == 0 rows"
    if offset_dst == 0 and offset_src == 0:
        twin = _run_score(gpu, form, heads, c_per, Inp(dev, x_r), Inp(dev, x_l),
                          d_a, False).read(name + " fp32")
        _assert_bits(got, twin, name + " vs fp32 entry")


def test_score_bf16_att_off_alignment(gpu):
    """att (fp32) one float off its alignment: one column per lane."""
    heads, c_per = 8, 16
    dev = gpu["dev"]
    (l_bits, _), (r_bits, _), att = _v2_inputs(heads, c_per)
    ref, mag = _score_ref(heads, c_per)
    name = "score bf16 K=8 C=16, att one float off"
    got = _run_score(gpu, "auto", heads, c_per, Inp16(dev, r_bits),
                     Inp16(dev, l_bits), Inp(dev, att, 1), True).read(name)
    _assert_bound(got, ref, 1e-5 + 1e-4 * mag, name)


@functools.lru_cache(maxsize=None)
def _backward_case(heads, c_per, d):
    g = R.edge_case_graph()
    (_, x_l), (_, x_r), att = _v2_inputs(heads, c_per)
    own, nbr_rows = _own_nbr(d, x_l, x_r)
    off, nbr, start, _, _ = _direction(d)
    f = heads * c_per
    rng = np.random.default_rng([24000, heads, c_per, int(d == "csr")])
    gs = rng.normal(size=(g.edges, heads)).astype(np.float32)
    pre = (rng.normal(size=own.shape) + 3).astype(np.float32)
    pre_att = (rng.normal(size=f) + 3).astype(np.float32)
    assert (pre != 0).all() and (pre_att != 0).all()
    res = V.backward(off, nbr, start, gs, own, nbr_rows, att, SLOPE, heads,
                     pre, pre_att if d == "csc" else None)
    for a in (gs, pre, pre_att) + res:
        a.setflags(write=False)
    return (gs, pre, pre_att) + res


def _run_backward(gpu, d, form, heads, d_own, d_nbr, shape, att, gs, pre,
                  pre_att, slope, with_att, bf16, name):
    """One launch; returns (grad_own, grad_att buffer contents)."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    _, _, start, koff, knbr = _direction(d)
    d_att, d_gs = Inp(dev, att), Inp(dev, gs)
    out = Buf(dev, shape, pre)
    out_att = Buf(dev, (att.size,), pre_att)
    (st.edge_gatv2_backward_bf16 if bf16 else st.edge_gatv2_backward)(
        out.ptr, out_att.ptr if with_att else None, d_gs.ptr, d_own.ptr,
        d_nbr.ptr, d_att.ptr, slope, gpu[koff].data_ptr(),
        gpu[knbr].data_ptr(), start, shape[0], g.edges, shape[1], heads)
    return out.read(name), out_att.read(name + " grad_att")


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("d", ["csc", "csr"])
@pytest.mark.parametrize("heads,c_per,form", FORMS)
def test_backward_bf16(gpu, heads, c_per, form, d, offset):
    """CSC walk (own = x_r) with grad_att, CSR walk (own = x_l) with grad_att
    NULL, onto non-zero prefills, at the bounds of test_backward.  offset
    moves both bf16 pointers one element.  With aligned pointers and the same
    form grad_own of a vertex of at most 256 edges is the fp32 entry's on the
    widened rows bit for bit."""
    g = R.edge_case_graph()
    dev = gpu["dev"]
    (l_bits, x_l), (r_bits, x_r), att = _v2_inputs(heads, c_per)
    own, nbr_rows = _own_nbr(d, x_l, x_r)
    own_bits, nbr_bits = _own_nbr(d, l_bits, r_bits)
    gs, pre, pre_att, ref, mag, ref_att, mag_att = _backward_case(
        heads, c_per, d)
    name = f"backward bf16 {d} K={heads} C={c_per} {form} offset={offset}"
    got, got_att = _run_backward(
        gpu, d, form, heads, Inp16(dev, own_bits, offset),
        Inp16(dev, nbr_bits, offset), own.shape, att, gs, pre, pre_att, SLOPE,
        d == "csc", True, name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    deg = np.diff(_direction(d)[0].astype(np.int64))
    assert (deg == 0).any()
    _assert_bits(got[deg == 0], pre[deg == 0],
                 name + ", vertices without edges")
    if d == "csc":
        _assert_bound(got_att, ref_att,
                      (g.edges + 2) * 2.0 ** -24 * mag_att, name + " grad_att")
    else:
        _assert_bits(got_att, pre_att, name + " grad_att with NULL")
    if offset == 0:
        twin, _ = _run_backward(
            gpu, d, form, heads, Inp(dev, own), Inp(dev, nbr_rows), own.shape,
            att, gs, pre, pre_att, SLOPE, d == "csc", False, name + " fp32")
        one = deg <= R.SPLIT
        assert one.any()
        _assert_bits(got[one], twin[one], name + " vs fp32 entry, unsplit")


@pytest.mark.parametrize("d", ["csc", "csr"])
@pytest.mark.parametrize("heads,c_per,form", [
    (8, 16, "auto"), (8, 16, "general"), (3, 7, "auto"), (1, 128, "auto")])
def test_backward_bf16_mask_convention(gpu, heads, c_per, form, d):
    """test_backward_mask_convention on bf16 rows: grad_score and att
    integers in [-3, 3], slope = 0.5, integer prefill make fp32 exact in any
    order, so grad_own of an unsplit vertex equals the float64 reference bit
    for bit — on the rows where the two bf16 values cancel to t == 0 too,
    which take the slope (lrelu'(0) = 1 would differ: the terms are
    non-zero)."""
    g = R.edge_case_graph()
    dev = gpu["dev"]
    (l_bits, x_l), (r_bits, x_r), _ = _v2_inputs(heads, c_per)
    own, nbr_rows = _own_nbr(d, x_l, x_r)
    own_bits, nbr_bits = _own_nbr(d, l_bits, r_bits)
    off, nbr, start, _, _ = _direction(d)
    f = heads * c_per
    rng = np.random.default_rng([25000, heads, c_per, int(d == "csr")])
    att = rng.integers(1, 4, (heads, c_per)).astype(np.float32)
    att *= rng.choice([-1, 1], att.shape)
    gs = rng.integers(-3, 4, (g.edges, heads)).astype(np.float32)
    pre = rng.integers(1, 9, own.shape).astype(np.float32)
    ref, _, _, _ = V.backward(off, nbr, start, gs, own, nbr_rows, att, 0.5,
                              heads, pre)
    name = f"mask bf16 {d} K={heads} C={c_per} {form}"
    got, _ = _run_backward(gpu, d, form, heads, Inp16(dev, own_bits),
                           Inp16(dev, nbr_bits), own.shape, att, gs, pre,
                           np.ones(f), 0.5, False, True, name)
    deg = np.diff(off.astype(np.int64))
    one = deg <= R.SPLIT
    assert (ref.astype(np.float32) == ref).all()
    _assert_bits(got[one], ref[one].astype(np.float32), name)
    voe = np.repeat(np.arange(len(deg)), deg)
    rows = nbr.astype(np.int64) - start
    zero_edge = (own[voe] + nbr_rows[rows] == 0).all(axis=1)
    hit = np.unique(voe[zero_edge & (gs != 0).any(axis=1)])
    assert one[hit].sum() > 20


@pytest.mark.parametrize("heads,c_per,form", [
    (8, 16, "auto"), (8, 16, "general"), (3, 7, "auto"), (2, 128, "auto"),
    (1, 602, "auto")])
def test_backward_bf16_grad_att_exact_on_a_grid(gpu, heads, c_per, form):
    """Rows on a 2^-3 grid in [-2, 2] (representable in bf16), grad_score
    integers in [-3, 3], slope = 0.5 and integer prefills: every term is a
    multiple of 2^-4 and 22k of them stay below 2^19, so fp32 adds them
    exactly in any order and grad_att — registers, LDS, atomics — is bit-equal
    to the float64 reference; so is grad_own, split vertices included."""
    g = R.edge_case_graph()
    dev = gpu["dev"]
    f = heads * c_per
    rng = np.random.default_rng([26000, heads, c_per])
    x_l = (rng.integers(-16, 17, (g.v_src, f)) / 8.0).astype(np.float32)
    x_r = (rng.integers(-16, 17, (g.batch, f)) / 8.0).astype(np.float32)
    l_bits, r_bits = round_bf16(x_l), round_bf16(x_r)
    assert (widen(l_bits) == x_l).all() and (widen(r_bits) == x_r).all()
    att = rng.integers(-3, 4, (heads, c_per)).astype(np.float32)
    gs = rng.integers(-3, 4, (g.edges, heads)).astype(np.float32)
    pre = rng.integers(1, 9, x_r.shape).astype(np.float32)
    pre_att = rng.integers(1, 9, f).astype(np.float32)
    ref, _, ref_att, mag_att = V.backward(
        g.column_offset, g.row_indices, g.src_start, gs, x_r, x_l, att, 0.5,
        heads, pre, pre_att)
    assert mag_att.max() < 2.0 ** 19
    assert (ref_att.astype(np.float32) == ref_att).all()
    name = f"grid bf16 csc K={heads} C={c_per} {form}"
    got, got_att = _run_backward(gpu, "csc", form, heads, Inp16(dev, r_bits),
                                 Inp16(dev, l_bits), x_r.shape, att, gs, pre,
                                 pre_att, 0.5, True, True, name)
    _assert_bits(got_att, ref_att.astype(np.float32), name + " grad_att")
    _assert_bits(got, ref.astype(np.float32), name + " grad_own")


# --------------------------------------------------------------------------
# nothing to do, invalid heads
# --------------------------------------------------------------------------
def test_nothing_to_do_writes_nothing(gpu):
    """A batch whose destinations all have degree 0, edges = 0 and
    batch_size = 0 leave the prefilled outputs of every new entry
    bit-unchanged."""
    g = R.empty_graph()
    dev, st = gpu["dev"], gpu["s"]
    assert g.edges == 0 and g.batch == 7
    rng = np.random.default_rng(6300)
    coff, rows = _up32(dev, g.column_offset), _up32(dev, g.row_indices)
    heads, c_per = 4, 3
    f = heads * c_per
    inp = Inp(dev, rng.normal(size=(32, f)))
    inp16 = Inp16(dev, round_bf16(rng.normal(size=(32, f))))
    mk = lambda *shape: Buf(dev, shape, rng.normal(size=shape) + 1)
    cp, rp = coff.data_ptr(), rows.data_ptr()
    s, e = g.src_start, g.src_start + g.v_src
    for batch, edges, cp_ in ((g.batch, 0, cp), (0, 0, cp),
                              (0, 5, gpu["coff"].data_ptr())):
        for k in (heads, 1):
            a = mk(g.batch, f)
            st.gather_by_dst_from_src_heads_bf16(
                inp16.ptr, a.ptr, inp.ptr, rp, cp_, s, e, s, s + g.batch,
                edges, batch, f, k)
            a.assert_untouched("gather_by_dst_from_src_heads_bf16")
            a = mk(g.batch, f)
            st.gather_by_src_from_dst_heads_bf16(
                inp16.ptr, a.ptr, inp.ptr, cp_, rp, s, s + g.batch, s, e,
                edges, batch, f, k)
            a.assert_untouched("gather_by_src_from_dst_heads_bf16")
            a = mk(8, k)
            st.edge_dot_heads_bf16(a.ptr, inp.ptr, inp16.ptr, rp, cp_, s,
                                   batch, edges, f, k)
            a.assert_untouched("edge_dot_heads_bf16")
        a = mk(8, heads)
        st.edge_gatv2_score_bf16(a.ptr, inp16.ptr, inp16.ptr, inp.ptr, SLOPE,
                                 rp, cp_, s, batch, edges, f, heads)
        a.assert_untouched("edge_gatv2_score_bf16")
        a, b = mk(g.batch, f), mk(f)
        st.edge_gatv2_backward_bf16(a.ptr, b.ptr, inp.ptr, inp16.ptr,
                                    inp16.ptr, inp.ptr, SLOPE, cp_, rp, s,
                                    batch, edges, f, heads)
        a.assert_untouched("edge_gatv2_backward_bf16 grad_own")
        b.assert_untouched("edge_gatv2_backward_bf16 grad_att")


def test_invalid_heads_raise_in_the_binding(gpu):
    st = gpu["s"]
    for f, heads in ((32, 5), (4, 8), (32, 0)):
        with pytest.raises(ValueError):
            st.gather_by_dst_from_src_heads_bf16(0, 0, 0, 0, 0, 0, 1, 0, 1, 1,
                                                 1, f, heads)
        with pytest.raises(ValueError):
            st.gather_by_src_from_dst_heads_bf16(0, 0, 0, 0, 0, 0, 1, 0, 1, 1,
                                                 1, f, heads)
        with pytest.raises(ValueError):
            st.edge_dot_heads_bf16(0, 0, 0, 0, 0, 0, 1, 1, f, heads)
        with pytest.raises(ValueError):
            st.edge_gatv2_score_bf16(0, 0, 0, 0, SLOPE, 0, 0, 0, 1, 1, f,
                                     heads)
        with pytest.raises(ValueError):
            st.edge_gatv2_backward_bf16(0, 0, 0, 0, 0, 0, SLOPE, 0, 0, 0, 1, 1,
                                        f, heads)
        with pytest.raises(ValueError):
            gpu["shim"].gather_plan_heads_bf16(f, heads, 16, 1, 1)
