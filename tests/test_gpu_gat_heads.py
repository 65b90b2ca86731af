"""Multi-head GAT on the GPU (marked gpu): the heads gathers, the K-head
attention forward, the per-head edge dot and the K-column weight sum against
the float64 references of tests/heads_ref.py, and gat.GATLayer(heads=K) with
gat.attend against an independent dense-index torch layer.

The kernel cases run on edge_ref.edge_case_graph (about 22k edges; degrees on
both sides of 64 and 256 and their multiples, a degree-5000 hub, zero degrees
at both ends and in the middle, src_start = 1000, a shuffled mirror map onto
fewer rows than sources); the split is assumed to be the default of 256.
Buffers follow tests/test_gpu_edge_kernels.py: every output sits between two
guard bands of sentinel floats that must come back bit-unchanged, an output
the op must fully write starts as NaN, one it adds to starts from random
non-zero values that the reference includes.

Bounds, none taken from what the kernels give (the file-header rules of
test_gpu_edge_kernels.py): copies and single fp32 adds are exact; sums of
signed terms are held to 1e-4*|ref| + 1e-4*mag with mag the sum of the
absolute terms, prefill included; softmax outputs to a purely relative
1e-4*|ref| (derivation at test_softmax_forward there; |leaky_relu(m)| <= 20
here as in test_attention_forward); per-head dots to 1e-5 + 1e-4*mag with the
head's own mag, as test_edge_dot (at most 128 terms per head here).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = np.float32(-12345.678)
SLOPE = 0.2


# --------------------------------------------------------------------------
# buffers and comparisons (the pattern of test_gpu_edge_kernels.py; `shift`
# moves the body off its 256-byte alignment by that many floats)
# --------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Buf:
    """A float32 device buffer of `shape` between two guard bands; filled
    with NaN, or with `fill`."""

    def __init__(self, dev, shape, fill=None, shift=0):
        shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.shape, self.n = shape, int(np.prod(shape))
        self.lo = GUARD + shift
        host = np.full(self.n + 2 * GUARD + shift, SENTINEL, dtype=np.float32)
        body = host[self.lo:self.lo + self.n]
        body[:] = np.nan if fill is None else np.asarray(
            fill, dtype=np.float32).reshape(-1)
        self.before = host
        self.t = torch.from_numpy(host.copy()).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * self.lo

    @property
    def prefill(self):
        return self.before[self.lo:self.lo + self.n].reshape(self.shape)

    def read(self, name):
        torch.cuda.synchronize()
        after = self.t.cpu().numpy()
        for side, sl in (("front", slice(0, self.lo)),
                         ("back", slice(self.lo + self.n, None))):
            assert (_bits(after[sl]) == _bits(self.before[sl])).all(), (
                f"{name}: {side} guard band overwritten")
        return after[self.lo:self.lo + self.n].reshape(self.shape)

    def assert_untouched(self, name):
        got = self.read(name)
        assert (_bits(got) == _bits(self.prefill)).all(), (
            f"{name}: written although there was nothing to do")


class Inp:
    """A float32 device input whose first element sits `shift` floats past
    the allocation's alignment."""

    def __init__(self, dev, a, shift=0):
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        self.t = torch.from_numpy(
            np.concatenate([np.zeros(shift, dtype=np.float32), a])).to(dev)
        self.ptr = self.t.data_ptr() + 4 * shift


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


def _up32(dev, a):
    return torch.from_numpy(
        np.array(a, dtype=np.uint32).view(np.int32)).to(dev)


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    g = R.edge_case_graph()
    perm, pos = R.csc_to_csr(g.row_indices)
    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    env = {"dev": dev, "shim": shim, "s": shim.Stream.wrap_torch_current(),
           "general": shim.Stream.wrap_torch_current(),
           "coff": _up32(dev, g.column_offset), "rows": _up32(dev, g.row_indices),
           "mi": _up32(dev, g.mirror_index), "pos": _up32(dev, pos),
           "roff": _up32(dev, roff),
           "cidx": _up32(dev, _csr_topology()[1])}
    env["general"].heads_dbg_general(1)
    yield env
    env["general"].destroy()


def _stream(gpu, form):
    """`general`: a stream on which the heads edge entries run their general
    kernel forms even where the shape has a faster one."""
    return gpu["general"] if form == "general" else gpu["s"]


def test_graph_coverage():
    R.assert_coverage(R.edge_case_graph())


# --------------------------------------------------------------------------
# heads gather, both directions
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _csr_topology():
    """(row_offset, column_indices holding global destination ids, perm): the
    edges of the edge-case graph grouped by source; destination d is global
    vertex src_start + d, so dst_start = src_start."""
    g = R.edge_case_graph()
    perm, _ = R.csc_to_csr(g.row_indices)
    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    cidx = (g.src_start + g.dst_of_edge[perm]).astype(np.uint32)
    return roff, cidx, perm


def _topology(direction):
    """(offset, nbr, nbr_start, gathered rows, output rows)"""
    g = R.edge_case_graph()
    if direction == "fwd":
        return g.column_offset, g.row_indices, g.src_start, g.v_src, g.batch
    roff, cidx, _ = _csr_topology()
    return roff, cidx, g.src_start, g.batch, g.v_src


GATHER_CASES = [(8, 16),   # 4-wide lanes
                (4, 6),    # 2-wide lanes: C % 4 != 0 although f % 4 == 0
                (3, 7),    # strided; heads change inside a lane's 4 elements
                (5, 33),   # f = 165: a head boundary inside a 64-lane stride
                (8, 64),   # f = 512: two slabs
                (16, 1),   # C = 1, the tensor_weight form
                (1, 33)]   # one head on a ragged width


@functools.lru_cache(maxsize=None)
def _gather_case(heads, c_per, direction, equal_weights=False):
    g = R.edge_case_graph()
    off, nbr, start, n_in, n_out = _topology(direction)
    f = heads * c_per
    rng = np.random.default_rng([7000, heads, c_per, int(direction == "bwd"),
                                 int(equal_weights)])
    x = rng.uniform(-1, 1, (n_in, f)).astype(np.float32)
    if equal_weights:
        w = np.repeat(rng.uniform(-1, 1, (g.edges, 1)), heads, axis=1)
    else:
        w = rng.uniform(-1, 1, (g.edges, heads))
    w = np.ascontiguousarray(w, dtype=np.float32)
    pre = (rng.normal(size=(n_out, f)) + 3).astype(np.float32)
    assert (pre != 0).all()
    ref, mag = H.gather(off, nbr, start, x, w, heads, pre)
    for a in (x, w, pre, ref, mag):
        a.setflags(write=False)
    return x, w, pre, ref, mag


def _run_gather(gpu, direction, x, w, pre, heads, shift=0, scalar=False,
                name="gather"):
    """One launch of the heads entry (or, scalar=True, of the scalar entry
    with w as its per-edge weight) onto `pre`; returns the output."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], gpu["s"]
    _, _, start, n_in, n_out = _topology(direction)
    f = x.shape[1]
    d_x, d_w = Inp(dev, x, shift), Inp(dev, w)
    out = Buf(dev, (n_out, f), pre, shift)
    if direction == "fwd":
        entry = (st.gather_by_dst_from_src if scalar
                 else st.gather_by_dst_from_src_heads)
        args = (d_x.ptr, out.ptr, d_w.ptr, gpu["rows"].data_ptr(),
                gpu["coff"].data_ptr(), start, start + n_in, start,
                start + n_out, g.edges, n_out, f)
    else:
        entry = (st.gather_by_src_from_dst if scalar
                 else st.gather_by_src_from_dst_heads)
        args = (d_x.ptr, out.ptr, d_w.ptr, gpu["roff"].data_ptr(),
                gpu["cidx"].data_ptr(), start, start + n_out, start,
                start + n_in, g.edges, n_out, f)
    entry(*args, True if scalar else heads)
    return out.read(name)


def _unsplit_rows(direction):
    off = _topology(direction)[0].astype(np.int64)
    return np.diff(off) <= R.SPLIT


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("heads,c_per", GATHER_CASES)
def test_gather_heads(gpu, heads, c_per, direction, shift):
    """output[v, c] += sum_e w[e, c // C] * input[nbr(e), c] onto a non-zero
    prefill, with weights uniform in [-1, 1].  shift = 1 moves the input and
    output pointers one float off, so that only 4-byte alignment is left and
    the strided path runs at every width.  Rows without edges stay
    bit-unchanged, and the launch is reported as NTS_SCHED_ITEM."""
    x, w, pre, ref, mag = _gather_case(heads, c_per, direction)
    name = f"gather {direction} K={heads} C={c_per} shift={shift}"
    f = heads * c_per
    want = 1 if shift else (4 if c_per % 4 == 0 else 2 if c_per % 2 == 0 else 1)
    off = _topology(direction)[0]
    plan = gpu["shim"].gather_plan_heads(f, heads, 4 if shift else 256,
                                         len(off) - 1, int(off[-1]))
    assert plan["vector_width"] == want, plan
    got = _run_gather(gpu, direction, x, w, pre, heads, shift, name=name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    empty = np.diff(off.astype(np.int64)) == 0
    assert empty.any()
    _assert_bits(got[empty], pre[empty], name + ", rows without edges")
    if heads > 1:
        assert gpu["s"].gather_schedule_last()[0] == 0


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_gather_one_head_is_the_scalar_entry(gpu, direction):
    """heads = 1 delegates to the scalar gather's launch (read in
    launch_gather_heads); what can be observed is the same result on the same
    prefill, bit for bit on rows of at most 256 edges.  Split rows merge by
    atomics in an order that varies from launch to launch and are held to
    the bound."""
    x, w, pre, ref, mag = _gather_case(1, 33, direction)
    name = f"gather {direction} K=1 against the scalar entry"
    got = _run_gather(gpu, direction, x, w, pre, 1, name=name)
    base = _run_gather(gpu, direction, x, w, pre, 1, scalar=True, name=name)
    one = _unsplit_rows(direction)
    assert one.any()
    _assert_bits(got[one], base[one], name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)


@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("heads,c_per", [(4, 6), (3, 7), (5, 33), (8, 16)])
def test_gather_equal_weights_against_scalar_entry(gpu, heads, c_per,
                                                   direction):
    """With the same weight in every head the heads gather computes what the
    scalar entry computes with that weight column.  At C = 6, 7, 33 the
    scalar entry runs a wider lane or the strided path, another instruction
    sequence, so the two are held to the bound; at (8, 16) both run 4-wide
    lanes and the same per-element fmaf chain in edge order, so rows of at
    most 256 edges are bit-equal."""
    x, w, pre, ref, mag = _gather_case(heads, c_per, direction, True)
    assert (w == w[:, :1]).all()
    name = f"gather {direction} K={heads} C={c_per}, equal weights"
    got = _run_gather(gpu, direction, x, w, pre, heads, name=name)
    base = _run_gather(gpu, direction, x, np.ascontiguousarray(w[:, 0]), pre,
                       heads, scalar=True, name=name + " (scalar entry)")
    bound = 1e-4 * np.abs(ref) + 1e-4 * mag
    _assert_bound(got, ref, bound, name)
    _assert_bound(got, base.astype(np.float64), bound, name + " vs scalar")
    if (heads, c_per) == (8, 16):
        one = _unsplit_rows(direction)
        assert one.any()
        _assert_bits(got[one], base[one], name + ", unsplit rows")


# --------------------------------------------------------------------------
# attention forward, K heads
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attention_case(heads, with_mirror):
    g = R.edge_case_graph()
    per_head = [R.attention_inputs(g, seed=k) for k in range(heads)]
    full, mirror, s_dst = (np.ascontiguousarray(
        np.stack([p[i] for p in per_head], axis=1)) for i in range(3))
    s_src = mirror if with_mirror else full
    m_ref, s_ref = H.attention_forward(
        g.column_offset, g.row_indices, s_src, s_dst,
        g.mirror_index if with_mirror else None, SLOPE)
    return s_src, s_dst, m_ref, s_ref


@pytest.mark.parametrize("with_perm", [True, False])
@pytest.mark.parametrize("with_mirror", [True, False])
@pytest.mark.parametrize("heads,form", [(2, "auto"), (3, "auto"), (8, "auto"),
                                        (2, "general"), (8, "general"),
                                        (1, "auto"), (1, "general")])
def test_attention_forward_heads(gpu, heads, form, with_mirror, with_perm):
    """Per head the inputs of test_attention_forward (seed = head), m exactly
    0 on some edges.  m_sum_out is one fp32 add: bit-equal to numpy float32.
    The softmax is within 1e-4*|ref|; its permuted copy is bit-equal to it
    moved through the slot map; each (destination, head) with edges sums to 1
    within 1e-4."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    s_src, s_dst, m_ref, s_ref = _attention_case(heads, with_mirror)
    assert (m_ref == 0).any() and m_ref.min() < -15 and m_ref.max() > 15
    pos = R.csc_to_csr(g.row_indices)[1]
    name = (f"attention fwd K={heads} {form} mirror={with_mirror} "
            f"perm={with_perm}")
    d_src, d_dst = Inp(dev, s_src), Inp(dev, s_dst)
    shape = (g.edges, heads)
    out, msum = Buf(dev, shape), Buf(dev, shape)
    out2 = Buf(dev, shape) if with_perm else None
    st.edge_attention_forward_heads(
        out.ptr, out2.ptr if out2 else None,
        gpu["pos"].data_ptr() if out2 else None, msum.ptr, d_src.ptr,
        d_dst.ptr, gpu["rows"].data_ptr(),
        gpu["mi"].data_ptr() if with_mirror else None, SLOPE,
        gpu["coff"].data_ptr(), g.batch, g.edges, heads)
    got_m = msum.read(name)
    assert np.isfinite(got_m).all(), f"{name}: m_sum slot not written"
    _assert_bits(got_m, m_ref, name + " m_sum")
    got = out.read(name)
    _assert_bound(got, s_ref, 1e-4 * np.abs(s_ref), name + " softmax")
    total = R.segment_sum(got, g.column_offset)
    live = g.deg > 0
    assert np.abs(total[live] - 1).max() <= 1e-4, name + " sums to 1"
    if out2 is not None:
        got2 = out2.read(name)
        assert np.isfinite(got2).all(), f"{name}: permuted slot not written"
        _assert_bits(got2[pos], got, name + " permuted output")


# --------------------------------------------------------------------------
# per-head edge dot
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _dot_case(heads, c_per):
    g = R.edge_case_graph()
    f = heads * c_per
    rng = np.random.default_rng([8000, heads, c_per])
    a = rng.uniform(-1, 1, (g.batch, f)).astype(np.float32)
    b = rng.uniform(-1, 1, (g.v_src, f)).astype(np.float32)
    return (a, b) + H.edge_dot(g.column_offset, g.row_indices, g.src_start,
                               a, b, heads)


@pytest.mark.parametrize("heads,c_per,form,shift", [
    # segmented butterfly, 4 columns per lane: 4, 16 and 32 lanes per head;
    # a 12-lane row in a 16-lane group; two 64-lane steps per row
    (8, 16, "auto", 0), (2, 64, "auto", 0), (2, 128, "auto", 0),
    (3, 16, "auto", 0), (8, 64, "auto", 0),
    # 2 columns per lane and 1, by the width and by the pointers' alignment
    (16, 2, "auto", 0), (16, 1, "auto", 0), (8, 16, "auto", 2),
    (8, 16, "auto", 1),
    (4, 6, "auto", 0), (3, 7, "auto", 0),  # general loop
    (1, 33, "auto", 0),                    # the single-head kernel
    (1, 33, "general", 0),
    (8, 16, "general", 0), (2, 64, "general", 0), (2, 128, "general", 0)])
def test_edge_dot_heads(gpu, heads, c_per, form, shift):
    """out[e, k] = dst_rows[dst, head k] . src_rows[src - src_start, head k].
    shift moves both row pointers that many floats off their alignment.
    Bound as test_edge_dot, per head with that head's mag: 1e-5 +
    1e-4*sum_j|a_j b_j|; a head has at most 128 terms, whose fp32 error is
    at most 128*2^-24 = 7.6e-6 of that sum in any order."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    a, b, ref, mag = _dot_case(heads, c_per)
    name = f"edge_dot K={heads} C={c_per} {form} shift={shift}"
    d_a, d_b = Inp(dev, a, shift), Inp(dev, b, shift)
    out = Buf(dev, (g.edges, heads))
    st.edge_dot_heads(out.ptr, d_a.ptr, d_b.ptr, gpu["rows"].data_ptr(),
                      gpu["coff"].data_ptr(), g.src_start, g.batch, g.edges,
                      heads * c_per, heads)
    _assert_bound(out.read(name), ref, 1e-5 + 1e-4 * mag, name)


# --------------------------------------------------------------------------
# K-column weight sum
# --------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["csc", "csr"])
@pytest.mark.parametrize("heads,form", [(2, "auto"), (3, "auto"), (8, "auto"),
                                        (2, "general"), (8, "general"),
                                        (1, "auto"), (1, "general")])
def test_weight_sum_heads(gpu, heads, form, order):
    """out[v, k] += sum of signed weights[e, k] over v's edge range, onto a
    non-zero prefill; over the CSC offsets (split destinations) and the CSR
    offsets.  Bound 1e-4*|ref| + 1e-4*mag; vertices without edges stay
    bit-unchanged."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    off = g.column_offset if order == "csc" else _csr_topology()[0]
    d_off = gpu["coff"] if order == "csc" else gpu["roff"]
    n = len(off) - 1
    rng = np.random.default_rng([9000, heads, int(order == "csr")])
    w = rng.normal(size=(g.edges, heads)).astype(np.float32)
    pre = (rng.normal(size=(n, heads)) + 2).astype(np.float32)
    ref, mag = H.weight_sum(off, w, pre)
    name = f"weight_sum K={heads} {form} {order}"
    d_w = Inp(dev, w)
    out = Buf(dev, (n, heads), pre)
    st.weight_sum_heads(out.ptr, d_w.ptr, d_off.data_ptr(), n, g.edges, heads)
    got = out.read(name)
    _assert_bound(got, ref, 1e-4 * np.abs(ref) + 1e-4 * mag, name)
    zero = np.diff(off.astype(np.int64)) == 0
    assert zero.any()
    _assert_bits(got[zero], pre[zero], name + " at degree 0")


# --------------------------------------------------------------------------
# one head against the scalar entries
# --------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["auto", "general"])
def test_one_head_is_the_scalar_entries(gpu, form):
    """At K = 1 the three heads edge entries compute what
    nts_edge_attention_forward, nts_weight_sum and nts_edge_dot compute, bit
    for bit wherever no atomic merge is involved: m_sum and the dot on every
    edge, the softmax on the edges of destinations of at most 256 edges, the
    weight sum on those destinations.  Split destinations merge by fp32
    atomics in an order that varies from launch to launch and stay under the
    bounds of test_attention_forward_heads and test_weight_sum_heads."""
    g = R.edge_case_graph()
    dev, st = gpu["dev"], _stream(gpu, form)
    one = g.deg <= R.SPLIT
    one_e = one[g.dst_of_edge]
    assert one.any() and not one.all()
    name = f"K=1 {form} against the scalar entry: "

    s_src, s_dst, m_ref, s_ref = _attention_case(1, True)
    d_src, d_dst = Inp(dev, s_src), Inp(dev, s_dst)
    got = []
    for heads_entry in (True, False):
        out, msum, out2 = (Buf(dev, (g.edges, 1)) for _ in range(3))
        args = (out.ptr, out2.ptr, gpu["pos"].data_ptr(), msum.ptr, d_src.ptr,
                d_dst.ptr, gpu["rows"].data_ptr(), gpu["mi"].data_ptr(), SLOPE,
                gpu["coff"].data_ptr(), g.batch)
        if heads_entry:
            st.edge_attention_forward_heads(*args, g.edges, 1)
        else:
            st.edge_attention_forward(*args)
        got.append([b.read(name + "attention") for b in (out, msum, out2)])
    (out_h, msum_h, out2_h), (out_s, msum_s, out2_s) = got
    _assert_bits(msum_h, msum_s, name + "m_sum")
    _assert_bits(out_h[one_e], out_s[one_e], name + "softmax, unsplit")
    pos = R.csc_to_csr(g.row_indices)[1]
    _assert_bits(out2_h[pos][one_e], out2_s[pos][one_e],
                 name + "permuted softmax, unsplit")
    _assert_bound(out_h, s_ref, 1e-4 * np.abs(s_ref), name + "softmax")

    rng = np.random.default_rng(9100)
    w = rng.normal(size=(g.edges, 1)).astype(np.float32)
    pre = (rng.normal(size=(g.batch, 1)) + 2).astype(np.float32)
    ref, mag = H.weight_sum(g.column_offset, w, pre)
    d_w = Inp(dev, w)
    out_h, out_s = Buf(dev, (g.batch, 1), pre), Buf(dev, (g.batch, 1), pre)
    st.weight_sum_heads(out_h.ptr, d_w.ptr, gpu["coff"].data_ptr(), g.batch,
                        g.edges, 1)
    st.weight_sum(out_s.ptr, d_w.ptr, gpu["coff"].data_ptr(), g.batch)
    got_h, got_s = out_h.read(name + "weight_sum"), out_s.read(name)
    _assert_bits(got_h[one], got_s[one], name + "weight_sum, unsplit")
    _assert_bound(got_h, ref, 1e-4 * np.abs(ref) + 1e-4 * mag,
                  name + "weight_sum")

    a, b, ref, mag = _dot_case(1, 33)
    d_a, d_b = Inp(dev, a), Inp(dev, b)
    out_h, out_s = Buf(dev, (g.edges, 1)), Buf(dev, (g.edges, 1))
    st.edge_dot_heads(out_h.ptr, d_a.ptr, d_b.ptr, gpu["rows"].data_ptr(),
                      gpu["coff"].data_ptr(), g.src_start, g.batch, g.edges,
                      33, 1)
    st.edge_dot(out_s.ptr, d_a.ptr, d_b.ptr, gpu["rows"].data_ptr(),
                gpu["coff"].data_ptr(), g.src_start, g.batch, 33)
    _assert_bits(out_h.read(name + "edge_dot"), out_s.read(name),
                 name + "edge_dot")


# --------------------------------------------------------------------------
# nothing to do
# --------------------------------------------------------------------------
def test_zero_degree_batch_writes_nothing(gpu):
    """On a batch whose destinations all have degree 0 the six heads entries
    leave their prefilled outputs bit-unchanged."""
    g = R.empty_graph()
    dev, st = gpu["dev"], gpu["s"]
    assert g.edges == 0 and g.batch == 7
    rng = np.random.default_rng(6100)
    coff, rows = _up32(dev, g.column_offset), _up32(dev, g.row_indices)
    mi = _up32(dev, g.mirror_index)
    heads, c_per = 4, 3
    f = heads * c_per
    inp = Inp(dev, rng.normal(size=(32, f)))
    idx = _up32(dev, np.arange(16))
    mk = lambda *shape: Buf(dev, shape, rng.normal(size=shape) + 1)
    cp, rp = coff.data_ptr(), rows.data_ptr()
    s, e = g.src_start, g.src_start + g.v_src

    a = mk(g.batch, f)
    st.gather_by_dst_from_src_heads(inp.ptr, a.ptr, inp.ptr, rp, cp, s, e, s,
                                    s + g.batch, 0, g.batch, f, heads)
    a.assert_untouched("gather_by_dst_from_src_heads")
    a = mk(g.batch, f)
    st.gather_by_src_from_dst_heads(inp.ptr, a.ptr, inp.ptr, cp, rp, s,
                                    s + g.batch, s, e, 0, g.batch, f, heads)
    a.assert_untouched("gather_by_src_from_dst_heads")
    a, b, c = mk(8, heads), mk(8, heads), mk(8, heads)
    st.edge_attention_forward_heads(a.ptr, b.ptr, idx.data_ptr(), c.ptr,
                                    inp.ptr, inp.ptr, rp, mi.data_ptr(), SLOPE,
                                    cp, g.batch, 0, heads)
    for buf in (a, b, c):
        buf.assert_untouched("edge_attention_forward_heads")
    a = mk(8, heads)
    st.edge_dot_heads(a.ptr, inp.ptr, inp.ptr, rp, cp, s, g.batch, 0, f, heads)
    a.assert_untouched("edge_dot_heads")
    a = mk(g.batch, heads)
    st.weight_sum_heads(a.ptr, inp.ptr, cp, g.batch, 0, heads)
    a.assert_untouched("weight_sum_heads")


# --------------------------------------------------------------------------
# the layer and autograd
# --------------------------------------------------------------------------
RTOL, ATOL = 1e-4, 2e-5   # of tests/test_gpu_gat_layer.py


def _assert_close(got, ref, name):
    got = got.detach().cpu().numpy().astype(np.float64)
    ref = ref.detach().cpu().numpy().astype(np.float64)
    err = np.abs(got - ref)
    bound = RTOL * np.abs(ref) + ATOL
    print(f"{name}: worst {float((err / bound).max()):.3e} of the tolerance")
    bad = err > bound
    assert not bad.any(), (f"{name}: {bad.sum()}/{bad.size} out of tol, "
                           f"worst {err.max():.3e}")


@functools.lru_cache(maxsize=None)
def _layer_chunk():
    from neutronstarlite_amd import graph as G
    v, e = 1200, 20000
    edges = G.rmat_edges(v, e, seed=13)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    return v, G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]


def torch_heads_reference(h, a_src, a_dst, dst_of_edge, src_of_edge, v, heads,
                          slope):
    """Independent dense-index multi-head GAT layer under torch autograd, in
    the dtype of h, with the no-max-subtraction softmax of the kernels."""
    h3 = h.view(v, heads, -1)
    s_src = (h3 * a_src).sum(-1)
    s_dst = (h3 * a_dst).sum(-1)
    e = torch.nn.functional.leaky_relu(
        s_src[src_of_edge] + s_dst[dst_of_edge], slope)
    ex = torch.exp(e)
    den = torch.zeros_like(s_dst).index_add_(0, dst_of_edge, ex)
    s = ex / den[dst_of_edge]
    y = torch.zeros_like(h3).index_add_(
        0, dst_of_edge, s.unsqueeze(2) * h3[src_of_edge])
    return y.view(v, -1)


@pytest.mark.parametrize("heads,c_per", [(4, 8), (8, 16), (3, 11), (2, 128)])
def test_layer_attend_autograd(heads, c_per):
    """gat.attend under autograd with a_src, a_dst of shape [K, C], against
    the dense-index layer computed in float64 from the same float32 inputs:
    y, grad h, grad a_src, grad a_dst.  A per-head sum has at most 128
    terms; the single-head cases of test_gpu_gat_layer.py hold sums of up to
    256 terms to this tolerance."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    f = heads * c_per
    rng = np.random.default_rng([5, heads, c_per])
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    h0 = up(rng.uniform(-1, 1, size=(v, f)))
    a_src0 = up(rng.uniform(-1, 1, size=(heads, c_per)))
    a_dst0 = up(rng.uniform(-1, 1, size=(heads, c_per)))
    gy = up(rng.uniform(-1, 1, size=(v, f)))

    layer = gat.GATLayer(ch, v, dev, heads=heads)
    h, a_src, a_dst = (t.clone().requires_grad_(True)
                       for t in (h0, a_src0, a_dst0))
    h3 = h.view(v, heads, c_per)
    y = gat.attend(h, (h3 * a_src).sum(-1), (h3 * a_dst).sum(-1), layer, SLOPE)
    assert y.shape == (v, f)
    y.backward(gy)

    hr, ar, dr = (t.double().requires_grad_(True)
                  for t in (h0, a_src0, a_dst0))
    y_ref = torch_heads_reference(hr, ar, dr, layer.dst_of_edge,
                                  layer.src_of_edge, v, heads, SLOPE)
    y_ref.backward(gy.double())
    tag = f"K={heads} C={c_per}"
    _assert_close(y, y_ref, f"attend y {tag}")
    _assert_close(h.grad, hr.grad, f"attend grad h {tag}")
    _assert_close(a_src.grad, ar.grad, f"attend grad a_src {tag}")
    _assert_close(a_dst.grad, dr.grad, f"attend grad a_dst {tag}")


def test_layer_backward_shapes_and_one_head_equals_default():
    """GATLayer(..., heads=1) makes the calls of the default constructor: on
    destinations of at most 256 in-edges (one work item, nothing depends on
    the order of atomics) y and g_dst are bit-equal; every result has the
    default's shape.  A K-head backward returns [V, K*C], [V, K], [V, K]."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    f = 32
    rng = np.random.default_rng(6)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    h, gy = (up(rng.uniform(-1, 1, size=(v, f))) for _ in range(2))
    a_src, a_dst = (up(rng.uniform(-1, 1, size=f)) for _ in range(2))
    results = []
    for layer in (gat.GATLayer(ch, v, dev), gat.GATLayer(ch, v, dev, heads=1)):
        y, saved = layer.forward(h, h @ a_src, h @ a_dst, SLOPE)
        results.append((y,) + tuple(layer.backward(gy, saved, SLOPE)))
    torch.cuda.synchronize()
    one = torch.from_numpy(
        np.diff(ch.column_offset.astype(np.int64)) <= R.SPLIT).to(dev)
    assert bool(one.any())
    for a, b in zip(*results):
        assert a.shape == b.shape
    for i, name in ((0, "y"), (3, "g_dst")):
        a, b = results[0][i][one], results[1][i][one]
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name

    heads = 4
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    s = up(rng.uniform(-1, 1, size=(v, heads)))
    y, saved = layer.forward(h, s, s.clone(), SLOPE)
    grad_h, g_src, g_dst = layer.backward(gy, saved, SLOPE)
    assert y.shape == (v, f) and grad_h.shape == (v, f)
    assert g_src.shape == (v, heads) and g_dst.shape == (v, heads)


def test_layer_input_checks():
    """Raised before anything is launched: the kernels take raw pointers."""
    from neutronstarlite_amd import gat
    dev = torch.device("cuda:0")
    v, ch = _layer_chunk()
    heads = 4
    layer = gat.GATLayer(ch, v, dev, heads=heads)
    h = torch.zeros(v, 32, device=dev)
    s = torch.zeros(v, heads, device=dev)
    with pytest.raises(ValueError):          # f % K != 0
        layer.forward(torch.zeros(v, 30, device=dev), s, s)
    with pytest.raises(ValueError):          # s_src of the single-head shape
        layer.forward(h, torch.zeros(v, device=dev), s)
    with pytest.raises(ValueError):          # s_dst with too few heads
        layer.forward(h, s, torch.zeros(v, 2, device=dev))
    with pytest.raises(ValueError):          # not contiguous
        layer.forward(torch.zeros(32, v, device=dev).t(), s, s)
    with pytest.raises(TypeError):           # not float32
        layer.forward(h.double(), s, s)
    with pytest.raises(TypeError):
        layer.forward(h, s.to(torch.bfloat16), s)
    with pytest.raises(TypeError):           # not on the device
        layer.forward(h.cpu(), s, s)
    with pytest.raises(ValueError):
        gat.GATLayer(ch, v, dev, heads=0)
    with pytest.raises(ValueError):          # checked by the binding
        layer.stream.gather_by_dst_from_src_heads(
            0, 0, 0, 0, 0, 0, v, 0, v, 1, v, 32, 5)
    y, saved = layer.forward(h, s, s)
    with pytest.raises(ValueError):          # grad_y of another width
        layer.backward(torch.zeros(v, 16, device=dev), saved)
