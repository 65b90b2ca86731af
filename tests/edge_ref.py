"""Plain float64 numpy references for the item-driven GAT edge kernels, and
the edge-case graph they are tested on.  A helper module: no tests here.

Every reference takes the CSC arrays (column_offset, row_indices: uint32,
row_indices holding GLOBAL source ids) and float32 inputs, computes in
float64 and returns float64.  Where a test's bound needs the size of the
computation, the function also returns `mag`, the sum of the absolute values
of the terms that were added (prefill included).

Semantics (pinned against oracle.c by tests/test_edge_ref.py):
  scatter_src_to_msg, scatter_dst_to_msg, softmax fwd/bwd   overwrite
  gather_msg_to_src, gather_msg_to_dst, scatter_grad_back   accumulate
"""
import functools
from types import SimpleNamespace

import numpy as np

SPLIT = 256  # default max edges per work item (NTS_SPLIT)
LANES = 64   # lanes that stride one item

# in-degrees that must each occur on one destination: around the lane stride,
# around the split and its multiples, a short last item (1000 = 3*256 + 232)
EDGE_DEGREES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 255, 256, 257,
                511, 512, 513, 1000)
HUB_DEGREE = 5000


# --------------------------------------------------------------------------
# graphs
# --------------------------------------------------------------------------
def build_graph(degrees, v_src, src_start, seed, forced=()):
    """CSC arrays of a graph with the given in-degree per destination.

    Sources are uniform over [src_start, src_start + v_src); destination d is
    global vertex src_start + d.  `forced` is a list of (edge slot, global
    source id) written after the draw.  mirror_index maps every referenced
    global source id onto one of M compacted rows, the unique sources being
    shuffled before they are numbered; unreferenced ids map to row 0 (they
    are never looked up)."""
    rng = np.random.default_rng(seed)
    deg = np.asarray(degrees, dtype=np.int64)
    coff = np.zeros(len(deg) + 1, dtype=np.int64)
    np.cumsum(deg, out=coff[1:])
    e = int(coff[-1])
    rows = rng.integers(src_start, src_start + v_src, e)
    for slot, src in forced:
        rows[slot] = src
    uniq = np.unique(rows)
    mirror_index = np.zeros(src_start + v_src, dtype=np.uint32)
    mirror_index[uniq[rng.permutation(len(uniq))]] = np.arange(
        len(uniq), dtype=np.uint32)
    g = SimpleNamespace(
        batch=len(deg), edges=e, v_src=v_src, src_start=src_start,
        deg=deg, column_offset=coff.astype(np.uint32),
        row_indices=rows.astype(np.uint32), mirror_index=mirror_index,
        uniq=uniq, m=len(uniq),
        dst_of_edge=np.repeat(np.arange(len(deg)), deg))
    for a in (g.deg, g.column_offset, g.row_indices, g.mirror_index, g.uniq,
              g.dst_of_edge):
        a.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def edge_case_graph():
    """The graph of tests/test_gpu_edge_kernels.py, about 22k edges:
    zero degree first, last and once in the middle; one destination of each
    degree in EDGE_DEGREES; one hub of HUB_DEGREE; 640 destinations with a
    degree uniform in [0, 40]; one duplicated edge (on the degree-3
    destination) and one self loop (on the degree-5 one); global source ids
    from src_start = 1000; M < v_src compacted mirror rows."""
    rng = np.random.default_rng(20240)
    inner = np.concatenate([np.array(EDGE_DEGREES + (HUB_DEGREE,)),
                            rng.integers(0, 41, 640)])
    inner = inner[rng.permutation(len(inner))]
    mid = len(inner) // 2
    deg = np.concatenate([[0], inner[:mid], [0], inner[mid:], [0]])
    src_start, v_src = 1000, 6000
    off = np.concatenate([[0], np.cumsum(deg)])
    d3 = int(np.flatnonzero(deg == 3)[0])
    d5 = int(np.flatnonzero(deg == 5)[0])
    forced = [(off[d3], src_start + 17), (off[d3] + 1, src_start + 17),
              (off[d5] + 2, src_start + d5)]
    g = build_graph(deg, v_src, src_start, seed=20241, forced=forced)
    g.dup_dst, g.loop_dst = d3, d5
    return g


@functools.lru_cache(maxsize=None)
def small_graph():
    """A second, smaller topology (40 destinations, one of them split)."""
    rng = np.random.default_rng(77)
    deg = rng.integers(0, 9, 40)
    deg[0], deg[7], deg[-1] = 0, 300, 0
    return build_graph(deg, 500, 200, seed=78)


@functools.lru_cache(maxsize=None)
def tiny_graph():
    """Ten destinations, nothing split."""
    return build_graph([0, 1, 2, 0, 70, 5, 64, 3, 1, 0], 50, 3, seed=79)


@functools.lru_cache(maxsize=None)
def empty_graph():
    """A batch whose destinations all have degree 0."""
    return build_graph([0] * 7, 20, 5, seed=80)


def assert_coverage(g):
    """The properties of the edge-case graph that the GPU tests rely on."""
    deg = g.deg
    for d in EDGE_DEGREES + (HUB_DEGREE,):
        assert (deg == d).sum() >= 1, f"no destination of degree {d}"
    assert deg.max() > SPLIT                          # split: atomics on sums
    assert (deg[deg > SPLIT] % SPLIT != 0).any()      # short last item
    assert (deg[deg > SPLIT] % SPLIT == 0).any()      # full last item
    assert ((deg > LANES) & (deg % LANES != 0)).any()  # ragged lane stride
    assert deg[0] == 0 and deg[-1] == 0               # zero degree, both ends
    assert (deg[1:-1] == 0).any()                     # and in the middle
    assert g.src_start != 0
    assert g.row_indices.min() >= g.src_start
    assert g.row_indices.max() < g.src_start + g.v_src
    assert g.m < g.v_src                              # unreferenced sources
    mi = g.mirror_index[g.uniq]
    assert sorted(mi.tolist()) == list(range(g.m))    # onto M rows
    assert (mi != np.arange(g.m)).any()               # not the sorted order
    assert (np.diff(mi.astype(np.int64)) < 0).any()   # shuffled numbering
    off = g.column_offset.astype(np.int64)
    r = g.row_indices
    a = off[g.dup_dst]
    assert r[a] == r[a + 1]                           # duplicated edge
    seg = r[off[g.loop_dst]:off[g.loop_dst + 1]]
    assert (seg == g.src_start + g.loop_dst).any()    # self loop
    assert 20000 <= g.edges <= 24000


# --------------------------------------------------------------------------
# helpers
# --------------------------------------------------------------------------
def _f64(a, f=None):
    a = np.asarray(a, dtype=np.float64)
    return a if f is None else a.reshape(-1, f)


def _dst_of_edge(column_offset):
    off = np.asarray(column_offset, dtype=np.int64)
    return np.repeat(np.arange(len(off) - 1), np.diff(off))


def segment_sum(x, offset):
    """(n_segments, f) float64 sums of the rows of x (E, f) per segment."""
    off = np.asarray(offset, dtype=np.int64)
    x = _f64(x)
    out = np.zeros((len(off) - 1,) + x.shape[1:])
    live = np.diff(off) > 0
    if live.any():
        out[live] = np.add.reduceat(x, off[:-1][live], axis=0)
    return out


# --------------------------------------------------------------------------
# the five edge scatter/gather ops
# --------------------------------------------------------------------------
def scatter_src_to_msg(column_offset, row_indices, mirror_index, mirror):
    """msg[e] = mirror[mirror_index[src(e)]] (overwrite; a pure copy)."""
    rows = np.asarray(mirror_index)[np.asarray(row_indices)].astype(np.int64)
    return _f64(mirror)[rows]


def gather_msg_to_src(column_offset, row_indices, mirror_index, msg, prefill):
    """mirror[mirror_index[src(e)]] += msg[e].  Returns (out, mag)."""
    rows = np.asarray(mirror_index)[np.asarray(row_indices)].astype(np.int64)
    out, mag = _f64(prefill).copy(), np.abs(_f64(prefill))
    np.add.at(out, rows, _f64(msg))
    np.add.at(mag, rows, np.abs(_f64(msg)))
    return out, mag


def scatter_dst_to_msg(column_offset, row_indices, dst_feat):
    """msg[e] = dst_feat[dst(e)] (overwrite; a pure copy)."""
    return _f64(dst_feat)[_dst_of_edge(column_offset)]


def gather_msg_to_dst(column_offset, row_indices, msg, prefill):
    """dst_feat[dst(e)] += msg[e].  Returns (out, mag)."""
    out = _f64(prefill) + segment_sum(msg, column_offset)
    mag = np.abs(_f64(prefill)) + segment_sum(np.abs(_f64(msg)), column_offset)
    return out, mag


def scatter_grad_back_to_msg(column_offset, row_indices, grad, prefill):
    """msg_grad[e] += grad[dst(e)].  Returns (out, mag)."""
    g = _f64(grad)[_dst_of_edge(column_offset)]
    return _f64(prefill) + g, np.abs(_f64(prefill)) + np.abs(g)


# --------------------------------------------------------------------------
# softmax and attention
# --------------------------------------------------------------------------
def softmax_forward(column_offset, x):
    """Per destination and column: exp(x) / sum exp(x), no max subtraction."""
    ex = np.exp(_f64(x))
    return ex / segment_sum(ex, column_offset)[_dst_of_edge(column_offset)]


def softmax_backward(column_offset, g, s, lrelu_in=None, slope=0.0,
                     dst_prefill=None):
    """v[e] = g*s - (sum_e g*s)*s, times (lrelu_in > 0 ? 1 : slope) if given.

    Returns (v, mag) with mag = |g*s| + s*sum|g*s| per edge, and, with
    dst_prefill, also (dsum, dmag): dsum[d] = prefill[d] + sum_e v[e] and
    dmag[d] = |prefill[d]| + sum_e |v[e]| (v of width 1)."""
    doe = _dst_of_edge(column_offset)
    gs = _f64(g) * _f64(s)
    v = gs - segment_sum(gs, column_offset)[doe] * _f64(s)
    mag = np.abs(gs) + _f64(s) * segment_sum(np.abs(gs), column_offset)[doe]
    if lrelu_in is not None:
        v = v * np.where(_f64(lrelu_in) > 0, 1.0, float(np.float32(slope)))
    if dst_prefill is None:
        return v, mag
    p = _f64(dst_prefill).reshape(-1, 1)
    dsum = p + segment_sum(v.reshape(-1, 1), column_offset)
    dmag = np.abs(p) + segment_sum(np.abs(v).reshape(-1, 1), column_offset)
    return v, mag, dsum.reshape(-1), dmag.reshape(-1)


def attention_forward(column_offset, row_indices, s_src, s_dst, mirror_index,
                      slope):
    """m = s_src[mirror_index[src]] + s_dst[dst] (s_src[src] when
    mirror_index is None), leaky-relu, exp, normalize per destination.

    Returns (m, s): m as float32 (one fp32 add, so exactly what the kernel
    must store) and the float64 softmax of leaky_relu(m)."""
    rows = np.asarray(row_indices).astype(np.int64)
    if mirror_index is not None:
        rows = np.asarray(mirror_index)[rows].astype(np.int64)
    ss = np.asarray(s_src, dtype=np.float32).reshape(-1)
    sd = np.asarray(s_dst, dtype=np.float32).reshape(-1)
    m = ss[rows] + sd[_dst_of_edge(column_offset)]
    assert m.dtype == np.float32
    m64 = m.astype(np.float64)
    a = np.where(m64 > 0, m64, float(np.float32(slope)) * m64)
    return m, softmax_forward(column_offset, a.reshape(-1, 1)).reshape(-1)


# --------------------------------------------------------------------------
# weight sum, edge dot, slot maps
# --------------------------------------------------------------------------
def weight_sum(offset, weights, prefill):
    """out[v] += sum of weights over v's edge range.  Returns (out, mag)."""
    w = _f64(weights).reshape(-1, 1)
    p = _f64(prefill).reshape(-1)
    return (p + segment_sum(w, offset).reshape(-1),
            np.abs(p) + segment_sum(np.abs(w), offset).reshape(-1))


def edge_dot(column_offset, row_indices, src_start, dst_rows, src_rows):
    """out[e] = dst_rows[dst(e)] . src_rows[src(e) - src_start].
    Returns (dot, mag) with mag = sum_j |a_j b_j|."""
    doe = _dst_of_edge(column_offset)
    src = np.asarray(row_indices).astype(np.int64) - int(src_start)
    a, b = _f64(dst_rows), _f64(src_rows)
    dot = np.empty(len(src))
    mag = np.empty(len(src))
    for lo in range(0, len(src), 4096):   # bounded temporaries at wide f
        prod = a[doe[lo:lo + 4096]] * b[src[lo:lo + 4096]]
        dot[lo:lo + 4096] = prod.sum(axis=1)
        mag[lo:lo + 4096] = np.abs(prod).sum(axis=1)
    return dot, mag


def csc_to_csr(row_indices):
    """(perm, pos): perm[k] is the CSC slot of the k-th edge in CSR order
    (stable argsort of the sources); pos = its inverse, the CSR slot of CSC
    edge e, so csr[pos[e]] = csc[e] and csr = csc[perm]."""
    perm = np.argsort(np.asarray(row_indices).astype(np.int64), kind="stable")
    pos = np.empty_like(perm)
    pos[perm] = np.arange(len(perm))
    return perm, pos


def csr_offsets(row_indices, src_start, v_src):
    """Row offsets (v_src + 1, uint32) of the same edges grouped by source."""
    cnt = np.bincount(np.asarray(row_indices).astype(np.int64) - src_start,
                      minlength=v_src)
    return np.concatenate([[0], np.cumsum(cnt)]).astype(np.uint32)


# --------------------------------------------------------------------------
# inputs shared by the CPU and the GPU tests
# --------------------------------------------------------------------------
OVERWRITE = ("scatter_src_to_msg", "scatter_dst_to_msg",
             "edge_softmax_forward", "edge_softmax_backward")
ACCUMULATE = ("gather_msg_to_src", "gather_msg_to_dst",
              "scatter_grad_back_to_msg")

SCORE_REGIMES = ("normal", "wide", "equal")


def softmax_scores(regime, e, f, seed=0):
    """(e, f) float32 scores: normal with scale 2, uniform in [-30, 30], or
    all equal (then the softmax is exactly 1/deg)."""
    rng = np.random.default_rng([seed, f, SCORE_REGIMES.index(regime)])
    if regime == "normal":
        x = rng.normal(scale=2.0, size=(e, f))
    elif regime == "wide":
        x = rng.uniform(-30.0, 30.0, size=(e, f))
    else:
        x = np.full((e, f), 1.25)
    return x.astype(np.float32)


def attention_inputs(g, seed=0):
    """(s_src_full, s_src_mirror, s_dst): attention scalars uniform in
    [-10, 10], so m = s_src + s_dst spans about [-20, 20]; on the first edge
    of every fifth live destination s_dst is set to minus that edge's source
    scalar, so m is exactly 0 there.  s_src_full is indexed by global source
    id, s_src_mirror by compacted mirror row; they hold the same values."""
    rng = np.random.default_rng([seed, 5])
    full = rng.uniform(-10, 10, g.src_start + g.v_src).astype(np.float32)
    s_dst = rng.uniform(-10, 10, g.batch).astype(np.float32)
    off = g.column_offset.astype(np.int64)
    for d in np.flatnonzero(g.deg > 0)[::5]:
        s_dst[d] = -full[g.row_indices[off[d]]]
    mirror = np.zeros(g.m, dtype=np.float32)
    mirror[g.mirror_index[g.uniq]] = full[g.uniq]
    return full, mirror, s_dst
