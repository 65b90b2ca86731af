"""Coalesced chunks: nts_coalesce_edges merges a chunk's parallel edges once
and the weighted gathers of HipEngine walk the merged lists.

Two hand-built chunks.  SMALL (50 vertices, destinations 0..39 populated):
an empty list, a list without repeats, one neighbour 7 times, repeats that
are not adjacent in CSC order, 300 copies of one pair (two work items at the
default split of 256 edges, one edge once merged) and short random lists.
WIDE (700 vertices): a list of 600 distinct neighbours plus 150 repeats, which
stays split after merging, and a few short lists.

Weights are the GCN norm-degree weights of the multigraph times a per-edge
factor in [0.5, 1.5): the magnitudes of the real workload, but unequal inside
a run of parallel edges, so that the order of the weight sum shows in its
bits.  The gathers are held to the tolerance of test_gpu_parity.py (RTOL 1e-4,
ATOL 1e-5) against the fp64 sum over the ORIGINAL edge list.
"""
import numpy as np
import pytest
import torch

from neutronstarlite_amd import graph as G

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5
SPLIT = 256              # default max edges per work item (NTS_SPLIT)


def _chunk(src, dst, v, seed):
    edges = np.stack([np.asarray(src), np.asarray(dst)], 1).astype(np.uint32)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    w = (w * np.random.default_rng(seed).uniform(0.5, 1.5, len(w))).astype(
        np.float32)
    return G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]


def _edges(lists, rng):
    """(src, dst) of the lists interleaved in a random edge-generation order
    that keeps the order inside each list."""
    keys = np.concatenate([np.sort(rng.random(len(lists[d]))) for d in lists])
    src = np.array([s for d in lists for s in lists[d]])
    dst = np.array([d for d in lists for _ in lists[d]])
    order = np.argsort(keys, kind="stable")
    return src[order], dst[order]


def _small():
    rng = np.random.default_rng(3)
    lists = {1: [3, 7, 1, 20], 2: [11] * 7, 3: [5, 9, 5, 2, 9, 5],
             4: [30] * 300}
    for d in range(5, 40):
        lists[d] = list(rng.integers(0, 50, rng.integers(0, 13)))
    return 50, _chunk(*_edges(lists, rng), 50, 5)


def _wide():
    rng = np.random.default_rng(4)
    hub = np.concatenate([rng.permutation(700)[:600],
                          rng.integers(0, 700, 150)])
    lists = {0: list(rng.permutation(hub)), 2: [1, 1, 699, 0, 699],
             3: [4], 699: [0, 698, 0]}
    return 700, _chunk(*_edges(lists, rng), 700, 6)


def _simple():
    """no repeated (src, dst) pair"""
    rng = np.random.default_rng(9)
    pairs = rng.permutation(60 * 60)[:500]
    return 60, _chunk(pairs // 60, pairs % 60, 60, 7)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def cases(dev):
    """name -> (v, host chunk, DeviceChunk(coalesce=True)); built once."""
    from neutronstarlite_amd.ops import DeviceChunk
    out = {}
    for name, (v, ch) in (("small", _small()), ("wide", _wide())):
        out[name] = (v, ch, DeviceChunk(ch, dev, coalesce=True))
    return out


def _directions(ch):
    return {"csc": (ch.column_offset, ch.row_indices, ch.edge_weight_forward),
            "csr": (ch.row_offset, ch.column_indices,
                    ch.edge_weight_backward)}


def _coalesce_ref(offset, nbr, w):
    """np.unique per list; the weights of a pair added as np.float32 one by
    one in original edge position."""
    off, nbrs, ws = [0], [], []
    for v in range(len(offset) - 1):
        e0, e1 = int(offset[v]), int(offset[v + 1])
        for n in np.unique(nbr[e0:e1]):
            total = None
            for e in range(e0, e1):
                if nbr[e] == n:
                    total = w[e] if total is None else np.float32(total + w[e])
            nbrs.append(n)
            ws.append(total)
        off.append(len(nbrs))
    return (np.array(off, dtype=np.uint32), np.array(nbrs, dtype=np.uint32),
            np.array(ws, dtype=np.float32))


def _host(coalesced):
    offset, nbr, w, edges = coalesced
    return (offset.cpu().numpy().view(np.uint32),
            nbr.cpu().numpy().view(np.uint32), w.cpu().numpy(), edges)


def test_the_chunks_hold_the_cases(cases):
    _, ch, _ = cases["small"]
    deg = np.diff(ch.column_offset.astype(np.int64))
    assert deg[0] == 0 and deg[2] == 7 and deg[4] == 300 > SPLIT
    assert list(ch.row_indices[ch.column_offset[3]:ch.column_offset[4]]) == [
        5, 9, 5, 2, 9, 5]
    assert list(ch.row_indices[ch.column_offset[1]:ch.column_offset[2]]) == [
        3, 7, 1, 20]
    _, ch, _ = cases["wide"]
    hub = ch.row_indices[:ch.column_offset[1]]
    assert len(hub) == 750 and len(np.unique(hub)) > 2 * SPLIT


@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("direction", ["csc", "csr"])
def test_coalescer_output(cases, name, direction):
    _, ch, dch = cases[name]
    offset, nbr, w = _directions(ch)[direction]
    ref_off, ref_nbr, ref_w = _coalesce_ref(offset, nbr, w)
    got_off, got_nbr, got_w, edges = _host(getattr(dch, direction + "_coalesced"))
    assert edges == len(ref_nbr) < len(nbr)
    assert got_nbr.shape == got_w.shape == (edges,)
    assert np.array_equal(got_off, ref_off)
    assert np.array_equal(got_nbr, ref_nbr)
    assert np.array_equal(got_w.view(np.uint32), ref_w.view(np.uint32)), (
        f"weights differ in bits at {np.flatnonzero(got_w != ref_w)[:8]}")
    # the original arrays are untouched
    for t, a in ((dch.column_offset, ch.column_offset),
                 (dch.row_indices, ch.row_indices),
                 (dch.row_offset, ch.row_offset),
                 (dch.column_indices, ch.column_indices)):
        assert np.array_equal(t.cpu().numpy().view(np.uint32), a)
    assert np.array_equal(dch.w_fwd.cpu().numpy(), ch.edge_weight_forward)
    assert np.array_equal(dch.w_bwd.cpu().numpy(), ch.edge_weight_backward)
    assert dch.edge_size == ch.edge_size


def test_coalescer_output_over_many_sort_tiles(dev):
    """20 000 edges are five 4096-element tiles of the radix sort, whose
    passes then scatter across tiles; R-MAT repeats many pairs."""
    from neutronstarlite_amd.ops import DeviceChunk
    v = 1000
    edges = G.rmat_edges(v, 20000, seed=9)
    ch = _chunk(edges[:, 0], edges[:, 1], v, 8)
    assert ch.edge_size > 4 * 4096
    dch = DeviceChunk(ch, dev, coalesce=True)
    for direction, (offset, nbr, w) in _directions(ch).items():
        lists = np.repeat(np.arange(v), np.diff(offset.astype(np.int64)))
        order = np.lexsort((nbr, lists))        # stable: ties keep position
        key = lists[order] * v + nbr[order]
        heads = np.flatnonzero(np.r_[True, key[1:] != key[:-1]])
        ref_w = []
        for a, b in zip(heads, np.r_[heads[1:], len(key)]):
            total = w[order[a]]
            for e in order[a + 1:b]:
                total = np.float32(total + w[e])
            ref_w.append(total)
        ref_off = np.searchsorted(lists[order][heads], np.arange(v + 1))
        got_off, got_nbr, got_w, edges_c = _host(
            getattr(dch, direction + "_coalesced"))
        assert edges_c == len(heads) < ch.edge_size
        assert np.array_equal(got_off, ref_off.astype(np.uint32))
        assert np.array_equal(got_nbr, nbr[order][heads])
        assert np.array_equal(got_w.view(np.uint32),
                              np.array(ref_w, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", ["small", "wide"])
def test_two_calls_are_bit_equal(dev, cases, name):
    from neutronstarlite_amd.ops import DeviceChunk
    _, ch, dch = cases[name]
    again = DeviceChunk(ch, dev, coalesce=True)
    for attr in ("csc_coalesced", "csr_coalesced"):
        a, b = _host(getattr(dch, attr)), _host(getattr(again, attr))
        assert a[3] == b[3]
        for x, y in zip(a[:3], b[:3]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))


def _gather(eng, dch, direction, xt, y0, with_weight=True):
    y = y0.clone()
    (eng.csc_forward if direction == "csc" else eng.csr_backward)(
        dch, xt, y, with_weight)
    torch.cuda.synchronize()
    return y.cpu().numpy()


@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("direction", ["csc", "csr"])
@pytest.mark.parametrize("f,dtype", [(8, torch.float32), (72, torch.float32),
                                     (72, torch.bfloat16)])
def test_gather_agreement(dev, cases, name, direction, f, dtype):
    """y += gather over the merged lists, against the fp64 sum over the
    original edge list; bit-equal twice where a vertex is a single item."""
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = cases[name]
    offset, nbr, w = _directions(ch)[direction]
    rng = np.random.default_rng(f)
    xt = torch.from_numpy(
        rng.uniform(-1, 1, (v, f)).astype(np.float32)).to(dev).to(dtype)
    y0 = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    x64 = xt.float().cpu().numpy().astype(np.float64)   # bf16: the rounded rows
    ref = y0.astype(np.float64)
    lists = np.repeat(np.arange(v), np.diff(offset.astype(np.int64)))
    np.add.at(ref, lists, w.astype(np.float64)[:, None] * x64[nbr])
    assert np.abs(ref - y0).max() > 0.1

    eng = HipEngine()
    y0t = torch.from_numpy(y0).to(dev)
    got = _gather(eng, dch, direction, xt, y0t)
    err = np.abs(got - ref)
    tol = RTOL * np.abs(ref) + ATOL
    print(f"{name} {direction} f={f} {dtype}: max err {err.max():.3e}, "
          f"max err/tol {(err / tol).max():.3f}")
    assert (err <= tol).all(), (
        f"{int((err > tol).sum())} elements out of tolerance, worst "
        f"{err.max():.3e}")

    again = _gather(eng, dch, direction, xt, y0t)
    merged_offset = _host(getattr(dch, direction + "_coalesced"))[0]
    single = np.diff(merged_offset.astype(np.int64)) <= SPLIT
    split = name == "wide" and direction == "csc"   # the 600-neighbour list
    assert single.sum() == v - split
    assert np.array_equal(got[single].view(np.uint32),
                          again[single].view(np.uint32))


def test_no_repeat_chunk_keeps_its_launch(dev):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = _simple()
    pairs = ch.row_indices.astype(np.int64) * v + np.repeat(
        np.arange(v), np.diff(ch.column_offset.astype(np.int64)))
    assert len(np.unique(pairs)) == ch.edge_size
    on = DeviceChunk(ch, dev, coalesce=True)
    off = DeviceChunk(ch, dev, coalesce=False)
    assert on.csc_coalesced is None and on.csr_coalesced is None
    assert off.csc_coalesced is None and off.csr_coalesced is None
    eng = HipEngine()
    rng = np.random.default_rng(1)
    for f in (8, 72):
        xt = torch.from_numpy(
            rng.uniform(-1, 1, (v, f)).astype(np.float32)).to(dev)
        y0 = torch.from_numpy(
            rng.uniform(-1, 1, (v, f)).astype(np.float32)).to(dev)
        for direction in ("csc", "csr"):
            a = _gather(eng, on, direction, xt, y0)
            b = _gather(eng, off, direction, xt, y0)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


@pytest.mark.parametrize("name", ["small", "wide"])
@pytest.mark.parametrize("direction", ["csc", "csr"])
def test_unweighted_gather_walks_the_original_list(dev, cases, name,
                                                   direction):
    """An unweighted gather counts every parallel edge, so it must not see
    the merged lists.  Rows of small integers make every fp32 sum exact, so
    the comparison is bit for bit even where a split vertex merges its items
    with atomics in any order; a walk over the merged lists would give
    1 * x where this gives 300 * x."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch, dch = cases[name]
    plain = DeviceChunk(ch, dev, coalesce=False)
    assert plain.csc_coalesced is None and plain.csr_coalesced is None
    eng = HipEngine()
    rng = np.random.default_rng(2)
    offset, nbr, _ = _directions(ch)[direction]
    for f in (8, 72):
        x = rng.integers(-8, 9, (v, f)).astype(np.float32)
        y0 = rng.integers(-8, 9, (v, f)).astype(np.float32)
        xt, y0t = torch.from_numpy(x).to(dev), torch.from_numpy(y0).to(dev)
        a = _gather(eng, dch, direction, xt, y0t, with_weight=False)
        b = _gather(eng, plain, direction, xt, y0t, with_weight=False)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        ref = y0.astype(np.float64)
        lists = np.repeat(np.arange(v), np.diff(offset.astype(np.int64)))
        np.add.at(ref, lists, x.astype(np.float64)[nbr])
        assert np.array_equal(a, ref.astype(np.float32))
