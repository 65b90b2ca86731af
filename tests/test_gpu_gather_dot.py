"""Fused CSR gather + per-edge dot (gather_by_src_from_dst_dot, marked gpu).

One pass over the gathered rows gives both
    out[v, :]       += sum_{e in row v} w[e] * inp[col[e], :]
    dot[dot_pos[e]]  = inp[col[e], :] . dot_vec[v, :]
on the hub graph of test_gpu_gather_sched.py (RMAT plus a star), whose row
degrees cover partial 4-edge unrolls, partial 16-edge batches and rows split
into several work items (merged by atomics).  Reference: float64 numpy.

Gathered rows are held to the project tolerance.  Per-edge dots are held to
|got - ref| <= 1e-5 + 1e-4 * sum_j |a_j b_j|: the fp32 forward-error bound of
an f-term dot is f * 2^-24 * sum|a_j b_j| < 2e-5 * sum|a_j b_j| for f <= 256,
whatever the summation order, so the margin is at least five-fold."""
import functools

import numpy as np
import pytest
import torch

from neutronstarlite_amd import graph as G

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5  # the project tolerance (test_gpu_parity.py)
SPLIT = 256              # default max edges per work item (NTS_SPLIT)
V = 3000


@functools.lru_cache(maxsize=None)
def _graph():
    """RMAT V=3000, E=60000 plus a star of 5000 in-edges on vertex 0."""
    edges = G.rmat_edges(V, 60000, seed=7)
    star_src = np.random.default_rng(3).integers(0, V, 5000)
    star = np.stack([star_src, np.zeros_like(star_src)], axis=1)
    edges = np.concatenate([edges, star.astype(edges.dtype)])
    outd, ind = G.degrees(edges, V)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    return G.build_chunks(edges, w, np.array([0, V], dtype=np.uint32), 0)[0]


@functools.lru_cache(maxsize=None)
def _case(f):
    """(inp, dot_vec, out_ref, dot_ref, dot_mag) for width f, computed once."""
    ch = _graph()
    rng = np.random.default_rng(100 + f)
    inp = rng.uniform(-1, 1, (V, f)).astype(np.float32)
    vec = rng.uniform(-1, 1, (V, f)).astype(np.float32)
    off = ch.row_offset.astype(np.int64)
    deg = np.diff(off)
    col = ch.column_indices.astype(np.int64) - ch.dst_s
    row_of_edge = np.repeat(np.arange(V), deg)
    rows = inp.astype(np.float64)[col]                       # E x f
    prod = rows * vec.astype(np.float64)[row_of_edge]
    dot_ref = prod.sum(axis=1)
    dot_mag = np.abs(prod).sum(axis=1)
    weighted = rows * ch.edge_weight_backward.astype(np.float64)[:, None]
    out_ref = np.zeros((V, f))
    live = deg > 0
    out_ref[live] = np.add.reduceat(weighted, off[:-1][live], axis=0)
    for a in (inp, vec, out_ref, dot_ref, dot_mag):
        a.setflags(write=False)
    return inp, vec, out_ref, dot_ref, dot_mag


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    ch = _graph()

    def up32(a):
        return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).to(dev)

    perm = np.random.default_rng(5).permutation(ch.edge_size).astype(np.uint32)
    return {"dev": dev, "s": shim.Stream.wrap_torch_current(),
            "roff": up32(ch.row_offset), "cols": up32(ch.column_indices),
            "w": torch.from_numpy(ch.edge_weight_backward).to(dev),
            "perm": perm, "d_perm": up32(perm)}


def _run(gpu, f, with_pos):
    ch, dev = _graph(), gpu["dev"]
    inp, vec = _case(f)[:2]
    d_inp = torch.tensor(inp, device=dev)
    d_vec = torch.tensor(vec, device=dev)
    out = torch.zeros(V, f, device=dev)
    dot = torch.full((ch.edge_size,), float("nan"), device=dev)
    rc = gpu["s"].gather_by_src_from_dst_dot(
        d_inp.data_ptr(), out.data_ptr(), gpu["w"].data_ptr(),
        gpu["roff"].data_ptr(), gpu["cols"].data_ptr(), int(ch.dst_s),
        int(ch.src_n), int(ch.edge_size), f, d_vec.data_ptr(),
        dot.data_ptr(),
        gpu["d_perm"].data_ptr() if with_pos else None)
    torch.cuda.synchronize()
    return rc, out.cpu().numpy(), dot.cpu().numpy()


def _assert_rows(got, ref, name):
    err = np.abs(got - ref)
    bad = err > RTOL * np.abs(ref) + ATOL
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} out of tol"


def test_degree_coverage():
    deg = np.diff(_graph().row_offset.astype(np.int64))
    assert (deg % 4 != 0).any() and (deg % 4 == 0).any()
    assert ((deg > 16) & (deg % 16 != 0)).any()      # partial LDS batch
    assert ((deg > 0) & (deg < 4)).any()             # tail loop only
    assert deg.max() > SPLIT                         # split row: atomics
    assert (deg[deg > SPLIT] % SPLIT != 0).any()     # short last item


# f=34: dwordx2, 17 of 32 lanes live; f=128: dwordx4, G=32; f=256: G=64
@pytest.mark.parametrize("with_pos", [False, True])
@pytest.mark.parametrize("f", [34, 128, 256])
def test_fused_gather_and_dot(gpu, f, with_pos):
    _, _, out_ref, dot_ref, dot_mag = _case(f)
    rc, out, dot = _run(gpu, f, with_pos)
    assert rc == 1, "the fused kernel must run at this width"
    _assert_rows(out, out_ref, f"gather f={f}")
    if with_pos:
        placed = np.empty_like(dot)
        placed[:] = dot[gpu["perm"]]  # dot_out[dot_pos[e]] is edge e's dot
        dot = placed
    assert np.isfinite(dot).all(), "every edge slot is written"
    err = np.abs(dot - dot_ref)
    bad = err > 1e-5 + 1e-4 * dot_mag
    assert not bad.any(), (
        f"dot f={f} pos={with_pos}: {bad.sum()}/{bad.size} out of bound, "
        f"worst {(err / (1e-5 + 1e-4 * dot_mag)).max():.3e} of it")


@pytest.mark.parametrize("with_pos", [False, True])
def test_ragged_width_falls_back_to_plain_gather(gpu, with_pos):
    """f=33 cannot fuse: returns 0, and the plain gather has still run."""
    rc, out, _ = _run(gpu, 33, with_pos)
    assert rc == 0
    _assert_rows(out, _case(33)[2], "fallback gather f=33")
