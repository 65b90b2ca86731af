"""Row staging of the gather SpMM kernel (marked gpu).

A staged gather first copies the gathered rows into the stream's buffer at a
pitch of whole 128-byte lines (k_repitch), then reads that buffer with dwordx4
lanes; output rows keep their pitch.  Every output element is still one lane's
fmaf chain over the item's edges in edge order, so for vertices that are not
split into several work items a staged gather must be BIT-identical to the
unstaged launch: a difference is a bug, not rounding.  Split (hub) vertices
merge with atomics and are held to the project tolerance against the CPU
oracle instead, as are the cases that have no unstaged twin."""
import numpy as np
import pytest
import torch

import oracle
from neutronstarlite_amd import graph as G

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5  # the project tolerance (test_gpu_parity.py)
SPLIT = 256              # default max edges per work item (NTS_SPLIT)

ITEM, PHASE, XCD = 0, 1, 2
AUTO, FORCE, NEVER = 0, 1, -1


def assert_close(got, ref, name=""):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    err = np.abs(got - ref)
    tol = RTOL * np.abs(ref) + ATOL
    bad = err > tol
    assert not bad.any(), (
        f"{name}: {bad.sum()}/{bad.size} out of tol; worst "
        f"{(err / np.maximum(np.abs(ref), 1e-30)).max():.3e} rel")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _chunk(edges, v, weights=None):
    if weights is None:
        outd, ind = G.degrees(edges, v)
        weights = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    return G.build_chunks(edges, weights, np.array([0, v], dtype=np.uint32),
                          0)[0]


@pytest.fixture(scope="module")
def bounded_graph():
    """V=2000, per-destination degree uniform in [0, 200] (zero-degree
    vertices included), sources uniform: no vertex reaches the work-item
    split in either direction, so no atomics run."""
    v = 2000
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 201, size=v)
    deg[:3] = 0
    dst = np.repeat(np.arange(v, dtype=np.uint32), deg)
    src = rng.integers(0, v, size=dst.size).astype(np.uint32)
    edges = np.stack([src, dst], axis=1)
    assert np.bincount(dst, minlength=v).max() <= SPLIT
    assert np.bincount(src, minlength=v).max() <= SPLIT
    w = rng.uniform(0.1, 1.0, size=dst.size).astype(np.float32)
    return v, _chunk(edges, v, w)


@pytest.fixture(scope="module")
def hub_graph():
    """RMAT V=3000, E=60000 plus a star of 5000 in-edges on vertex 0: hubs
    split into several work items in both directions (atomic merge)."""
    v = 3000
    edges = G.rmat_edges(v, 60000, seed=7)
    star_src = np.random.default_rng(3).integers(0, v, 5000)
    star = np.stack([star_src, np.zeros_like(star_src)], axis=1)
    edges = np.concatenate([edges, star.astype(edges.dtype)])
    assert np.bincount(edges[:, 1], minlength=v).max() > SPLIT
    assert np.bincount(edges[:, 0], minlength=v).max() > SPLIT
    return v, _chunk(edges, v)


def _run(eng, dch, direction, inp, with_weight=True, out=None):
    rows = dch.dst_n if direction == "fwd" else dch.src_n
    if out is None:
        out = torch.zeros(rows, inp.shape[1], device=inp.device)
    if direction == "fwd":
        eng.csc_forward(dch, inp, out, with_weight)
    else:
        eng.csr_backward(dch, inp, out, with_weight)
    return out


def _pitch(f):
    return -(-f // 32) * 32


@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("f", [2, 33, 130, 602, 1433])
def test_staged_bit_equal_to_unstaged(dev, bounded_graph, f, direction,
                                      with_weight):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = bounded_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    x = torch.from_numpy(np.random.default_rng(f).uniform(
        -1, 1, (v, f)).astype(np.float32)).to(dev)
    eng.stream.gather_staging(NEVER)
    eng.stream.gather_schedule(ITEM, -1)  # exactly the pre-window launch
    base = _run(eng, dch, direction, x, with_weight)
    assert eng.stream.gather_staging_last() == (False, 0)
    assert base.abs().max().item() > 0
    eng.stream.gather_staging(FORCE)
    for sched in (ITEM, PHASE, XCD):
        # 128 is the window of the automatic staged launch
        for window in (0, 38, 128, 152):
            eng.stream.gather_schedule(sched, window)
            got = _run(eng, dch, direction, x, with_weight)
            # staged for real: the test cannot pass by falling back
            assert eng.stream.gather_staging_last() == (True, _pitch(f))
            assert torch.equal(got, base), (
                f"f={f} {direction} w={with_weight} schedule {sched} window "
                f"{window} (ran {eng.stream.gather_schedule_last()}): "
                f"{(got != base).sum().item()} elements differ")
    torch.cuda.synchronize()


@pytest.mark.parametrize("f", [602, 70])
def test_staged_split_hubs_match_oracle(dev, hub_graph, f):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = hub_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    eng.stream.gather_staging(FORCE)
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    g = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward, x, 0, v, f)
    gx_ref = oracle.csr_backward(ch.row_offset, ch.column_indices,
                                 ch.edge_weight_backward, g, 0, v, f)
    xt, gt = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
    for sched, window in [(ITEM, -1), (PHASE, 0), (PHASE, 38), (XCD, 152)]:
        eng.stream.gather_schedule(sched, window)
        assert_close(_run(eng, dch, "fwd", xt), y_ref,
                     f"fwd f={f} sched {sched} window {window}")
        assert eng.stream.gather_staging_last() == (True, _pitch(f))
        assert_close(_run(eng, dch, "bwd", gt), gx_ref,
                     f"bwd f={f} sched {sched} window {window}")
        assert eng.stream.gather_staging_last() == (True, _pitch(f))


@pytest.mark.parametrize("f", [602, 33])
def test_staged_input_view_at_4_byte_offset(dev, hub_graph, f):
    """The copy reads single dwords; the gather still runs dwordx4 lanes."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = hub_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    eng.stream.gather_staging(FORCE)
    x = np.random.default_rng(4).uniform(-1, 1, (v, f)).astype(np.float32)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward, x, 0, v, f)
    flat = torch.zeros(v * f + 1, device=dev)
    xt = flat[1:].view(v, f)
    xt.copy_(torch.from_numpy(x))
    assert xt.data_ptr() % 8 == 4 and xt.is_contiguous()
    for sched, window in [(ITEM, -1), (PHASE, 0), (XCD, 38)]:
        eng.stream.gather_schedule(sched, window)
        assert_close(_run(eng, dch, "fwd", xt), y_ref,
                     f"input view f={f} sched {sched} window {window}")
        assert eng.stream.gather_staging_last() == (True, _pitch(f))


@pytest.mark.parametrize("f", [602, 604])
def test_staged_output_view_at_4_byte_offset(dev, hub_graph, f):
    """Store width 1: the output rows are only dword-aligned."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = hub_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    eng.stream.gather_staging(FORCE)
    x = np.random.default_rng(5).uniform(-1, 1, (v, f)).astype(np.float32)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward, x, 0, v, f)
    xt = torch.from_numpy(x).to(dev)
    for sched, window in [(ITEM, -1), (PHASE, 0), (XCD, 38)]:
        eng.stream.gather_schedule(sched, window)
        flat = torch.zeros(v * f + 2, device=dev)
        y = flat[1:-1].view(v, f)
        assert y.data_ptr() % 8 == 4 and y.is_contiguous()
        _run(eng, dch, "fwd", xt, out=y)
        assert eng.stream.gather_staging_last() == (True, _pitch(f))
        assert_close(y, y_ref,
                     f"output view f={f} sched {sched} window {window}")
        # nothing was written around the view
        assert flat[0].item() == 0 and flat[-1].item() == 0


@pytest.mark.parametrize("request_", [(0, 0), (PHASE, 0), (XCD, 38)])
def test_staged_accumulate_across_chunks(dev, request_):
    """Two chunks into the same output rows must ADD; the second chunk's
    rows start at a non-zero src_start."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, f, parts = 1000, 602, 2
    edges = G.rmat_edges(v, 20000, seed=9)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    offs = G.partition_offsets(edges, v, parts)
    x = np.random.default_rng(1).uniform(-1, 1, (v, f)).astype(np.float32)
    eng = HipEngine()
    eng.stream.gather_staging(FORCE)
    eng.stream.gather_schedule(*request_)
    lo, hi = int(offs[0]), int(offs[1])
    y = torch.zeros(hi - lo, f, device=dev)
    chunks = G.build_chunks(edges, w, offs, 0)
    assert len(chunks) == 2 and chunks[1].src_s > 0
    for k, ch in enumerate(chunks):
        blk = torch.from_numpy(
            np.ascontiguousarray(x[int(offs[k]):int(offs[k + 1])])).to(dev)
        eng.csc_forward(DeviceChunk(ch, dev), blk, y)
        assert eng.stream.gather_staging_last() == (True, 608)
    whole = _chunk(edges, v)
    y_ref = oracle.csc_forward(whole.column_offset, whole.row_indices,
                               whole.edge_weight_forward, x, 0, v, f)
    assert_close(y, y_ref[lo:hi], f"chunked fwd {request_}")


def test_staging_buffer_reuse_and_growth(dev, hub_graph):
    """Three gathers back to back on one stream, no sync between them: small,
    larger (the buffer grows), small again, each with its own input."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    eng = HipEngine()
    eng.stream.gather_staging(FORCE)
    small_v = 300
    small = _chunk(G.rmat_edges(small_v, 4000, seed=2), small_v)
    big_v, big = hub_graph
    jobs = []
    for k, (v, ch, f) in enumerate([(small_v, small, 70), (big_v, big, 602),
                                    (small_v, small, 130)]):
        x = np.random.default_rng(20 + k).uniform(
            -1, 1, (v, f)).astype(np.float32)
        jobs.append((v, ch, f, x, DeviceChunk(ch, dev),
                     torch.from_numpy(x).to(dev)))
    torch.cuda.synchronize()
    outs = []
    for v, ch, f, x, dch, xt in jobs:
        outs.append(_run(eng, dch, "fwd", xt))
        assert eng.stream.gather_staging_last() == (True, _pitch(f))
    for (v, ch, f, x, dch, xt), y in zip(jobs, outs):
        y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                                   ch.edge_weight_forward, x, 0, v, f)
        assert_close(y, y_ref, f"back to back V={v} f={f}")


def test_small_shapes_do_not_stage_by_themselves(dev, bounded_graph):
    """Automatic mode leaves a cache-resident matrix alone."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = bounded_graph
    eng = HipEngine()
    _run(eng, DeviceChunk(ch, dev), "fwd", torch.zeros(v, 602, device=dev))
    assert eng.stream.gather_staging_last() == (False, 0)
