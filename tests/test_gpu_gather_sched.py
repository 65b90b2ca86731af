"""Column schedules of the gather SpMM kernel (marked gpu).

A gather task is (work item, column window); the schedules (item-major,
phase-major, XCD-affine) only permute which task runs when.  Every output
element stays one lane's fmaf chain over the item's edges in edge order, so
for vertices that are not split into several work items the output must be
BIT-identical to schedule 0 — a difference is a bug, not rounding.  Split (hub) vertices merge with atomics and are held to
the project tolerance against the CPU oracle instead."""
import numpy as np
import pytest
import torch

import oracle
from neutronstarlite_amd import graph as G

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5  # the project tolerance (test_gpu_parity.py)
SPLIT = 256              # default max edges per work item (NTS_SPLIT)

ITEM, PHASE, XCD = 0, 1, 2
SCHEDULES = (ITEM, PHASE, XCD)
# 0 = the schedule's default width; at f=602, 38/76 give 16/8 windows (no
# left-over for the XCD classes), 64 gives 10 (two shared out), 152/302 give
# 4/2 (classes share a window); 6, 38, 64, 76 do not divide most widths; 2000
# is wider than every f
WINDOWS = (0, 6, 38, 64, 76, 128, 152, 256, 302, 2000)


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
    assert (np.bincount(dst, minlength=v) == 0).any()
    w = rng.uniform(0.1, 1.0, size=dst.size).astype(np.float32)
    return v, _chunk(edges, v, w)


def _run(eng, dch, direction, inp, with_weight):
    rows = dch.dst_n if direction == "fwd" else dch.src_n
    out = torch.zeros(rows, inp.shape[1], device=inp.device)
    if direction == "fwd":
        eng.csc_forward(dch, inp, out, with_weight)
    else:
        eng.csr_backward(dch, inp, out, with_weight)
    return out


@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("f", [2, 33, 130, 602, 1433])
def test_bit_equal_across_schedules(dev, bounded_graph, f, direction,
                                    with_weight):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = bounded_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    x = torch.from_numpy(np.random.default_rng(f).uniform(
        -1, 1, (v, f)).astype(np.float32)).to(dev)
    eng.stream.gather_schedule(ITEM, -1)  # exactly the pre-window launch
    base = _run(eng, dch, direction, x, with_weight)
    assert eng.stream.gather_schedule_last()[0] == ITEM
    assert base.abs().max().item() > 0
    for sched in SCHEDULES:
        for window in WINDOWS:
            if sched == ITEM and window == 0:
                continue  # (0, 0) is the automatic request
            eng.stream.gather_schedule(sched, window)
            got = _run(eng, dch, direction, x, with_weight)
            assert torch.equal(got, base), (
                f"f={f} {direction} w={with_weight} schedule {sched} window "
                f"{window} (ran {eng.stream.gather_schedule_last()}): "
                f"{(got != base).sum().item()} elements differ")
    torch.cuda.synchronize()


def test_requested_schedules_really_run(dev, bounded_graph):
    """The bit-equality above must not pass by falling back: at f=602 the
    schedule that was asked for runs wherever it can."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = bounded_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    x = torch.zeros(v, 602, device=dev)
    for sched, window, ran in [
            (PHASE, 0, (PHASE, 128)), (PHASE, 64, (PHASE, 64)),
            (PHASE, 75, (PHASE, 76)),            # rounded up to dwordx2
            (XCD, 0, (XCD, 64)), (XCD, 38, (XCD, 38)), (XCD, 76, (XCD, 76)),
            (XCD, 152, (XCD, 152)), (XCD, 302, (XCD, 302)),  # 4 and 2 windows
            (XCD, 128, (ITEM, 128)),             # 5 windows: not one a class
            (PHASE, 2000, (ITEM, 128)),          # one window
            (ITEM, 76, (ITEM, 76)), (ITEM, -1, (ITEM, 128))]:
        eng.stream.gather_schedule(sched, window)
        _run(eng, dch, "fwd", x, True)
        assert eng.stream.gather_schedule_last() == ran, (sched, window)


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


@pytest.mark.parametrize("f", [602, 70])
def test_split_hubs_match_oracle(dev, hub_graph, f):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = hub_graph
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    g = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward, x, 0, v, f)
    gx_ref = oracle.csr_backward(ch.row_offset, ch.column_indices,
                                 ch.edge_weight_backward, g, 0, v, f)
    xt, gt = torch.from_numpy(x).to(dev), torch.from_numpy(g).to(dev)
    for sched in SCHEDULES:
        for window in (0, 10, 38, 152):
            eng.stream.gather_schedule(sched, window if (sched or window)
                                       else -1)
            assert_close(_run(eng, dch, "fwd", xt, True), y_ref,
                         f"fwd f={f} sched {sched} window {window}")
            assert_close(_run(eng, dch, "bwd", gt, True), gx_ref,
                         f"bwd f={f} sched {sched} window {window}")


@pytest.mark.parametrize("v,e", [(10, 30), (2, 3)])
def test_tiny_grid_covers_every_column(dev, v, e):
    """A grid too small to give each of the 8 classes a workgroup must still
    cover every column under an XCD-affine request (V=2: at most 6
    workgroups, the current order runs)."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    f = 602
    edges = G.rmat_edges(v, e, seed=5)
    ch = _chunk(edges, v)
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    x = np.random.default_rng(8).uniform(-1, 1, (v, f)).astype(np.float32)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward, x, 0, v, f)
    assert (np.abs(y_ref).max(axis=0) > 0).all()  # every column carries data
    xt = torch.from_numpy(x).to(dev)
    for sched, window in [(XCD, 76), (XCD, 38), (XCD, 64), (XCD, 152), (PHASE, 76)]:
        eng.stream.gather_schedule(sched, window)
        assert_close(_run(eng, dch, "fwd", xt, True), y_ref,
                     f"tiny V={v} sched {sched} window {window}")
        if v == 2 and sched >= XCD:
            assert eng.stream.gather_schedule_last()[0] == ITEM


def test_unaligned_input_windows(dev, hub_graph):
    """A (V, f) view at a 4-byte storage offset forces the strided-dword
    path; windows must bound it the same way."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = hub_graph
    f = 602
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    x = np.random.default_rng(4).uniform(-1, 1, (v, f)).astype(np.float32)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward, x, 0, v, f)
    flat = torch.zeros(v * f + 1, device=dev)
    xt = flat[1:].view(v, f)
    xt.copy_(torch.from_numpy(x))
    assert xt.data_ptr() % 8 == 4 and xt.is_contiguous()
    for sched, window in [(ITEM, -1), (ITEM, 76), (PHASE, 0), (PHASE, 76),
                          (XCD, 0), (XCD, 38), (XCD, 100), (PHASE, 300)]:
        eng.stream.gather_schedule(sched, window)
        assert_close(_run(eng, dch, "fwd", xt, True), y_ref,
                     f"unaligned sched {sched} window {window}")


@pytest.mark.parametrize("request_", [(0, 0), (PHASE, 0), (XCD, 0),
                                      (XCD, 38)])
def test_accumulate_across_chunks(dev, request_):
    """Two chunks into the same output rows must ADD under the automatic
    choice and under every schedule."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, f, parts = 1000, 602, 2
    edges = G.rmat_edges(v, 20000, seed=9)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    offs = G.partition_offsets(edges, v, parts)
    x = np.random.default_rng(1).uniform(-1, 1, (v, f)).astype(np.float32)
    eng = HipEngine()
    eng.stream.gather_schedule(*request_)
    lo, hi = int(offs[0]), int(offs[1])
    y = torch.zeros(hi - lo, f, device=dev)
    for k, ch in enumerate(G.build_chunks(edges, w, offs, 0)):
        blk = torch.from_numpy(
            np.ascontiguousarray(x[int(offs[k]):int(offs[k + 1])])).to(dev)
        eng.csc_forward(DeviceChunk(ch, dev), blk, y)
    whole = _chunk(edges, v)
    y_ref = oracle.csc_forward(whole.column_offset, whole.row_indices,
                               whole.edge_weight_forward, x, 0, v, f)
    assert_close(y, y_ref[lo:hi], f"chunked fwd {request_}")


def test_automatic_choice(dev):
    """One-window widths, low-degree graphs and matrices that fit the
    Infinity Cache keep schedule 0 at the native slab; a wide, high-reuse
    matrix beyond the cache engages the blocked schedule and stays right."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    eng = HipEngine()

    def run(v, e, f, check):
        edges = G.rmat_edges(v, e, seed=7)
        ch = _chunk(edges, v)
        dch = DeviceChunk(ch, dev)
        if check:
            x = np.random.default_rng(2).uniform(
                -1, 1, (v, f)).astype(np.float32)
            xt = torch.from_numpy(x).to(dev)
        else:
            xt = torch.zeros(v, f, device=dev)
        y = _run(eng, dch, "fwd", xt, True)
        ran = eng.stream.gather_schedule_last()
        if check:
            assert_close(y, oracle.csc_forward(
                ch.column_offset, ch.row_indices, ch.edge_weight_forward, x,
                0, v, f), f"auto V={v} f={f} ran {ran}")
        return ran

    # one window (f=128, dwordx4), degree 40
    assert run(70_000, 2_800_000, 128, False) == (ITEM, 128)
    # five slabs, 277 MB matrix, but ~6 edges per row
    assert run(115_000, 575_000, 602, False) == (ITEM, 128)
    # five slabs, high reuse, but the 48 MB matrix fits the Infinity Cache
    assert run(20_000, 800_000, 602, False) == (ITEM, 128)
    # every engagement condition met (270 MB, 34 edges per row)
    assert run(112_000, 3_700_000, 602, True) == (PHASE, 128)
