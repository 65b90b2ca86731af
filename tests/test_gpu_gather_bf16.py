"""The gather SpMM over bfloat16 feature rows (marked gpu).

bf16 -> fp32 is exact (the bf16 bits are the high half of the fp32), and the
bf16 kernel instantiation runs the same fp32 fmaf chain per output element,
over the item's edges in edge order, as the fp32 one run on the widened
values.  So on every vertex that is not split into several work items the
two must agree BIT FOR BIT, under every lane width, alignment and schedule:
one differing element is a bug, not rounding.  Split (hub) vertices merge
with atomics and are held to the project tolerance against the CPU oracle on
the widened values, the fp32 kernel's own bar."""
import numpy as np
import pytest
import torch

import oracle
from neutronstarlite_amd import graph as G

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5  # the project tolerance (test_gpu_parity.py)
SPLIT = 256              # default max edges per work item (NTS_SPLIT)
ITEM, PHASE, XCD = 0, 1, 2

# (0, 0) is the automatic request
REQUESTS = [(0, 0), (ITEM, -1), (PHASE, 64), (PHASE, 76), (XCD, 38),
            (XCD, 152)]
# elements per lane at 16-byte alignment: every width, ragged strided tails
# (1, 7, 33, 1433), multi-slab rows (130, 602, 608, 1433)
LANE = {1: 1, 7: 1, 33: 1, 130: 2, 132: 4, 136: 8, 602: 2, 608: 8, 1433: 1}
# what the requests must really run at the two wide even widths
RAN = {602: [(ITEM, 128), (ITEM, 128), (PHASE, 64), (PHASE, 76), (XCD, 38),
             (XCD, 152)],
       608: [(ITEM, 512), (ITEM, 512), (PHASE, 64), (PHASE, 80), (XCD, 40),
             (XCD, 152)]}


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
def bounded(dev):
    """V=2000, per-destination degree uniform in [0, 200], sources uniform:
    no vertex reaches the work-item split in either direction, so no atomics
    run and results are deterministic to the bit."""
    from neutronstarlite_amd.ops import DeviceChunk
    v = 2000
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 201, size=v)
    deg[:3] = 0
    dst = np.repeat(np.arange(v, dtype=np.uint32), deg)
    src = rng.integers(0, v, size=dst.size).astype(np.uint32)
    assert np.bincount(dst, minlength=v).max() <= SPLIT
    assert np.bincount(src, minlength=v).max() <= SPLIT
    w = rng.uniform(0.1, 1.0, size=dst.size).astype(np.float32)
    ch = _chunk(np.stack([src, dst], axis=1), v, w)
    return v, ch, DeviceChunk(ch, dev)


@pytest.fixture(scope="module")
def hub(dev):
    """RMAT V=3000, E=60000 plus 5000 in-edges on vertex 0: hubs split into
    several work items in both directions (atomic merge)."""
    from neutronstarlite_amd.ops import DeviceChunk
    v = 3000
    edges = G.rmat_edges(v, 60000, seed=7)
    star_src = np.random.default_rng(3).integers(0, v, 5000)
    star = np.stack([star_src, np.zeros_like(star_src)], axis=1)
    edges = np.concatenate([edges, star.astype(edges.dtype)])
    assert np.bincount(edges[:, 1], minlength=v).max() > SPLIT
    assert np.bincount(edges[:, 0], minlength=v).max() > SPLIT
    ch = _chunk(edges, v)
    return v, ch, DeviceChunk(ch, dev)


def bf16_bits(bits, dev):
    return torch.tensor(bits, dtype=torch.int16, device=dev).view(
        torch.bfloat16)


def make_input(v, f, seed, dev, largest=True):
    """U(-1,1) rounded to bf16, with exact zeros, -0.0 and bf16 subnormals
    planted, and (where the comparison is exact) the largest finite bf16.
    No NaN, and no negative huge value: sums may reach +inf, never NaN."""
    rng = np.random.default_rng(seed)
    x = torch.from_numpy(rng.uniform(-1, 1, (v, f)).astype(np.float32)).to(
        dev).to(torch.bfloat16)
    special = [0x0000, -0x8000, 0x0001, 0x007f, -0x8000 + 0x0040]
    if largest:
        special.append(0x7f7f)
    flat = x.view(-1)
    where = torch.from_numpy(rng.choice(flat.numel(), 8 * len(special),
                                        replace=flat.numel() < 64)).to(dev)
    flat[where] = bf16_bits(special, dev).repeat(8)
    assert not torch.isnan(x.float()).any()
    return x


def run(eng, dch, direction, inp, with_weight=True):
    rows = dch.dst_n if direction == "fwd" else dch.src_n
    out = torch.zeros(rows, inp.shape[1], device=inp.device)
    if direction == "fwd":
        eng.csc_forward(dch, inp, out, with_weight)
    else:
        eng.csr_backward(dch, inp, out, with_weight)
    return out


def align_of(t):
    """Alignment of a tensor's storage, as nts_gather_plan_bf16 takes it
    (every output here is a fresh allocation, 16-byte aligned at least)."""
    return 16 if t.data_ptr() % 16 == 0 else t.data_ptr() % 16


def check_bit_identity(eng, dch, direction, x16, with_weight, requests, lane,
                       ran=None):
    """bf16 gather under each request == fp32 gather of the widened values,
    and the lane width and schedule meant really ran."""
    from neutronstarlite_amd import shim
    v, f = x16.shape
    eng.stream.gather_schedule(ITEM, -1)
    base = run(eng, dch, direction, x16.float(), with_weight)
    assert base.abs().max().item() > 0
    for i, req in enumerate(requests):
        eng.stream.gather_schedule(*req)
        got = run(eng, dch, direction, x16, with_weight)
        last = eng.stream.gather_schedule_last()
        p = shim.gather_plan_bf16(f, align_of(x16), v, v, dch.edge_size, *req)
        assert p["vector_width"] == lane, (f, req, p)
        assert last == (p["schedule"], p["window"]), (f, req, last, p)
        if ran is not None:
            assert last == ran[i], (f, req, last)
        assert got.dtype == torch.float32
        assert torch.equal(got, base), (
            f"f={f} {direction} w={with_weight} request {req} ran {last} "
            f"lane {lane}: {(got != base).sum().item()} elements differ")
    eng.stream.gather_schedule(0, 0)


@pytest.mark.parametrize("with_weight", [True, False])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
@pytest.mark.parametrize("f", sorted(LANE))
def test_bit_identical_to_fp32_kernel(dev, bounded, f, direction,
                                      with_weight):
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = bounded
    x16 = make_input(v, f, 100 + f, dev)
    assert x16.data_ptr() % 16 == 0
    check_bit_identity(HipEngine(), dch, direction, x16, with_weight,
                       REQUESTS, LANE[f], RAN.get(f))


@pytest.mark.parametrize("f,offset,lane", [
    (608, 1, 1), (608, 2, 2), (608, 4, 4), (601, 0, 1), (601, 1, 1)])
@pytest.mark.parametrize("direction", ["fwd", "bwd"])
def test_alignment_picks_the_lane_width(dev, bounded, f, offset, lane,
                                        direction):
    """Views of one flat bf16 buffer at 1, 2 and 4 elements in: 2-, 4- and
    8-byte aligned rows force the 1-, 2- and 4-wide forms at f=608."""
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = bounded
    flat = torch.zeros(v * f + 8, dtype=torch.bfloat16, device=dev)
    x16 = flat[offset:offset + v * f].view(v, f)
    x16.copy_(make_input(v, f, 7 * f + offset, dev))
    assert x16.is_contiguous()
    assert x16.data_ptr() == flat.data_ptr() + 2 * offset
    if offset:
        assert align_of(x16) == 2 * offset
    for with_weight in (True, False):
        check_bit_identity(HipEngine(), dch, direction, x16, with_weight,
                           [(0, 0), (PHASE, 76), (XCD, 38)], lane)


@pytest.mark.parametrize("f", [602, 70])
def test_split_hubs_match_oracle(dev, hub, f):
    """Atomically merged hubs: the fp32 kernel's own tolerance against the
    CPU oracle on the widened values.  (No largest-finite value here: a sum
    that overflows would make the comparison vacuous.)"""
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = hub
    eng = HipEngine()
    x16 = make_input(v, f, 42, dev, largest=False)
    g16 = make_input(v, f, 43, dev, largest=False)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward,
                               x16.float().cpu().numpy(), 0, v, f)
    gx_ref = oracle.csr_backward(ch.row_offset, ch.column_indices,
                                 ch.edge_weight_backward,
                                 g16.float().cpu().numpy(), 0, v, f)
    for sched in (ITEM, PHASE, XCD):
        for window in (0, 10, 38):
            eng.stream.gather_schedule(sched, window if (sched or window)
                                       else -1)
            assert_close(run(eng, dch, "fwd", x16), y_ref,
                         f"fwd f={f} sched {sched} window {window}")
            assert_close(run(eng, dch, "bwd", g16), gx_ref,
                         f"bwd f={f} sched {sched} window {window}")
    if f == 602:  # the requests are not all falling back
        eng.stream.gather_schedule(XCD, 38)
        run(eng, dch, "fwd", x16)
        assert eng.stream.gather_schedule_last() == (XCD, 38)


@pytest.mark.parametrize("request_", [(0, 0), (PHASE, 0), (XCD, 38)])
def test_accumulate_across_chunks(dev, request_):
    """Two bf16 chunks gathered into the same fp32 rows must ADD."""
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, f, parts = 1000, 602, 2
    edges = G.rmat_edges(v, 20000, seed=9)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    offs = G.partition_offsets(edges, v, parts)
    x16 = make_input(v, f, 1, dev, largest=False)
    x = x16.float().cpu().numpy()
    eng = HipEngine()
    eng.stream.gather_schedule(*request_)
    lo, hi = int(offs[0]), int(offs[1])
    y = torch.zeros(hi - lo, f, device=dev)
    for k, ch in enumerate(G.build_chunks(edges, w, offs, 0)):
        blk = x16[int(offs[k]):int(offs[k + 1])].contiguous()
        eng.csc_forward(DeviceChunk(ch, dev), blk, y)
    whole = _chunk(edges, v)
    y_ref = oracle.csc_forward(whole.column_offset, whole.row_indices,
                               whole.edge_weight_forward, x, 0, v, f)
    assert_close(y, y_ref[lo:hi], f"chunked fwd {request_}")


def test_automatic_choice_counts_real_bytes(dev):
    """The fault of an engagement rule can show only at size: 112 000 rows
    of f=602 are beyond the Infinity Cache in fp32 (blocked schedule) and
    inside it in bf16 (native launch); 230 000 rows are beyond it in bf16
    too, and the blocked schedule that then runs stays right (against the
    fp32 kernel on the widened values, hubs included: project tolerance)."""
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    eng = HipEngine()
    f = 602

    def graph(v, e):
        dch = DeviceChunk(_chunk(G.rmat_edges(v, e, seed=7), v), dev)
        torch.manual_seed(v)
        return dch, (torch.rand(v, f, device=dev) * 2 - 1).to(torch.bfloat16)

    def run_auto(dch, x):
        eng.stream.gather_schedule(0, 0)
        y = run(eng, dch, "fwd", x)
        return y, eng.stream.gather_schedule_last()

    dch, x16 = graph(112_000, 3_700_000)
    assert run_auto(dch, x16.float())[1] == (PHASE, 128)
    assert run_auto(dch, x16)[1] == (ITEM, 128)
    del dch, x16
    v = 230_000
    dch, x16 = graph(v, 8_000_000)
    y16, ran = run_auto(dch, x16)
    p = shim.gather_plan_bf16(f, 16, v, v, dch.edge_size)
    assert p["blocked"] and ran == (p["schedule"], p["window"]), (ran, p)
    eng.stream.gather_schedule(ITEM, -1)
    y32 = run(eng, dch, "fwd", x16.float())
    assert_close(y16, y32.cpu().numpy(), f"auto bf16 ran {ran}")


@pytest.mark.parametrize("v,e", [(10, 30), (2, 3)])
def test_tiny_grid_covers_every_column(dev, v, e):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    f = 602
    ch = _chunk(G.rmat_edges(v, e, seed=5), v)
    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    x = np.random.default_rng(8).uniform(-1, 1, (v, f)).astype(np.float32)
    x16 = torch.from_numpy(x).to(dev).to(torch.bfloat16)
    y_ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                               ch.edge_weight_forward,
                               x16.float().cpu().numpy(), 0, v, f)
    assert (np.abs(y_ref).max(axis=0) > 0).all()  # every column carries data
    for sched, window in [(XCD, 76), (XCD, 38), (XCD, 64), (XCD, 152)]:
        eng.stream.gather_schedule(sched, window)
        assert_close(run(eng, dch, "fwd", x16), y_ref,
                     f"tiny V={v} sched {sched} window {window}")
        ran = eng.stream.gather_schedule_last()
        assert ran[0] == (ITEM if v == 2 else XCD), ran


def test_empty_chunk_is_a_no_op(dev):
    from neutronstarlite_amd.ops import HipEngine
    eng = HipEngine()
    eng.stream.timing(True)
    eng.stream.timing_reset()
    f = 602
    x16 = torch.ones(4, f, dtype=torch.bfloat16, device=dev)
    y = torch.full((4, f), 3.0, device=dev)
    off = torch.zeros(5, dtype=torch.int32, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    w = torch.ones(1, device=dev)
    for edges, batch in [(0, 4), (0, 0), (1, 0)]:
        for entry in (eng.stream.gather_by_dst_from_src_bf16,
                      eng.stream.gather_by_src_from_dst_bf16):
            entry(x16.data_ptr(), y.data_ptr(), w.data_ptr(), idx.data_ptr(),
                  off.data_ptr(), 0, 4, 0, 4, edges, batch, f, True)
    from neutronstarlite_amd import shim
    assert eng.stream.kernel_launches(shim.KTAG_FWD) == 0
    assert eng.stream.kernel_launches(shim.KTAG_BWD) == 0
    assert torch.equal(y, torch.full((4, f), 3.0, device=dev))
    eng.stream.timing(False)


def test_operator_surface(dev, bounded):
    from neutronstarlite_amd.ops import (HipEngine, SingleGPUFuseOp,
                                         aggregate)
    v, ch, dch = bounded
    f = 130
    eng = HipEngine()
    op = SingleGPUFuseOp(dch, eng)
    x16 = make_input(v, f, 5, dev, largest=False)
    g16 = make_input(v, f, 6, dev, largest=False)
    y = op.forward(x16)
    gx = op.backward(g16)
    assert y.dtype == torch.float32 and gx.dtype == torch.float32
    assert torch.equal(y, run(eng, dch, "fwd", x16))
    assert torch.equal(gx, run(eng, dch, "bwd", g16))
    assert torch.equal(y, op.forward(x16.float()))   # unsplit: to the bit
    assert torch.equal(gx, op.backward(g16.float()))

    # autograd: fp32 y from a bf16 leaf, whose .grad comes back as bf16
    leaf = x16.clone().requires_grad_(True)
    out = aggregate(leaf, dch, eng)
    assert out.dtype == torch.float32 and torch.equal(out, y)
    grad = g16.float()
    out.backward(grad)
    assert leaf.grad.dtype == torch.bfloat16
    assert torch.equal(leaf.grad,
                       run(eng, dch, "bwd", grad).to(torch.bfloat16))
    # an fp32 leaf keeps an fp32 gradient
    leaf32 = x16.float().requires_grad_(True)
    aggregate(leaf32, dch, eng).backward(grad)
    assert leaf32.grad.dtype == torch.float32
    assert torch.equal(leaf32.grad, run(eng, dch, "bwd", grad))


def test_minibatch_op_takes_bf16(dev):
    from neutronstarlite_amd.ops import (HipEngine, MiniBatchFuseOp,
                                         minibatch_aggregate)
    from neutronstarlite_amd.sampler import sample_subgraph
    v, e, f = 3000, 60000, 40
    edges = G.rmat_edges(v, e, seed=7)
    outd, ind = G.degrees(edges, v)
    ch = _chunk(edges, v)
    rng = np.random.default_rng(8)
    targets = rng.choice(v, size=256, replace=False).astype(np.uint32)
    layer = sample_subgraph(ch.column_offset, ch.row_indices, targets,
                            [10], outd, ind, seed=9)[0]
    op = MiniBatchFuseOp(layer, dev, HipEngine())
    x16 = make_input(layer.n_src, f, 3, dev, largest=False)
    g16 = make_input(layer.n_dst, f, 4, dev, largest=False)
    y = op.forward(x16)
    gx = op.backward(g16)
    assert y.dtype == torch.float32 and gx.dtype == torch.float32
    assert y.shape == (layer.n_dst, f) and gx.shape == (layer.n_src, f)
    # fan-in <= 10: forward vertices are never split, so to the bit
    assert torch.equal(y, op.forward(x16.float()))
    assert_close(gx, op.backward(g16.float()).cpu().numpy(), "minibatch bwd")
    leaf = x16.clone().requires_grad_(True)
    out = minibatch_aggregate(leaf, op)
    assert torch.equal(out, y)
    out.backward(g16.float())
    assert leaf.grad.dtype == torch.bfloat16


@pytest.mark.parametrize("bad", [torch.float16, torch.float64, torch.int16])
def test_other_dtypes_raise_before_any_launch(dev, bounded, bad):
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.ops import HipEngine, SingleGPUFuseOp
    v, ch, dch = bounded
    eng = HipEngine()
    eng.stream.timing(True)
    eng.stream.timing_reset()
    x = torch.ones(v, 8, device=dev).to(bad)
    y32 = torch.zeros(v, 8, device=dev)
    with pytest.raises(TypeError):
        eng.csc_forward(dch, x, y32)
    with pytest.raises(TypeError):
        eng.csr_backward(dch, x, y32)   # used to misread the bytes as fp32
    with pytest.raises(TypeError):
        SingleGPUFuseOp(dch, eng).forward(x)
    # the output is fp32, whatever the input
    for inp in (torch.ones(v, 8, device=dev),
                torch.ones(v, 8, device=dev, dtype=torch.bfloat16)):
        for out_dtype in (torch.bfloat16, torch.float64):
            out = torch.zeros(v, 8, device=dev, dtype=out_dtype)
            with pytest.raises(TypeError):
                eng.csc_forward(dch, inp, out)
            with pytest.raises(TypeError):
                eng.csr_backward(dch, inp, out)
            assert out.abs().max().item() == 0
    for tag in (shim.KTAG_FWD, shim.KTAG_BWD, shim.KTAG_ITEMS):
        assert eng.stream.kernel_launches(tag) == 0
    assert y32.abs().max().item() == 0
    eng.stream.timing(False)


@pytest.mark.parametrize("f", [136, 602])
def test_storage_rounding_bound(dev, bounded, f):
    """What storing the rows as bf16 costs, as a test: rounding x to bf16
    moves each element by at most 2^-8 |x| (bf16 keeps 8 significant bits,
    round to nearest), so the sums move by at most 2^-8 sum_e |w_e||x_e|; the
    second term is the project tolerance for the fp32 accumulation itself."""
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = bounded
    eng = HipEngine()
    x = torch.from_numpy(np.random.default_rng(f).uniform(
        -1, 1, (v, f)).astype(np.float32)).to(dev)
    y32 = run(eng, dch, "fwd", x)
    y16 = run(eng, dch, "fwd", x.to(torch.bfloat16))
    # sum_e |w_e||x_e| in float64 on the host
    dst = np.repeat(np.arange(v), np.diff(ch.column_offset.astype(np.int64)))
    a = torch.sparse_coo_tensor(
        torch.from_numpy(np.stack([dst, ch.row_indices.astype(np.int64)])),
        torch.from_numpy(np.abs(ch.edge_weight_forward).astype(np.float64)),
        (v, v))
    s = torch.sparse.mm(a, x.cpu().double().abs())
    bound = 2.0 ** -8 * s + (RTOL * y32.cpu().double().abs() + ATOL)
    err = (y16.cpu().double() - y32.cpu().double()).abs()
    print(f"f={f}: worst err/bound {(err / bound).max().item():.3f}")
    assert (err <= bound).all(), (
        f"{(err > bound).sum().item()} elements beyond the bound")
    assert err.max().item() > 0  # the rounding is really there
