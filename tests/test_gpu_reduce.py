"""Max / min neighbour aggregation with its arg record, and the backward
scatter (marked gpu), against tests/reduce_ref.py.

There is no rounding in the forward: the output is one of the inputs and the
arg is the lowest edge position that attains it, so ANY differing element is
a bug.  That holds on split (hub) vertices too, whose work items merge through
64-bit atomic keys: the tie input makes the reference itself show a hub column
whose extremum sits at two positions in different work items, and the arg
must still be the lowest.  The backward adds with fp32 atomics in no fixed
order: exact for small-integer gradients, and within the worst-case bound of
an arbitrarily ordered fp32 sum otherwise."""
import os
import sys

import numpy as np
import pytest
import torch

from neutronstarlite_amd import graph as G

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

SPLIT = 256              # default max edges per work item (NTS_SPLIT)
WIDTHS = [1, 7, 33, 130, 132, 602]
# dwords per lane at 16-byte alignment: ragged strided tails (1, 7, 33),
# dwordx2 with a multi-slab row (130, 602), dwordx4 (132)
LANE = {1: 1, 7: 1, 33: 1, 130: 2, 132: 4, 602: 2}
OPS = ["max", "min"]
GRAPHS = ["bounded", "hub"]
NO_EDGE = R.NO_EDGE


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
    """V=2000, per-destination degree uniform in [0, 200], the first three
    at 0, sources uniform: no vertex reaches the work-item split."""
    from neutronstarlite_amd.ops import DeviceChunk
    v = 2000
    rng = np.random.default_rng(11)
    deg = rng.integers(0, 201, size=v)
    deg[:3] = 0
    dst = np.repeat(np.arange(v, dtype=np.uint32), deg)
    src = rng.integers(0, v, size=dst.size).astype(np.uint32)
    assert np.bincount(dst, minlength=v).max() <= SPLIT
    w = rng.uniform(0.1, 1.0, size=dst.size).astype(np.float32)
    ch = _chunk(np.stack([src, dst], axis=1), v, w)
    assert (degrees_of(ch)[:3] == 0).all()
    return v, ch, DeviceChunk(ch, dev)


@pytest.fixture(scope="module")
def hub(dev):
    """RMAT V=3000, E=60000 plus 5000 in-edges on vertex 0: vertex 0 (and
    the RMAT hubs) split into several work items, merged through keys."""
    from neutronstarlite_amd.ops import DeviceChunk
    v = 3000
    edges = G.rmat_edges(v, 60000, seed=7)
    star_src = np.random.default_rng(3).integers(0, v, 5000)
    star = np.stack([star_src, np.zeros_like(star_src)], axis=1)
    edges = np.concatenate([edges, star.astype(edges.dtype)])
    assert np.bincount(edges[:, 1], minlength=v).max() > SPLIT
    ch = _chunk(edges, v)
    assert int(ch.column_offset[1]) - int(ch.column_offset[0]) >= 5000
    return v, ch, DeviceChunk(ch, dev)


@pytest.fixture
def graph(request, bounded, hub):
    return {"bounded": bounded, "hub": hub}[request.param]


def degrees_of(ch):
    return np.diff(ch.column_offset.astype(np.int64))


# ---- inputs and the references, computed once per (graph, width, kind) ----
def continuous_input(ch, v, f, seed):
    """U(-1,1) with +-inf planted, one all -inf source row that the graph
    really reads, and one destination whose column 0 is -inf on every in-edge
    (under max its arg must still be its first edge)."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    flat = x.reshape(-1)
    where = rng.choice(flat.size, min(64, flat.size), replace=False)
    flat[where[::2]] = np.inf
    flat[where[1::2]] = -np.inf
    x[int(ch.row_indices[len(ch.row_indices) // 2])] = -np.inf
    deg = degrees_of(ch)
    d = int(np.nonzero((deg >= 2) & (deg <= 8))[0][0])
    e0, e1 = int(ch.column_offset[d]), int(ch.column_offset[d + 1])
    x[ch.row_indices[e0:e1].astype(np.int64), 0] = -np.inf
    assert not np.isnan(x).any()
    return x


def tie_input(v, f, seed):
    rng = np.random.default_rng(seed)
    vals = np.array([-2, -1, -0.0, +0.0, 1, 2], dtype=np.float32)
    return vals[rng.integers(0, len(vals), (v, f))]


_cache = {}


def case(name, ch, v, f, kind):
    """(x, {op: (y_ref, arg_ref)}), read-only, shared by the tests."""
    key = (name, f, kind)
    if key not in _cache:
        x = (continuous_input(ch, v, f, 1000 + f) if kind == "cont"
             else tie_input(v, f, 2000 + f))
        refs = {op: R.reduce_forward(ch.column_offset, ch.row_indices, x, op)
                for op in OPS}
        x.setflags(write=False)
        for pair in refs.values():
            for a in pair:
                a.setflags(write=False)
        _cache[key] = (x, refs)
    return _cache[key]


def garbage(shape, dev):
    """Pre-filled outputs: the entry must overwrite every row."""
    y = torch.full(shape, 123.25, device=dev)
    arg = torch.full(shape, 7, dtype=torch.int32, device=dev)
    return y, arg


def run_fwd(eng, dch, x_t, op, message=False):
    y, arg = garbage((dch.dst_n, x_t.shape[1]), x_t.device)
    eng.csc_reduce(dch, x_t, y, arg, op, message)
    return y, arg


def as_u32(arg_t):
    return arg_t.cpu().numpy().view(np.uint32)


def check_forward(y, arg, y_ref, arg_ref, ch, what):
    got_arg, got_y = as_u32(arg), y.cpu().numpy()
    bad = got_arg != arg_ref
    assert not bad.any(), (
        f"{what}: {bad.sum()} args differ, first at {np.argwhere(bad)[0]}: "
        f"got {got_arg[bad][0]} want {arg_ref[bad][0]}")
    assert np.array_equal(got_y, y_ref), (
        f"{what}: {(got_y != y_ref).sum()} values differ")
    zero = degrees_of(ch) == 0      # `bounded` has some, by construction
    assert (got_y[zero] == 0).all() and (got_arg[zero] == NO_EDGE).all()


def plan_of(dch, f, *tensors):
    from neutronstarlite_amd import shim
    align = 16
    for t in tensors:
        while t.data_ptr() % align:
            align //= 2
    return shim.reduce_plan(f, align, dch.dst_n, dch.edge_size)


# ---- 1 and 3: continuous input, exact; zero-degree rows; overwrite ----
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("graph", GRAPHS, indirect=True)
def test_continuous_input_is_exact(dev, graph, f, op, request):
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = graph
    name = request.node.callspec.params["graph"]
    x, refs = case(name, ch, v, f, "cont")
    eng = HipEngine()
    x_t = torch.tensor(x).to(dev)
    y, arg = run_fwd(eng, dch, x_t, op)
    assert plan_of(dch, f, x_t, y, arg)["vector_width"] == LANE[f]
    assert eng.stream.gather_schedule_last()[0] == 0   # NTS_SCHED_ITEM
    check_forward(y, arg, *refs[op], ch, f"{name} f={f} {op}")


# ---- 2: ties; the hub merge must keep the lowest position ----
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("graph", GRAPHS, indirect=True)
def test_ties_go_to_the_lowest_position(dev, graph, f, op, request):
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = graph
    name = request.node.callspec.params["graph"]
    x, refs = case(name, ch, v, f, "tie")
    y_ref, arg_ref = refs[op]
    if name == "hub":
        # from the reference alone: some column of hub vertex 0 attains its
        # extremum at two positions >= SPLIT apart, i.e. in two work items
        e0, e1 = int(ch.column_offset[0]), int(ch.column_offset[1])
        seg = x[ch.row_indices[e0:e1].astype(np.int64)]
        hit = seg == y_ref[0]
        first = hit.argmax(axis=0)
        last = len(seg) - 1 - hit[::-1].argmax(axis=0)
        assert (last - first >= SPLIT).any()
        assert (arg_ref[0] == e0 + first).all()
    y, arg = run_fwd(HipEngine(), dch, torch.tensor(x).to(dev), op)
    check_forward(y, arg, y_ref, arg_ref, ch, f"ties {name} f={f} {op}")


# ---- alignment: views 1 and 2 floats in force the strided / dwordx2 paths --
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("offset,lane", [(1, 1), (2, 2)])
@pytest.mark.parametrize("graph", GRAPHS, indirect=True)
def test_alignment_picks_the_lane_width(dev, graph, offset, lane, op,
                                        request):
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = graph
    f = 132
    name = request.node.callspec.params["graph"]
    x, refs = case(name, ch, v, f, "tie")

    def view(dtype, fill):
        flat = torch.full((v * f + 8,), fill, dtype=dtype, device=dev)
        t = flat[offset:offset + v * f].view(v, f)
        assert t.is_contiguous()
        assert t.data_ptr() == flat.data_ptr() + 4 * offset
        return t

    x_t = view(torch.float32, 0.0)
    x_t.copy_(torch.tensor(x))
    eng = HipEngine()
    # each of the three pointers alone must narrow the lanes
    for which in range(3):
        y, arg = garbage((v, f), dev)
        xin = x_t if which == 0 else torch.tensor(x).to(dev)
        if which == 1:
            y = view(torch.float32, 123.25)
        if which == 2:
            arg = view(torch.int32, 7)
        assert plan_of(dch, f, xin, y, arg)["vector_width"] == lane
        eng.csc_reduce(dch, xin, y, arg, op)
        check_forward(y, arg, *refs[op], ch,
                      f"{name} offset {offset} on pointer {which} {op}")


# ---- 4: the message form, forward and backward, both exact ----
@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("f", [1, 33])
def test_message_form(dev, bounded, f, op):
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = bounded
    e = ch.edge_size
    rng = np.random.default_rng(50 + f)
    msg = rng.uniform(-1, 1, (e, f)).astype(np.float32)
    msg[rng.integers(0, e, 16), rng.integers(0, f, 16)] = -np.inf
    y_ref, arg_ref = R.reduce_forward(ch.column_offset, None, msg, op)
    eng = HipEngine()
    y, arg = run_fwd(eng, dch, torch.from_numpy(msg).to(dev), op,
                     message=True)
    check_forward(y, arg, y_ref, arg_ref, ch, f"message f={f} {op}")
    g = rng.uniform(-1, 1, (v, f)).astype(np.float32)
    gm = torch.zeros(e, f, device=dev)
    eng.reduce_backward(dch, torch.from_numpy(g).to(dev), arg, gm,
                        message=True)
    # each target is written once: exact
    gm_ref = R.reduce_backward(arg_ref, g, None, e)
    assert np.array_equal(gm.cpu().numpy().astype(np.float64), gm_ref)


# ---- 5 and 6: the backward scatter ----
def backward_case(dev, graph, name, f, op, grad):
    from neutronstarlite_amd.ops import HipEngine
    v, ch, dch = graph
    x, refs = case(name, ch, v, f, "tie")   # ties: many gradients collide
    arg_ref = refs[op][1]
    arg_t = torch.from_numpy(arg_ref.view(np.int32).copy()).to(dev)
    gx = torch.zeros(v, f, device=dev)
    HipEngine().reduce_backward(dch, torch.from_numpy(grad).to(dev), arg_t,
                                gx)
    return gx.cpu().numpy(), arg_ref


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("graph", GRAPHS, indirect=True)
def test_backward_integer_gradients_bit_for_bit(dev, graph, f, op, request):
    name = request.node.callspec.params["graph"]
    v, ch, _ = graph
    grad = np.random.default_rng(70 + f).integers(
        -8, 9, (v, f)).astype(np.float32)
    got, arg_ref = backward_case(dev, graph, name, f, op, grad)
    ref = R.reduce_backward(arg_ref, grad, ch.row_indices, v)
    assert np.abs(ref).max() < 2 ** 24          # every partial sum is exact
    assert np.array_equal(got.astype(np.float64), ref), (
        f"{(got != ref).sum()} elements differ")
    assert np.abs(ref).max() > 8                # gradients really collide


@pytest.mark.parametrize("op", OPS)
@pytest.mark.parametrize("f", WIDTHS)
@pytest.mark.parametrize("graph", GRAPHS, indirect=True)
def test_backward_uniform_gradients_within_sum_bound(dev, graph, f, op,
                                                     request):
    """Per element |got - ref64| <= n * 2^-23 * sum|g_i|, n the number of
    terms added there: the worst case of an fp32 sum of n terms in any order
    ((n-1) * 2^-24 * sum|g_i| to first order), with a factor of two for the
    rounding of the comparison itself.  Derived, not tuned."""
    name = request.node.callspec.params["graph"]
    v, ch, _ = graph
    grad = np.random.default_rng(90 + f).uniform(
        -1, 1, (v, f)).astype(np.float32)
    got, arg_ref = backward_case(dev, graph, name, f, op, grad)
    ref = R.reduce_backward(arg_ref, grad, ch.row_indices, v)
    n = R.reduce_backward(arg_ref, np.ones_like(grad), ch.row_indices, v)
    mag = R.reduce_backward(arg_ref, np.abs(grad), ch.row_indices, v)
    err = np.abs(got.astype(np.float64) - ref)
    bound = n * 2.0 ** -23 * mag
    print(f"{name} f={f} {op}: max terms {int(n.max())}, worst err/bound "
          f"{(err / np.maximum(bound, 1e-300)).max():.3f}")
    assert (err <= bound).all(), (
        f"{(err > bound).sum()} elements beyond the bound")
    assert n.max() > 1


# ---- 7: autograd ----
@pytest.mark.parametrize("op", OPS)
def test_autograd_sum_backward(dev, bounded, op):
    from neutronstarlite_amd.ops import HipEngine, aggregate_reduce
    v, ch, dch = bounded
    f = 33
    x, refs = case("bounded", ch, v, f, "tie")
    y_ref, arg_ref = refs[op]
    leaf = torch.tensor(x).to(dev).requires_grad_(True)
    eng = HipEngine()
    y, arg = aggregate_reduce(leaf, dch, eng, op, return_arg=True)
    assert y.requires_grad and not arg.requires_grad
    assert np.array_equal(y.detach().cpu().numpy(), y_ref)
    assert np.array_equal(as_u32(arg), arg_ref)
    y.sum().backward()
    ref = R.reduce_backward(arg_ref, np.ones((v, f), np.float32),
                            ch.row_indices, v)
    assert leaf.grad.dtype == torch.float32
    assert np.array_equal(leaf.grad.cpu().numpy().astype(np.float64), ref)
    # the default return is y alone
    y2 = aggregate_reduce(leaf.detach(), dch, eng, op)
    assert torch.equal(y2, y.detach())


@pytest.mark.parametrize("op", OPS)
def test_edge_reduce_autograd(dev, bounded, op):
    from neutronstarlite_amd.ops import HipEngine, edge_reduce
    v, ch, dch = bounded
    f, e = 7, ch.edge_size
    msg = np.random.default_rng(5).integers(-3, 4, (e, f)).astype(np.float32)
    y_ref, arg_ref = R.reduce_forward(ch.column_offset, None, msg, op)
    leaf = torch.from_numpy(msg).to(dev).requires_grad_(True)
    y = edge_reduce(leaf, dch, HipEngine(), op)
    assert np.array_equal(y.detach().cpu().numpy(), y_ref)
    y.sum().backward()
    ref = R.reduce_backward(arg_ref, np.ones((v, f), np.float32), None, e)
    assert np.array_equal(leaf.grad.cpu().numpy().astype(np.float64), ref)


# ---- 8: the sampled-subgraph operator ----
@pytest.mark.parametrize("op", OPS)
def test_minibatch_reduce_pair(dev, op):
    from neutronstarlite_amd.ops import HipEngine, MiniBatchFuseOp
    from neutronstarlite_amd.sampler import sample_subgraph
    v, e, f = 3000, 60000, 40
    edges = G.rmat_edges(v, e, seed=7)
    outd, ind = G.degrees(edges, v)
    ch = _chunk(edges, v)
    rng = np.random.default_rng(8)
    targets = rng.choice(v, size=256, replace=False).astype(np.uint32)
    layer = sample_subgraph(ch.column_offset, ch.row_indices, targets,
                            [10], outd, ind, seed=9)[0]
    mb = MiniBatchFuseOp(layer, dev, HipEngine())
    x = tie_input(layer.n_src, f, 3)
    grad = rng.integers(-8, 9, (layer.n_dst, f)).astype(np.float32)
    y_ref, arg_ref = R.reduce_forward(layer.column_offset,
                                      layer.row_indices_local, x, op)
    y, arg = mb.reduce_forward(torch.tensor(x).to(dev), op)
    assert y.shape == (layer.n_dst, f) and arg.dtype == torch.int32
    assert np.array_equal(as_u32(arg), arg_ref)
    assert np.array_equal(y.cpu().numpy(), y_ref)
    gx = mb.reduce_backward(torch.from_numpy(grad).to(dev), arg)
    ref = R.reduce_backward(arg_ref, grad, layer.row_indices_local,
                            layer.n_src)
    assert gx.shape == (layer.n_src, f)
    assert np.array_equal(gx.cpu().numpy().astype(np.float64), ref)


# ---- the checks of the Python layer ----
def test_wrong_arguments_raise_before_any_launch(dev, bounded):
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.ops import HipEngine, aggregate_reduce
    v, ch, dch = bounded
    eng = HipEngine()
    eng.stream.timing(True)
    eng.stream.timing_reset()
    x = torch.ones(v, 8, device=dev)
    y, arg = garbage((v, 8), dev)
    with pytest.raises(ValueError):
        eng.csc_reduce(dch, x, y, arg, "sum")
    with pytest.raises(ValueError):
        aggregate_reduce(x, dch, eng, "mean")
    with pytest.raises(TypeError):
        eng.csc_reduce(dch, x.to(torch.bfloat16), y, arg, "max")
    with pytest.raises(TypeError):
        eng.csc_reduce(dch, x, y.double(), arg, "max")
    with pytest.raises(TypeError):
        eng.csc_reduce(dch, x, y, arg.long(), "max")
    with pytest.raises(TypeError):
        eng.csc_reduce(dch, x.cpu(), y, arg, "max")
    with pytest.raises(TypeError):
        eng.reduce_backward(dch, y.double(), arg, x)
    for tag in (shim.KTAG_FWD, shim.KTAG_BWD, shim.KTAG_ITEMS):
        assert eng.stream.kernel_launches(tag) == 0
    assert (y == 123.25).all() and (arg == 7).all()
    eng.stream.timing(False)


def test_edgeless_chunk_fills_every_row(dev):
    """edges == 0 with batch > 0 is not a no-op here: the entry overwrites,
    so every row becomes (0, NO_EDGE)."""
    from neutronstarlite_amd.ops import HipEngine
    eng = HipEngine()
    f = 33
    x = torch.ones(4, f, device=dev)
    y, arg = garbage((4, f), dev)
    off = torch.zeros(5, dtype=torch.int32, device=dev)
    idx = torch.zeros(1, dtype=torch.int32, device=dev)
    eng.stream.reduce_by_dst_from_src(
        "max", x.data_ptr(), y.data_ptr(), arg.data_ptr(), idx.data_ptr(),
        off.data_ptr(), 0, 4, 0, 4, 0, 4, f)
    assert (y == 0).all() and (as_u32(arg) == NO_EDGE).all()
