"""Stripes of the staged PHASE gather (k_gather_spmm_stripe; marked gpu).

A striped launch cuts the 128-float window into stripes of sf floats; a wave
runs one (work item, window, stripe) at a time, its 256 / sf sub-groups split
the item's edges and their partial sums are added by a fixed butterfly.  So
an unsplit vertex is no longer bit-identical to the unstriped launch (several
fmaf chains and a tree replace one chain): it is held to the project
tolerance against the CPU oracle, and to bit-equality between two runs.
Split vertices merge with atomics, as before.

Staging is forced, PHASE over 128-float windows is requested and the stripe
width is forced throughout; every case asserts that stripes really ran."""
import numpy as np
import pytest
import torch

import oracle
from neutronstarlite_amd import graph as G

pytestmark = pytest.mark.gpu

RTOL, ATOL = 1e-4, 1e-5  # the project tolerance (test_gpu_parity.py)
SPLIT = 256              # default max edges per work item (NTS_SPLIT)

PHASE, FORCE = 1, 1
WINDOW = 128
WIDTHS = (32, 130, 602, 608)
STRIPES = (16, 32, 64, 128)


def check_close(got, ref, name):
    got = got.detach().cpu().numpy()
    err = np.abs(got - ref)
    over = err - (RTOL * np.abs(ref) + ATOL)
    print(f"{name}: max abs err {err.max():.3e}, worst err - tol "
          f"{over.max():.3e}")
    bad = over > 0
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} out of tolerance"


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _chunk(edges, v, weights):
    return G.build_chunks(edges, weights, np.array([0, v], dtype=np.uint32),
                          0)[0]


@pytest.fixture(scope="module")
def bounded_graph():
    """The graph of tests/test_gpu_gather_sched.py: V=2000, per-destination
    degree uniform in [0, 200] (zero-degree vertices included), sources
    uniform; no vertex reaches the work-item split in either direction."""
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


# in-edge counts around P (2..16 sub-groups), 4 P and NTS_SPLIT, and a hub
TAIL_DEGREES = (1, 2, 7, 8, 9, 31, 32, 33, 255, 256, 257)
HUB_EDGES = 3000


@pytest.fixture(scope="module")
def tails_graph():
    """V=64: destination k has TAIL_DEGREES[k] in-edges, destination 20 is a
    hub of 3000 (split into 12 work items, merged by atomics); the rest have
    none.  Sources are uniform, so every source has about 70 out-edges."""
    v = 64
    rng = np.random.default_rng(5)
    deg = np.zeros(v, dtype=np.int64)
    deg[:len(TAIL_DEGREES)] = TAIL_DEGREES
    deg[20] = HUB_EDGES
    dst = np.repeat(np.arange(v, dtype=np.uint32), deg)
    src = rng.integers(0, v, size=dst.size).astype(np.uint32)
    edges = np.stack([src, dst], axis=1)
    w = rng.uniform(0.1, 1.0, size=dst.size).astype(np.float32)
    assert sorted(np.bincount(dst, minlength=v)[:11]) == sorted(TAIL_DEGREES)
    return v, _chunk(edges, v, w)


_refs = {}


def reference(tag, ch, v, f, direction, with_weight):
    """(input, oracle output), computed once per case and shared"""
    key = (tag, f, direction, with_weight)
    if key not in _refs:
        x = np.random.default_rng(f).uniform(-1, 1, (v, f)).astype(np.float32)
        if direction == "fwd":
            w = ch.edge_weight_forward
            ones = np.ones_like(w)
            ref = oracle.csc_forward(ch.column_offset, ch.row_indices,
                                     w if with_weight else ones, x, 0, v, f)
        else:
            w = ch.edge_weight_backward
            ones = np.ones_like(w)
            ref = oracle.csr_backward(ch.row_offset, ch.column_indices,
                                      w if with_weight else ones, x, 0, v, f)
        ref.setflags(write=False)
        _refs[key] = (x, ref)
    return _refs[key]


def striped_engine(sf):
    from neutronstarlite_amd.ops import HipEngine
    eng = HipEngine()
    eng.stream.gather_staging(FORCE)
    eng.stream.gather_schedule(PHASE, WINDOW)
    eng.stream.gather_stripes(sf)
    return eng


def run(eng, dch, direction, inp, with_weight, out=None, stripe=None):
    rows = dch.dst_n if direction == "fwd" else dch.src_n
    if out is None:
        out = torch.zeros(rows, inp.shape[1], device=inp.device)
    if direction == "fwd":
        eng.csc_forward(dch, inp, out, with_weight)
    else:
        eng.csr_backward(dch, inp, out, with_weight)
    if stripe is not None:
        # striped for real: the case cannot pass by falling back
        sf, per_wave = eng.stream.gather_stripes_last()
        assert sf == stripe and per_wave >= 1
        assert eng.stream.gather_schedule_last() == (PHASE, WINDOW)
        assert eng.stream.gather_staging_last() == (
            True, -(-inp.shape[1] // 32) * 32)
    return out


@pytest.mark.parametrize("sf", STRIPES)
@pytest.mark.parametrize("f", WIDTHS)
def test_unsplit_graph_matches_oracle_and_repeats(dev, bounded_graph, f, sf):
    from neutronstarlite_amd.ops import DeviceChunk
    v, ch = bounded_graph
    dch = DeviceChunk(ch, dev)
    eng = striped_engine(sf)
    for direction in ("fwd", "bwd"):
        for with_weight in (True, False):
            x, ref = reference("bounded", ch, v, f, direction, with_weight)
            xt = torch.from_numpy(x).to(dev)
            name = f"f={f} sf={sf} {direction} w={with_weight}"
            got = run(eng, dch, direction, xt, with_weight, stripe=sf)
            check_close(got, ref, name)
            again = run(eng, dch, direction, xt, with_weight, stripe=sf)
            assert torch.equal(got, again), (
                f"{name}: {(got != again).sum().item()} elements differ "
                "between two runs")


@pytest.mark.parametrize("sf", STRIPES)
@pytest.mark.parametrize("f", [130, 602])
def test_tails_and_split_hub_match_oracle(dev, tails_graph, f, sf):
    from neutronstarlite_amd.ops import DeviceChunk
    v, ch = tails_graph
    dch = DeviceChunk(ch, dev)
    eng = striped_engine(sf)
    for direction in ("fwd", "bwd"):
        for with_weight in (True, False):
            x, ref = reference("tails", ch, v, f, direction, with_weight)
            got = run(eng, dch, direction, torch.from_numpy(x).to(dev),
                      with_weight, stripe=sf)
            check_close(got, ref, f"tails f={f} sf={sf} {direction} "
                                  f"w={with_weight}")


@pytest.mark.parametrize("sf", [16, 128])
def test_accumulates_into_the_output(dev, bounded_graph, sf):
    """out comes back as what it held plus the aggregation; rows of
    zero-degree vertices are left exactly as they were."""
    from neutronstarlite_amd.ops import DeviceChunk
    v, ch = bounded_graph
    f = 602
    dch = DeviceChunk(ch, dev)
    eng = striped_engine(sf)
    pattern = (np.arange(v * f, dtype=np.float32).reshape(v, f) % 13) - 6.0
    for direction, offset in (("fwd", ch.column_offset),
                              ("bwd", ch.row_offset)):
        x, ref = reference("bounded", ch, v, f, direction, True)
        out = torch.from_numpy(pattern.copy()).to(dev)
        run(eng, dch, direction, torch.from_numpy(x).to(dev), True, out=out,
            stripe=sf)
        check_close(out, pattern + ref, f"accumulate sf={sf} {direction}")
        empty = np.flatnonzero(np.diff(offset.astype(np.int64)) == 0)
        assert empty.size or direction == "bwd"  # sources all have out-edges
        assert np.array_equal(out.cpu().numpy()[empty], pattern[empty])


def test_never_is_the_unstriped_staged_launch(dev, bounded_graph):
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    v, ch = bounded_graph
    f = 602
    dch = DeviceChunk(ch, dev)
    x, _ = reference("bounded", ch, v, f, "fwd", True)
    xt = torch.from_numpy(x).to(dev)
    plain = HipEngine()  # no stripe request: a schedule request runs as before
    plain.stream.gather_staging(FORCE)
    plain.stream.gather_schedule(PHASE, WINDOW)
    base = run(plain, dch, "fwd", xt, True)
    assert plain.stream.gather_stripes_last() == (0, 0)
    eng = striped_engine(32)
    run(eng, dch, "fwd", xt, True, stripe=32)
    eng.stream.gather_stripes(-1)
    got = run(eng, dch, "fwd", xt, True)
    assert eng.stream.gather_stripes_last() == (0, 0)
    assert eng.stream.gather_schedule_last() == (PHASE, WINDOW)
    assert eng.stream.gather_staging_last() == (True, 608)
    assert torch.equal(got, base)
