"""Every path of k_sample_reservoir against the host model of
tests/sampler_ref.py, bit for bit and in order, on synthetic columns whose
sources encode the edge slot; then sample_layer_gpu's compaction."""
import os
import sys

import numpy as np
import pytest
import torch

from neutronstarlite_amd import graph as G

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sampler_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x5A5A5A5A       # no source id of these tests
CNT_SENT = 0x3C3C3C3C
GUARD = 256
DEV = torch.device("cuda:0")


@pytest.fixture(scope="module")
def st():
    from neutronstarlite_amd import shim
    return shim.Stream.wrap_torch_current()


def _dev(a):
    from neutronstarlite_amd.ops import _u32_cuda
    return _u32_cuda(np.ascontiguousarray(a, dtype=np.uint32), DEV)


class Launch:
    """One CSC and destination list on the device; run() launches an entry
    into sentinel-filled outputs and returns (out_src rows, the guard
    region after the last row, out_cnt, its guard)."""

    def __init__(self, coff, rows, dst):
        self.coff, self.rows = np.asarray(coff), np.asarray(rows)
        self.dst = np.asarray(dst, dtype=np.int64)
        self.d_coff = _dev(coff)
        self.d_rows = _dev(rows if len(rows) else [0])
        self.d_dst = torch.from_numpy(self.dst.astype(np.int32)).to(DEV)

    def run(self, entry, fanout, seed=S.SEED):
        n = len(self.dst)
        out_src = torch.full((n * fanout + GUARD,), SENT, dtype=torch.int32,
                             device=DEV)
        out_cnt = torch.full((n + GUARD,), CNT_SENT, dtype=torch.int32,
                             device=DEV)
        entry(self.d_coff.data_ptr(), self.d_rows.data_ptr(),
              self.d_dst.data_ptr(), n, fanout, seed, out_src.data_ptr(),
              out_cnt.data_ptr())
        torch.cuda.synchronize()
        src = out_src.cpu().numpy().view(np.uint32)
        cnt = out_cnt.cpu().numpy().view(np.uint32)
        return (src[:n * fanout].reshape(n, fanout), src[n * fanout:],
                cnt[:n], cnt[n:])

    def expected(self, fanout, seed=S.SEED, forced=False):
        """Per distinct destination: (src_ids, count, path)."""
        out = {}
        for d in np.unique(self.dst):
            info = {}
            src, cnt = S.expected_sample(self.coff, self.rows, int(d), fanout,
                                         seed, forced=forced, info=info)
            out[int(d)] = (src, cnt, info["path"])
        return out

    def check(self, entry, fanout, seed=S.SEED, forced=False, paths=None):
        """The four assertions of every case; returns the rows."""
        rows, guard, cnt, cnt_guard = self.run(entry, fanout, seed)
        want = self.expected(fanout, seed, forced)
        for i, d in enumerate(self.dst):
            src, k, path = want[int(d)]
            deg = int(self.coff[d + 1]) - int(self.coff[d])
            where = f"row {i} dst {d} deg {deg} fanout {fanout} path {path}"
            if paths is not None:
                assert path in paths, where
            assert k == min(deg, fanout)
            assert cnt[i] == k, where
            assert np.array_equal(rows[i, :k], src), where
            assert (rows[i, k:] == SENT).all(), where + ": wrote past cnt"
        assert (guard == SENT).all() and (cnt_guard == CNT_SENT).all()
        again = self.run(entry, fanout, seed)
        for a, b in zip((rows, guard, cnt, cnt_guard), again):
            assert np.array_equal(a, b), "second launch differs"
        return rows


def _case(deg):
    coff, rows = S.case_csc(deg)
    return Launch(coff, rows, [0, 1, 2])


@pytest.mark.parametrize("fanout", S.A_FANOUTS)
def test_path_a_copies_the_column(st, fanout):
    """deg 0, 1 and fanout; fanout 70 takes two 64-lane strides."""
    coff, rows = S.slot_csc([0, 1, fanout, fanout, 0, 1],
                            [0, 0, 0, S.REPEAT_MOD, 0, 0])
    Launch(coff, rows, range(6)).check(st.sample_reservoir, fanout,
                                       paths={"A"})


@pytest.mark.parametrize("deg,fanout", S.B_CASES)
def test_path_b_direct(st, deg, fanout):
    _case(deg).check(st.sample_reservoir, fanout, paths={"B"})


@pytest.mark.parametrize("deg,fanout", S.C_CASES)
def test_path_c_hub(st, deg, fanout):
    _case(deg).check(st.sample_reservoir, fanout, paths={"C"})


@pytest.mark.parametrize("deg,fanout", S.D_CASES)
def test_path_d_threshold(st, deg, fanout):
    """Through the normal entry: collection caps 4 * fanout and 1024, the
    window of width one at fanout 1024, and deg < 2 * fanout, where the
    first threshold exceeds 2^32."""
    _case(deg).check(st.sample_reservoir, fanout, paths={"D"})


@pytest.mark.parametrize("deg,fanout", S.B_CASES + S.D_CASES)
def test_forced_entry_equals_the_normal_one(st, deg, fanout):
    """The header's promise for nts_sample_reservoir_dbg_fallback: D' gives
    exactly what B and D give."""
    ln = _case(deg)
    forced = ln.check(st.sample_reservoir_dbg_fallback, fanout, forced=True,
                      paths={"D'"})
    normal = ln.run(st.sample_reservoir, fanout)[0]
    assert np.array_equal(forced, normal)


@pytest.mark.parametrize("fanout,normal", [(64, "ABC"), (65, "ABD")])
def test_mixed_block(st, fanout, normal):
    """One launch whose destinations cycle A, B, C, D kinds at period 4, so
    the four waves of every block, which share s_key / s_slot, each take
    another path and leave the loop by another `continue`; destinations
    repeat.  fanout 64 puts B beside C (and D' through the forced entry),
    fanout 65 puts B beside D."""
    coff, rows, dst, _ = S.mixed_case()
    ln = Launch(coff, rows, dst)
    got = {p for _, _, p in ln.expected(fanout).values()}
    assert got == set(normal)
    ln.check(st.sample_reservoir, fanout)
    ln.check(st.sample_reservoir_dbg_fallback, fanout, forced=True,
             paths={"A", "D'"})


@pytest.fixture(scope="module")
def many():
    """5000 columns of deg 16 then 1000 of deg 3, and each column's expected
    sample at fanout 4, computed once."""
    coff, rows = S.slot_csc([16] * 5000 + [3] * 1000)
    want = [S.expected_sample(coff, rows, d, 4, S.SEED) for d in range(6000)]
    table = np.full((6000, 4), SENT, dtype=np.uint32)
    for d, (src, k) in enumerate(want):
        table[d, :k] = src
    cnt = np.array([k for _, k in want], dtype=np.uint32)
    return coff, rows, table, cnt


def _check_table(st, many, dst):
    coff, rows, table, cnt = many
    got, guard, got_cnt, cnt_guard = Launch(coff, rows, dst).run(
        st.sample_reservoir, 4)
    assert np.array_equal(got_cnt, cnt[dst])
    assert np.array_equal(got, table[dst])      # the unwritten tail included
    assert (guard == SENT).all() and (cnt_guard == CNT_SENT).all()


def test_many_destinations(st, many):
    """5000 path-B destinations of deg 16, fanout 4: every row exact."""
    _check_table(st, many, np.arange(5000))


def test_more_destinations_than_waves(st, many):
    """The launch is capped at 8192 blocks of 4 waves, so past 32768
    destinations a wave walks `i += n_waves`: 40000 entries at period 5
    (four deg-16 columns, then a deg-3 one) make a wave's second
    destination another kind than its first, path A's `continue` before
    path B and the reverse."""
    i = np.arange(40000)
    dst = np.where(i % 5 == 4, 5000 + i % 1000, (i * 7) % 5000)
    _check_table(st, many, dst)


@pytest.mark.parametrize("path,deg,fanout",
                         [("B", 512, 32), ("C", 50000, 16), ("D", 2048, 128)])
def test_nearby_seeds_give_unrelated_samples_on_the_device(st, path, deg,
                                                           fanout):
    """The overlap conditions of test_sampler_ref.py, from kernel output:
    sources are slots here, so a row reads back as edge slots."""
    assert S.path_of(deg, fanout) == path
    coff, rows = S.slot_csc([deg] * 4)
    ln = Launch(coff, rows, range(4))
    e0 = coff[:4].astype(np.int64)[:, None]
    memo = {}

    def edges(seed):
        if seed not in memo:
            got, _, cnt, _ = ln.run(st.sample_reservoir, fanout, seed)
            assert (cnt == fanout).all()
            memo[seed] = e0 + got
        return memo[seed]

    for seed in (0, 1, 2, 99, 1000, 1001):
        for other, mask in S.overlap_pairs(seed):
            for d in range(4):
                S.check_overlap(edges(seed)[d], edges(other)[d], mask, fanout,
                                f"{path} dst {d}: seeds {seed}, {other}")


# ---- sample_layer_gpu: compaction of the kernel's raw output ----

@pytest.fixture(scope="module")
def rmat():
    from neutronstarlite_amd.ops import _u32_cuda
    dev = DEV
    v, e = 4000, 80000
    edges = G.rmat_edges(v, e, seed=7)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    ch = G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]
    targets = np.random.default_rng(1).choice(
        v, size=300, replace=False).astype(np.int32)
    return {"v": v, "ch": ch, "targets": targets,
            "d_coff": _u32_cuda(ch.column_offset, dev),
            "d_rows": _u32_cuda(ch.row_indices, dev),
            "d_outd": torch.from_numpy(outd.astype(np.int64)).to(dev),
            "d_ind": torch.from_numpy(ind.astype(np.int64)).to(dev)}


@pytest.fixture(scope="module")
def rmat_layer(st, rmat):
    from neutronstarlite_amd.sampler_gpu import sample_layer_gpu
    dst = torch.from_numpy(rmat["targets"]).to(DEV)
    ly = sample_layer_gpu(st, rmat["d_coff"], rmat["d_rows"], dst, 7,
                          rmat["d_outd"], rmat["d_ind"], seed=3)
    torch.cuda.synchronize()
    return ly


def _np(t):
    return t.cpu().numpy()


def test_layer_csr_is_the_transpose_of_its_csc(rmat_layer):
    """The (src_local, dst_local, weight) triples of the two views are the
    same multiset, weights bitwise; within a CSR row the destinations
    ascend (the stable-permutation contract)."""
    ly = rmat_layer
    co, ri = _np(ly.column_offset).astype(np.int64), _np(ly.row_indices_local)
    ro = _np(ly.row_offset).astype(np.int64)
    ci = _np(ly.column_indices_local)
    wf = _np(ly.edge_weight).view(np.uint32)
    wb = _np(ly.edge_weight_backward).view(np.uint32)
    e = ly.e_size
    assert e > 0 and co[0] == 0 and co[-1] == e and ro[0] == 0 and ro[-1] == e
    assert len(co) == ly.n_dst + 1 and len(ro) == ly.n_src + 1
    assert (np.diff(co) >= 0).all() and (np.diff(ro) >= 0).all()
    assert len(ri) == len(ci) == len(wf) == len(wb) == e
    assert ri.min() >= 0 and ri.max() < ly.n_src
    assert ci.min() >= 0 and ci.max() < ly.n_dst
    csc = sorted(zip(ri.tolist(), np.repeat(np.arange(ly.n_dst),
                                            np.diff(co)).tolist(),
                     wf.tolist()))
    csr = sorted(zip(np.repeat(np.arange(ly.n_src), np.diff(ro)).tolist(),
                     ci.tolist(), wb.tolist()))
    assert csc == csr
    for s in range(ly.n_src):
        assert (np.diff(ci[ro[s]:ro[s + 1]]) >= 0).all(), f"CSR row {s}"


def test_layer_sources_are_the_kernels_raw_picks(st, rmat, rmat_layer):
    """src is strictly increasing and src[row_indices_local] is the
    kernel's out_src, destination-major; that raw output is the model's
    sample of every target's real column."""
    ly, ch, targets = rmat_layer, rmat["ch"], rmat["targets"]
    src = _np(ly.src)
    assert (np.diff(src) > 0).all()
    ln = Launch(ch.column_offset, ch.row_indices, targets)
    rows = ln.check(st.sample_reservoir, 7, seed=3)
    deg = (ch.column_offset[targets + 1].astype(np.int64)
           - ch.column_offset[targets])
    cnt = np.minimum(deg, 7)
    assert np.array_equal(np.diff(_np(ly.column_offset).astype(np.int64)), cnt)
    raw = np.concatenate([rows[i, :cnt[i]] for i in range(len(targets))])
    assert np.array_equal(src[_np(ly.row_indices_local)], raw.astype(np.int64))


def _tiny_layer(st, coff, rows, n_vertices, targets):
    from neutronstarlite_amd.sampler_gpu import sample_layer_gpu
    deg = torch.arange(1, n_vertices + 1, dtype=torch.int64, device=DEV)
    ly = sample_layer_gpu(st, _dev(coff), _dev(rows),
                          torch.tensor(targets, dtype=torch.int32,
                                       device=DEV),
                          3, deg + 1, deg, seed=11)
    torch.cuda.synchronize()
    return ly


def test_empty_layer(st):
    """No target has an in-edge: an empty layer, whose forward is zero."""
    from neutronstarlite_amd.ops import HipEngine, MiniBatchFuseOp
    ly = _tiny_layer(st, [0] * 6, [0], 5, [4, 0, 2])
    assert (ly.e_size, ly.n_src, ly.n_dst) == (0, 0, 3)
    assert _np(ly.column_offset).tolist() == [0, 0, 0, 0]
    assert _np(ly.row_offset).tolist() == [0]
    for t in (ly.src, ly.row_indices_local, ly.column_indices_local,
              ly.edge_weight, ly.edge_weight_backward):
        assert t.numel() == 0
    op = MiniBatchFuseOp(ly, DEV, HipEngine())
    y = op.forward(torch.zeros(0, 6, device=DEV))
    gx = op.backward(torch.ones(3, 6, device=DEV))
    torch.cuda.synchronize()
    assert y.shape == (3, 6) and not y.any()
    assert gx.shape == (0, 6)


def test_one_edge_layer(st):
    """Vertex 3 -> vertex 1 is the only edge below the targets."""
    from neutronstarlite_amd.ops import HipEngine, MiniBatchFuseOp
    ly = _tiny_layer(st, [0, 0, 1, 1, 1, 1], [3], 5, [0, 1, 2])
    assert (ly.e_size, ly.n_src, ly.n_dst) == (1, 1, 3)
    assert _np(ly.src).tolist() == [3]
    assert _np(ly.column_offset).tolist() == [0, 0, 1, 1]
    assert _np(ly.row_indices_local).tolist() == [0]
    assert _np(ly.row_offset).tolist() == [0, 1]
    assert _np(ly.column_indices_local).tolist() == [1]
    # outd[v] = v + 2, ind[v] = v + 1
    w = np.float32(1.0) / (np.sqrt(np.float32(5.0)) * np.sqrt(np.float32(2.0)))
    assert np.allclose(_np(ly.edge_weight), [w], rtol=1e-6, atol=0)
    assert torch.equal(ly.edge_weight, ly.edge_weight_backward)
    op = MiniBatchFuseOp(ly, DEV, HipEngine())
    x = torch.tensor([[1.0, -2.0, 0.5]], device=DEV)
    gy = torch.tensor([[9.0, 9.0, 9.0], [2.0, 4.0, -8.0], [7.0, 7.0, 7.0]],
                      device=DEV)
    y, gx = op.forward(x), op.backward(gy)
    torch.cuda.synchronize()
    wd = float(_np(ly.edge_weight)[0])
    want_y = np.zeros((3, 3), dtype=np.float32)
    want_y[1] = np.float32(wd) * _np(x)[0]
    assert np.allclose(_np(y), want_y, rtol=1e-6, atol=0)
    assert np.allclose(_np(gx), np.float32(wd) * _np(gy)[1:2], rtol=1e-6,
                       atol=0)
