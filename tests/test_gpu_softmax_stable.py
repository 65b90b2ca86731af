"""The stable (max-subtracted) edge softmax, Stream.edge_softmax_stable(1),
against the float64 references of tests/softmax_stable_ref.py (marked gpu).

Graphs are edge_ref's: edge_case_graph (about 22k edges: degrees on both
sides of the 64-lane stride and of the 256-edge split and its multiples, a
degree-5000 hub, zero degree at both ends and in the middle), small_graph
(one split destination), tiny_graph (nothing split) and empty_graph.  They
cover a destination that is one work item (its (max, sum) pair is stored
plainly), one that is several (maxima merged by an atomic max, sums added by
the split items' own pass), a short
last item and a ragged lane stride.  The split is assumed to be the default
of 256.  Buffers follow tests/test_gpu_edge_kernels.py: guard bands of
sentinel floats that must come back bit-unchanged, outputs that start as NaN.

The inputs are the five regimes of softmax_stable_ref (scores to +-200, near
+-1000, all 500, and -inf on a strict subset of a destination's edges); on
each of them the default arithmetic is non-finite (test_softmax_stable_ref.py).

Bounds, none taken from what the kernels give: see _assert_softmax.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import softmax_stable_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = np.float32(-12345.678)
SLOPE = 0.2
TINY = 1e-30   # below this reference value only 0 <= got <= 2e-30 is asked


# --------------------------------------------------------------------------
# buffers and comparisons (the pattern of test_gpu_edge_kernels.py)
# --------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


class Buf:
    """A float32 device buffer of `shape` between two guard bands; filled
    with NaN, or with `fill`."""

    def __init__(self, dev, shape, fill=None):
        shape = tuple(int(x) for x in np.atleast_1d(shape))
        self.shape, self.n = shape, int(np.prod(shape))
        host = np.full(self.n + 2 * GUARD, SENTINEL, dtype=np.float32)
        body = host[GUARD:GUARD + self.n]
        body[:] = np.nan if fill is None else np.asarray(
            fill, dtype=np.float32).reshape(-1)
        self.before = host
        self.t = torch.from_numpy(host.copy()).to(dev)

    @property
    def ptr(self):
        return self.t.data_ptr() + 4 * GUARD

    @property
    def prefill(self):
        return self.before[GUARD:GUARD + self.n].reshape(self.shape)

    def read(self, name):
        torch.cuda.synchronize()
        after = self.t.cpu().numpy()
        for side, sl in (("front", slice(0, GUARD)),
                         ("back", slice(GUARD + self.n, None))):
            assert (_bits(after[sl]) == _bits(self.before[sl])).all(), (
                f"{name}: {side} guard band overwritten")
        return after[GUARD:GUARD + self.n].reshape(self.shape)

    def assert_untouched(self, name):
        got = self.read(name)
        assert (_bits(got) == _bits(self.prefill)).all(), (
            f"{name}: written although there was nothing to do")


def _assert_bits(got, want, name):
    bad = _bits(got) != _bits(want)
    assert not bad.any(), f"{name}: {bad.sum()}/{bad.size} not bit-equal"


def _assert_softmax(got, ref, g, name, dead=None):
    """Finite everywhere; where ref >= 1e-30, |got - ref| <= 1e-4*|ref| (the
    project's bar, purely relative as in test_softmax_forward); below that
    0 <= got <= 2e-30; every live (destination, column) sums to 1 within
    1e-4; where `dead` (a -inf score), exactly +0.0f.

    Expected error of a value with ref >= 1e-30.  All terms are positive, so
    nothing cancels.  Such a value has x = a - M >= ln(1e-30) + ln S >= -69.1
    (ref = exp(x)/S and the sum S of exp(a' - M) is at least 1); the figures
    below take |x| <= 78, which is more than that.
      - a - M is one fp32 subtraction of two fp32 numbers: exact by Sterbenz
        in the +-1000 regimes, otherwise rounded at 2^-24*|x| <= 4.7e-6
        absolute in the exponent, so 4.7e-6 relative in exp(x);
      - __expf scales its argument by log2(e): x*log2(e) rounds at
        2^-24*113, times ln 2, another 4.7e-6, plus the hardware exp2 at
        about 1e-7;
      - S of an unsplit destination: a term exp(a' - M) is built as
        exp(a' - m) times at most a few rescales exp(m - m') along increasing
        maxima (a lane's running maximum, then the item's), whose arguments
        add up to a' - M and at most double the total magnitude rounded, so
        a term at depth t = M - a' carries about 2*1.2e-7*t; weighted by
        exp(-t)/S this is largest for one term at 0 and the rest at
        t = ln(deg) + 1, where it is 1.5e-6 at most.  S of a split one is a
        plain sum of exp(a' - M) with the exact M, each term as the value
        itself.  Terms below exp(-87) flush to 0 and weigh under 1e-37 of S.
        The additions themselves: at most 4 per lane, 6 butterfly steps and
        the 20 atomic adds of the hub's items at 2^-24 each, 1.8e-6;
      - one division, 6e-8.
    Together about 1.3e-5, a margin of about 8 under 1e-4."""
    assert np.isfinite(got).all(), f"{name}: non-finite output"
    assert (got >= 0).all(), f"{name}: negative weight"
    big = ref >= TINY
    err = np.abs(got.astype(np.float64) - ref)
    ratio = np.where(big, err / np.where(big, 1e-4 * ref, 1.0), 0.0)
    worst = float(ratio.max()) if ratio.size else 0.0
    print(f"{name}: worst {worst:.3e} of the bound")
    assert worst <= 1.0, (f"{name}: {(ratio > 1).sum()}/{ratio.size} out of "
                          f"bound, worst {worst:.3e} of it")
    assert (got[~big] <= 2 * TINY).all(), f"{name}: a value below 1e-30"
    total = R.segment_sum(got, g.column_offset)
    live = g.deg > 0
    if live.any():
        off1 = float(np.abs(total[live] - 1).max())
        print(f"{name}: row sums within {off1:.3e} of 1")
        assert off1 <= 1e-4, f"{name}: a destination sums to 1 +- {off1:.3e}"
    if dead is not None:
        assert dead.any()
        assert (_bits(got[dead]) == 0).all(), (
            f"{name}: a masked edge is not exactly +0.0f")


# --------------------------------------------------------------------------
# device state
# --------------------------------------------------------------------------
class DevGraph:
    def __init__(self, g, dev):
        def up32(a):
            return torch.from_numpy(
                np.array(a, order="C").view(np.int32)).to(dev)
        self.g = g
        self.coff = up32(g.column_offset)
        self.rows = up32(g.row_indices)
        self.mi = up32(g.mirror_index)
        self.pos_np = R.csc_to_csr(g.row_indices)[1]
        self.pos = up32(self.pos_np.astype(np.uint32))


@pytest.fixture(scope="module")
def gpu():
    assert torch.cuda.is_available()
    dev = torch.device("cuda:0")
    from neutronstarlite_amd import shim
    env = {"dev": dev, "shim": shim,
           "auto": shim.Stream.wrap_torch_current(),
           "general": shim.Stream.wrap_torch_current(),
           "big": DevGraph(R.edge_case_graph(), dev),
           "small": DevGraph(R.small_graph(), dev),
           "tiny": DevGraph(R.tiny_graph(), dev),
           "empty": DevGraph(R.empty_graph(), dev)}
    env["auto"].edge_softmax_stable(1)
    env["general"].edge_softmax_stable(1)
    env["general"].heads_dbg_general(1)
    env["up"] = lambda a: torch.from_numpy(np.array(a, order="C")).to(dev)
    yield env
    env["auto"].destroy()
    env["general"].destroy()


# --------------------------------------------------------------------------
# the two softmax entries
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _softmax_case(key, regime, f):
    g = {"big": R.edge_case_graph, "small": R.small_graph}[key]()
    if regime == "wide":
        x = R.softmax_scores("wide", g.edges, f)
    else:
        x = S.scores(regime, g.edges, f, column_offset=g.column_offset)
    ref = S.softmax_forward(g.column_offset, x)
    x.setflags(write=False)
    ref.setflags(write=False)
    return x, ref


def _check_softmax_entries(gpu, key, regime, f):
    dg, st, dev = gpu[key], gpu["auto"], gpu["dev"]
    g = dg.g
    x, ref = _softmax_case(key, regime, f)
    dead = np.isneginf(x) if regime == "masked" else None
    d_x = gpu["up"](x)
    shape = (g.edges, f)
    tag = f"stable softmax {key} f={f} {regime}"

    out, cached = Buf(dev, shape), Buf(dev, shape)
    st.edge_softmax_forward(out.ptr, d_x.data_ptr(), cached.ptr,
                            dg.rows.data_ptr(), dg.coff.data_ptr(), g.batch, f)
    assert st.edge_softmax_stable_last() == 1
    plain = out.read(tag)
    _assert_softmax(plain, ref, g, tag, dead)
    _assert_bits(cached.read(tag), plain, tag + " cached")

    for cmode in ("separate", "null", "output"):
        name = f"{tag} dual, cached {cmode}"
        out, out2 = Buf(dev, shape), Buf(dev, shape)
        cached = Buf(dev, shape) if cmode == "separate" else None
        cptr = (cached.ptr if cached is not None
                else out.ptr if cmode == "output" else None)
        st.edge_softmax_forward_dual(out.ptr, out2.ptr, dg.pos.data_ptr(),
                                     d_x.data_ptr(), cptr, dg.coff.data_ptr(),
                                     g.batch, f)
        got = out.read(name)
        _assert_softmax(got, ref, g, name, dead)
        got2 = out2.read(name)
        assert np.isfinite(got2).all(), f"{name}: permuted slot not written"
        _assert_bits(got2[dg.pos_np], got, name + " permuted output")
        if cached is not None:
            _assert_bits(cached.read(name), got, name + " cached")
    return plain, ref


@pytest.mark.parametrize("regime", S.REGIMES)
@pytest.mark.parametrize("f", [1, 3, 8])
def test_softmax_forward_stable(gpu, f, regime):
    """Plain and _dual (the CSC-to-CSR map as perm_pos; msg_cached separate,
    null, and equal to the output) on the edge-case graph."""
    plain, ref = _check_softmax_entries(gpu, "big", regime, f)
    if regime == "equal":
        g = R.edge_case_graph()
        assert np.allclose(ref, (1.0 / g.deg[g.dst_of_edge])[:, None],
                           rtol=1e-15, atol=0)


def test_softmax_forward_stable_small_graph(gpu):
    """A second topology: 40 destinations, one of them split in two."""
    _check_softmax_entries(gpu, "small", "masked", 3)
    _check_softmax_entries(gpu, "small", "high", 1)


@pytest.mark.parametrize("f", [1, 8])
def test_in_range_agreement(gpu, f):
    """At edge_ref's `wide` regime, uniform in [-30, 30], where the default is
    defined, the stable output meets the default's bound against the default's
    reference (equal to the stable reference to 1e-12 there,
    test_softmax_stable_ref.py)."""
    plain, ref = _check_softmax_entries(gpu, "big", "wide", f)
    g = R.edge_case_graph()
    x, _ = _softmax_case("big", "wide", f)
    ref_default = R.softmax_forward(g.column_offset, x)
    err = np.abs(plain - ref_default)
    assert (err <= 1e-4 * np.abs(ref_default)).all()


# --------------------------------------------------------------------------
# the two attention entries
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _attention_case(key, regime, heads):
    g = {"big": R.edge_case_graph, "small": R.small_graph}[key]()
    full, mirror, s_dst = S.attention_inputs(regime, g, heads)
    m_ref, s_ref = S.attention_forward(g.column_offset, g.row_indices, mirror,
                                       s_dst, g.mirror_index, SLOPE)
    return full, mirror, s_dst, m_ref, s_ref


def _run_attention(gpu, st, dg, entry, heads, s_src, s_dst, with_mirror,
                   with_perm, name):
    g, dev = dg.g, gpu["dev"]
    d_src, d_dst = gpu["up"](s_src), gpu["up"](s_dst)
    shape = (g.edges, heads)
    out, msum = Buf(dev, shape), Buf(dev, shape)
    out2 = Buf(dev, shape) if with_perm else None
    args = (out.ptr, out2.ptr if out2 else None,
            dg.pos.data_ptr() if out2 else None, msum.ptr, d_src.data_ptr(),
            d_dst.data_ptr(), dg.rows.data_ptr(),
            dg.mi.data_ptr() if with_mirror else None, SLOPE,
            dg.coff.data_ptr(), g.batch)
    if entry == "single":
        st.edge_attention_forward(*args)
    else:
        st.edge_attention_forward_heads(*args, g.edges, heads)
    assert st.edge_softmax_stable_last() == 1
    got_m, got = msum.read(name), out.read(name)
    got2 = out2.read(name) if out2 else None
    return got_m, got, got2


def _check_attention(gpu, key, regime, heads, form, entry="heads"):
    dg, st = gpu[key], gpu[form]
    g = dg.g
    full, mirror, s_dst, m_ref, s_ref = _attention_case(key, regime, heads)
    dead = np.isneginf(m_ref) if regime == "masked" else None
    if regime in ("huge", "masked"):
        assert (m_ref == 0).any()
    for with_mirror, with_perm in ((True, True), (False, False)):
        name = (f"stable attention {key} K={heads} {form} {entry} {regime} "
                f"mirror={with_mirror} perm={with_perm}")
        got_m, got, got2 = _run_attention(
            gpu, st, dg, entry, heads, mirror if with_mirror else full, s_dst,
            with_mirror, with_perm, name)
        assert not np.isnan(got_m).any(), f"{name}: m_sum slot not written"
        _assert_bits(got_m, m_ref, name + " m_sum")
        _assert_softmax(got, s_ref, g, name, dead)
        if got2 is not None:
            assert np.isfinite(got2).all(), f"{name}: permuted slot not written"
            _assert_bits(got2[dg.pos_np], got, name + " permuted output")


@pytest.mark.parametrize("regime", S.REGIMES)
@pytest.mark.parametrize("heads,form", [(1, "auto"), (2, "auto"), (3, "auto"),
                                        (8, "auto"), (8, "general")])
def test_attention_forward_stable(gpu, heads, form, regime):
    """nts_edge_attention_forward_heads at K = 1 (the single-head kernel), 2
    and 8 (the flat form), 3 (the general form) and 8 through
    heads_dbg_general; with mirror_index and perm_pos, and with neither.
    m_sum_out is one fp32 add, bit-equal to numpy float32 (-inf where the
    source is masked); the softmax as _assert_softmax, the activations being
    leaky_relu(m) in [-40, 200], 1000, -200 or 500; the permuted copy bit-equal
    through the slot map."""
    _check_attention(gpu, "big", regime, heads, form)


@pytest.mark.parametrize("regime", S.REGIMES)
def test_attention_forward_single_entry_stable(gpu, regime):
    """nts_edge_attention_forward itself."""
    _check_attention(gpu, "big", regime, 1, "auto", entry="single")


def test_attention_forward_stable_small_graph(gpu):
    _check_attention(gpu, "small", "masked", 2, "auto")
    _check_attention(gpu, "small", "huge", 3, "auto")


# --------------------------------------------------------------------------
# nothing to do, and the mode itself
# --------------------------------------------------------------------------
def test_zero_degree_batch_writes_nothing(gpu):
    """On a batch whose destinations all have degree 0 the four entries leave
    their prefilled outputs bit-unchanged in stable mode too."""
    dg, st, dev = gpu["empty"], gpu["auto"], gpu["dev"]
    g = dg.g
    assert g.edges == 0 and g.batch == 7
    rng = np.random.default_rng(6200)
    rows, coff, mi = dg.rows.data_ptr(), dg.coff.data_ptr(), dg.mi.data_ptr()
    f, heads = 3, 4
    inp = gpu["up"](rng.normal(size=(32, 4)).astype(np.float32))
    idx = gpu["up"](np.arange(16, dtype=np.int32))
    mk = lambda *shape: Buf(dev, shape, rng.normal(size=shape) + 1)
    a, c = mk(8, f), mk(8, f)
    st.edge_softmax_forward(a.ptr, inp.data_ptr(), c.ptr, rows, coff,
                            g.batch, f)
    a.assert_untouched("edge_softmax_forward")
    c.assert_untouched("edge_softmax_forward")
    a, b, c = mk(8, f), mk(8, f), mk(8, f)
    st.edge_softmax_forward_dual(a.ptr, b.ptr, idx.data_ptr(), inp.data_ptr(),
                                 c.ptr, coff, g.batch, f)
    for buf in (a, b, c):
        buf.assert_untouched("edge_softmax_forward_dual")
    a, b, c = mk(8), mk(8), mk(8)
    st.edge_attention_forward(a.ptr, b.ptr, idx.data_ptr(), c.ptr,
                              inp.data_ptr(), inp.data_ptr(), rows, mi, SLOPE,
                              coff, g.batch)
    for buf in (a, b, c):
        buf.assert_untouched("edge_attention_forward")
    a, b, c = mk(8, heads), mk(8, heads), mk(8, heads)
    st.edge_attention_forward_heads(a.ptr, b.ptr, idx.data_ptr(), c.ptr,
                                    inp.data_ptr(), inp.data_ptr(), rows, mi,
                                    SLOPE, coff, g.batch, 0, heads)
    for buf in (a, b, c):
        buf.assert_untouched("edge_attention_forward_heads")


def _tiny_default(gpu, st):
    """Default-regime softmax (f = 3) and attention (K = 1 and 2) outputs of
    tiny_graph on stream st, with what edge_softmax_stable_last reported."""
    dg, dev = gpu["tiny"], gpu["dev"]
    g = dg.g
    outs, modes = [], []
    x = R.softmax_scores("normal", g.edges, 3, seed=31)
    out = Buf(dev, (g.edges, 3))
    st.edge_softmax_forward(out.ptr, gpu["up"](x).data_ptr(), None,
                            dg.rows.data_ptr(), dg.coff.data_ptr(), g.batch, 3)
    outs.append(out.read("tiny softmax"))
    modes.append(st.edge_softmax_stable_last())
    for heads in (1, 2):
        per = [R.attention_inputs(g, seed=40 + k) for k in range(heads)]
        mirror, s_dst = (np.stack([p[i] for p in per], axis=1) for i in (1, 2))
        _, got, _ = _run_attention_any(gpu, st, dg, heads, mirror, s_dst)
        outs.append(got)
        modes.append(st.edge_softmax_stable_last())
    return outs, modes


def _run_attention_any(gpu, st, dg, heads, s_src, s_dst):
    g, dev = dg.g, gpu["dev"]
    d_src, d_dst = gpu["up"](s_src), gpu["up"](s_dst)
    out, msum = Buf(dev, (g.edges, heads)), Buf(dev, (g.edges, heads))
    st.edge_attention_forward_heads(
        out.ptr, None, None, msum.ptr, d_src.data_ptr(), d_dst.data_ptr(),
        dg.rows.data_ptr(), dg.mi.data_ptr(), SLOPE, dg.coff.data_ptr(),
        g.batch, g.edges, heads)
    return msum.read("tiny attention"), out.read("tiny attention"), None


def test_mode_reporting_and_default_not_disturbed(gpu):
    """edge_softmax_stable_last() is 0 on a fresh stream and after a default
    call, 1 after a stable call.  On a stream where the mode was set, used
    and cleared again, the default outputs on tiny_graph (nothing split: one
    wave reduction in a fixed order, one atomic add onto zero) are bit-equal
    to those of a fresh stream.  The stable outputs in between agree with
    the default ones within 2e-4 relative: in range each is within 1e-4 of
    the same float64 reference."""
    shim = gpu["shim"]
    fresh, used = (shim.Stream.wrap_torch_current() for _ in range(2))
    try:
        assert fresh.edge_softmax_stable_last() == 0
        base, modes = _tiny_default(gpu, fresh)
        assert modes == [0, 0, 0]
        used.edge_softmax_stable(1)
        stable, modes = _tiny_default(gpu, used)
        assert modes == [1, 1, 1]
        used.edge_softmax_stable(0)
        again, modes = _tiny_default(gpu, used)
        assert modes == [0, 0, 0]
        for i, (a, b, c) in enumerate(zip(base, again, stable)):
            _assert_bits(b, a, f"default after the mode was cleared, case {i}")
            assert np.isfinite(c).all()
            assert (np.abs(c - a.astype(np.float64)) <= 2e-4 * a).all(), (
                f"stable against default in range, case {i}")
    finally:
        fresh.destroy()
        used.destroy()
