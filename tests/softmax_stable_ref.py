"""Float64 numpy references for the stable (max-subtracted) edge softmax of
nts_edge_softmax_stable, and the out-of-range inputs it is tested on, built
on tests/edge_ref.py and tests/heads_ref.py.  A helper module: no tests here.

  s[e] = exp(a[e] - M) / sum_e' exp(a[e'] - M),  M = max_e' a[e'],

per destination and per column or head.  A score of -inf on some, not all, of
a destination's edges gives exactly 0 there.

Regimes, all outside what the default arithmetic (fp32 exp / sum / divide,
edge_ref.softmax_forward's formula) can represent:
  huge    uniform in [-200, 200]
  high    normal with scale 2, plus 1000
  low     normal with scale 2, minus 1000
  equal   all 500 (the softmax is exactly 1/deg)
  masked  huge, with -inf on about 30 % of the entries of every (destination,
          column) of degree >= 2, never on all of them
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402

REGIMES = ("huge", "high", "low", "equal", "masked")
OFFSET = {"high": 1000.0, "low": -1000.0}   # exact in float32, see scores()


# --------------------------------------------------------------------------
# references
# --------------------------------------------------------------------------
def segment_max(x, offset):
    """(n_segments, f) float64 maxima of the rows of x (E, f) per segment;
    -inf for an empty segment."""
    off = np.asarray(offset, dtype=np.int64)
    x = np.asarray(x, dtype=np.float64)
    out = np.full((len(off) - 1,) + x.shape[1:], -np.inf)
    live = np.diff(off) > 0
    if live.any():
        out[live] = np.maximum.reduceat(x, off[:-1][live], axis=0)
    return out


def softmax_forward(column_offset, x):
    """Per destination and column: exp(x - max) / sum exp(x - max), float64
    from the given (float32) scores.  Every destination must keep at least
    one finite score per column."""
    x = np.asarray(x, dtype=np.float64)
    doe = R._dst_of_edge(column_offset)
    mx = segment_max(x, column_offset)
    assert np.isfinite(mx[np.diff(np.asarray(column_offset, np.int64)) > 0]).all()
    ex = np.exp(x - mx[doe])
    return ex / R.segment_sum(ex, column_offset)[doe]


def attention_forward(column_offset, row_indices, s_src, s_dst, mirror_index,
                      slope):
    """K heads: m = s_src[mirror_index[src], k] + s_dst[dst, k] (s_src[src]
    when mirror_index is None), leaky-relu, stable softmax per (destination,
    head).  s_src (rows, K), s_dst (batch, K).  Returns (m float32 (E, K),
    exactly what the kernel must store, and the float64 softmax (E, K))."""
    rows = np.asarray(row_indices).astype(np.int64)
    if mirror_index is not None:
        rows = np.asarray(mirror_index)[rows].astype(np.int64)
    ss = np.asarray(s_src, dtype=np.float32)
    sd = np.asarray(s_dst, dtype=np.float32)
    assert ss.ndim == 2 and sd.ndim == 2 and ss.shape[1] == sd.shape[1]
    with np.errstate(invalid="raise"):          # no inf - inf in the inputs
        m = ss[rows] + sd[R._dst_of_edge(column_offset)]
    assert m.dtype == np.float32
    m64 = m.astype(np.float64)
    a = np.where(m64 > 0, m64, float(np.float32(slope)) * m64)
    return m, softmax_forward(column_offset, a)


def default_fp32(column_offset, x):
    """What the default kernels' arithmetic gives in float32: exp, sum per
    destination, divide, no max subtraction (non-finite on every regime
    here)."""
    x = np.asarray(x, dtype=np.float32)
    doe = R._dst_of_edge(column_offset)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ex = np.exp(x)
        den = np.zeros((len(column_offset) - 1,) + x.shape[1:], np.float32)
        np.add.at(den, doe, ex)
        return ex / den[doe]


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def _mask(rng, column_offset, width, protect=None):
    """(E, width) bool, True on about 30 % of the entries of every
    (destination, column) of degree >= 2, never on all of one's entries, and
    never where protect (E, width) is True."""
    off = np.asarray(column_offset, dtype=np.int64)
    e = int(off[-1])
    mask = rng.random((e, width)) < 0.3
    deg = np.diff(off)
    doe = np.repeat(np.arange(len(deg)), deg)
    mask[deg[doe] < 2] = False
    if protect is not None:
        mask &= ~protect
    for d in np.flatnonzero(deg >= 2):
        seg = mask[off[d]:off[d + 1]]
        for c in np.flatnonzero(seg.all(axis=0)):
            seg[rng.integers(0, len(seg)), c] = False
    return mask


def scores(regime, e, f, seed=0, column_offset=None):
    """(e, f) float32 scores of the regime.  `high` and `low` are float32
    values x with x - OFFSET[regime] exact in float32 (|x| lies in [512,
    2048), so x is a multiple of 2^-14 and so is the small difference).
    `masked` needs the graph's column_offset."""
    rng = np.random.default_rng([seed, f, 100 + REGIMES.index(regime)])
    if regime in ("huge", "masked"):
        x = rng.uniform(-200.0, 200.0, size=(e, f)).astype(np.float32)
        if regime == "masked":
            x[_mask(rng, column_offset, f)] = -np.inf
    elif regime in OFFSET:
        x = (rng.normal(scale=2.0, size=(e, f)) + OFFSET[regime]).astype(
            np.float32)
    else:
        x = np.full((e, f), 500.0, dtype=np.float32)
    return x


def without_offset(regime, x):
    """The float32 scores x of `high` / `low` minus the regime's offset,
    asserted exact."""
    base = x - np.float32(OFFSET[regime])
    assert base.dtype == np.float32
    assert (base.astype(np.float64) + OFFSET[regime] == x.astype(np.float64)).all()
    return base


def attention_inputs(regime, g, heads, seed=0):
    """(s_src_full, s_src_mirror, s_dst), (rows, K) float32, whose sums m =
    s_src + s_dst reach the regime's range:
      huge, masked  both uniform in [-100, 100]
      high, low     both normal with scale 1, plus / minus 500
      equal         both 250
    As edge_ref.attention_inputs, on the first edge of every fifth live
    destination s_dst is minus that edge's source scalar, so m is exactly 0
    there (huge and masked only: elsewhere the regime is its offset).
    masked sets s_src to -inf on about 30 % of the sources, never on a source
    of an exact-zero edge and never on all in-edges of a destination.
    s_src_full is indexed by global source id, s_src_mirror by mirror row."""
    rng = np.random.default_rng([seed, heads, 200 + REGIMES.index(regime)])
    n = g.src_start + g.v_src
    off = g.column_offset.astype(np.int64)
    if regime in ("huge", "masked"):
        full = rng.uniform(-100, 100, (n, heads)).astype(np.float32)
        s_dst = rng.uniform(-100, 100, (g.batch, heads)).astype(np.float32)
        zero_dst = np.flatnonzero(g.deg > 0)[::5]
        for d in zero_dst:
            s_dst[d] = -full[g.row_indices[off[d]]]
        if regime == "masked":
            dead = rng.random((n, heads)) < 0.3
            dead[g.row_indices[off[zero_dst]]] = False
            for d in np.flatnonzero(g.deg > 0):
                srcs = g.row_indices[off[d]:off[d + 1]]
                for k in np.flatnonzero(dead[srcs].all(axis=0)):
                    dead[srcs[0], k] = False
            full[dead] = -np.inf
    elif regime in OFFSET:
        half = OFFSET[regime] / 2
        full = (rng.normal(size=(n, heads)) + half).astype(np.float32)
        s_dst = (rng.normal(size=(g.batch, heads)) + half).astype(np.float32)
    else:
        full = np.full((n, heads), 250.0, dtype=np.float32)
        s_dst = np.full((g.batch, heads), 250.0, dtype=np.float32)
    mirror = np.zeros((g.m, heads), dtype=np.float32)
    mirror[g.mirror_index[g.uniq]] = full[g.uniq]
    return full, mirror, s_dst
