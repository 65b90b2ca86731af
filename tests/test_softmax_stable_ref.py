"""tests/softmax_stable_ref.py against tests/edge_ref.py and heads_ref.py
where both are defined, and the properties of its regimes that the GPU tests
of the stable softmax rely on (no GPU here)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402
import softmax_stable_ref as S  # noqa: E402

SLOPE = 0.2
GRAPHS = {"big": R.edge_case_graph, "small": R.small_graph,
          "tiny": R.tiny_graph}


def _rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if a.size else 0.0


@pytest.mark.parametrize("regime", R.SCORE_REGIMES)
@pytest.mark.parametrize("f", [1, 3])
def test_equals_edge_ref_in_range(regime, f):
    """Where exp cannot overflow, subtracting the maximum changes nothing
    beyond float64 rounding."""
    g = R.edge_case_graph()
    x = R.softmax_scores(regime, g.edges, f)
    assert _rel(S.softmax_forward(g.column_offset, x),
                R.softmax_forward(g.column_offset, x)) <= 1e-12


@pytest.mark.parametrize("heads", [1, 3])
@pytest.mark.parametrize("with_mirror", [True, False])
def test_attention_equals_heads_ref_in_range(heads, with_mirror):
    g = R.edge_case_graph()
    per_head = [R.attention_inputs(g, seed=k) for k in range(heads)]
    full, mirror, s_dst = (np.stack([p[i] for p in per_head], axis=1)
                           for i in range(3))
    args = (g.column_offset, g.row_indices, mirror if with_mirror else full,
            s_dst, g.mirror_index if with_mirror else None, SLOPE)
    m, s = S.attention_forward(*args)
    m_ref, s_ref = H.attention_forward(*args)
    assert (m.view(np.int32) == m_ref.view(np.int32)).all()
    assert _rel(s, s_ref) <= 1e-12
    if heads == 1:
        m1, s1 = R.attention_forward(args[0], args[1], args[2][:, 0],
                                     args[3][:, 0], args[4], SLOPE)
        assert (m[:, 0].view(np.int32) == m1.view(np.int32)).all()
        assert _rel(s[:, 0], s1) <= 1e-12


@pytest.mark.parametrize("regime", ["high", "low"])
def test_offset_regimes_equal_their_base(regime):
    """float32 scores that differ by a common offset exact in float32 have
    the same float64 softmax; the base is in edge_ref's range."""
    g = R.edge_case_graph()
    x = S.scores(regime, g.edges, 3)
    base = S.without_offset(regime, x)
    assert np.abs(base).max() < 30
    got = S.softmax_forward(g.column_offset, x)
    assert _rel(got, S.softmax_forward(g.column_offset, base)) <= 1e-12
    assert _rel(got, R.softmax_forward(g.column_offset, base)) <= 1e-12


def test_equal_regime_is_one_over_degree():
    g = R.edge_case_graph()
    got = S.softmax_forward(g.column_offset, S.scores("equal", g.edges, 2))
    assert np.allclose(got, (1.0 / g.deg[g.dst_of_edge])[:, None],
                       rtol=1e-15, atol=0)


@pytest.mark.parametrize("name", sorted(GRAPHS))
@pytest.mark.parametrize("f", [1, 3, 8])
def test_masked_keeps_a_finite_score(name, f):
    """About 30 % masked where the degree allows it, never a whole
    (destination, column); masked entries are exactly 0 in the reference and
    every live destination still sums to 1."""
    g = GRAPHS[name]()
    x = S.scores("masked", g.edges, f, column_offset=g.column_offset)
    dead = np.isneginf(x)
    assert np.isfinite(x[~dead]).all()
    live = g.deg > 0
    kept = R.segment_sum((~dead).astype(np.float64), g.column_offset)
    assert (kept[live] >= 1).all()
    assert not dead[(g.deg < 2)[g.dst_of_edge]].any()
    many = (g.deg >= 2)[g.dst_of_edge]
    assert 0.2 < dead[many].mean() < 0.35
    ref = S.softmax_forward(g.column_offset, x)
    assert (ref[dead] == 0).all() and (ref[~dead] > 0).all()
    assert np.abs(R.segment_sum(ref, g.column_offset)[live] - 1).max() < 1e-12


@pytest.mark.parametrize("regime", S.REGIMES)
@pytest.mark.parametrize("heads", [1, 3])
def test_attention_inputs(regime, heads):
    """m is one float32 add without inf - inf; the activations reach the
    regime's range; exact zeros and masked edges where promised; the two
    source layouts hold the same values."""
    g = R.edge_case_graph()
    full, mirror, s_dst = S.attention_inputs(regime, g, heads)
    m, s = S.attention_forward(g.column_offset, g.row_indices, mirror, s_dst,
                               g.mirror_index, SLOPE)
    m2, s2 = S.attention_forward(g.column_offset, g.row_indices, full, s_dst,
                                 None, SLOPE)
    assert (m.view(np.int32) == m2.view(np.int32)).all() and (s == s2).all()
    assert not np.isnan(m).any() and not np.isposinf(m).any()
    live = g.deg > 0
    assert np.abs(R.segment_sum(s, g.column_offset)[live] - 1).max() < 1e-12
    if regime in ("huge", "masked"):
        assert (m == 0).any() and m.max() > 150
        assert m[np.isfinite(m)].min() < -150
    if regime == "masked":
        dead = np.isneginf(m)
        assert 0.2 < dead.mean() < 0.35
        assert (s[dead] == 0).all()
    else:
        assert np.isfinite(m).all()
    if regime == "high":
        assert m.min() > 900
    if regime == "low":
        assert m.max() < -900
    if regime == "equal":
        assert (m == 500).all()


@pytest.mark.parametrize("regime", S.REGIMES)
def test_regimes_exceed_the_default_arithmetic(regime):
    """A plain float32 exp / sum / divide is non-finite somewhere on every
    regime (so the default mode cannot pass the GPU tests of the stable
    one), for the scores and for the attention activations."""
    g = R.edge_case_graph()
    x = S.scores(regime, g.edges, 3, column_offset=g.column_offset)
    assert not np.isfinite(S.default_fp32(g.column_offset, x)).all()
    full, _, s_dst = S.attention_inputs(regime, g, 2)
    m, _ = S.attention_forward(g.column_offset, g.row_indices, full, s_dst,
                               None, SLOPE)
    a = np.where(m > 0, m, np.float32(SLOPE) * m).astype(np.float32)
    assert not np.isfinite(S.default_fp32(g.column_offset, a)).all()
