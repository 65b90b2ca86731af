"""Attention dropout on the CPU: the library's exported keep decision
(shim.edge_dropout_keep, the function the kernels run) against the numpy
restatement of tests/dropout_ref.py, the statistics of that mask, and the
float64 references of dropout_ref.py against dense loops on a hand graph."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dropout_ref as D  # noqa: E402

SEEDS = (0, 1, 2, 12345, 2**63 + 5)
N = 2**20


@pytest.mark.parametrize("first", [0, 2**40 + 3])
@pytest.mark.parametrize("p", [0.0, 0.1, 0.5, 0.6, 0.9])
@pytest.mark.parametrize("seed", SEEDS)
def test_exported_mask_is_the_restatement(seed, p, first):
    """Element for element, from position 0 and from 2^40 + 3, where an index
    truncated to 32 bits would show; p = 0 keeps everything."""
    from neutronstarlite_amd import shim
    count = 5000
    got = shim.edge_dropout_keep(seed, p, first, count)
    assert got.dtype == np.bool_ and got.shape == (count,)
    want = D.keep_mask(seed, p, first, count)
    assert (got == want).all(), f"{(got != want).sum()} of {count} differ"
    if p == 0.0:
        assert got.all()
    else:
        assert not got.all() and got.any()
    if first and p:   # the high bits of the position matter
        assert (want != D.keep_mask(seed, p, first & 0xFFFFFFFF, count)).any()


def test_exported_mask_checks_its_arguments():
    from neutronstarlite_amd import shim
    for p in (-0.1, 1.0, 1.5, "0.5", None, True, 1 - 2.0**-30):
        with pytest.raises(ValueError):
            shim.edge_dropout_keep(0, p, 0, 4)
    for seed in (-1, 2**64, 1.5, None, True):
        with pytest.raises(ValueError):
            shim.edge_dropout_keep(seed, 0.5, 0, 4)
    with pytest.raises(ValueError):
        shim.edge_dropout_keep(0, 0.5, -1, 4)
    assert shim.edge_dropout_keep(0, 0.5, 7, 0).shape == (0,)


def _within(frac, prob, name):
    sigma = np.sqrt(prob * (1 - prob) / N)
    z = abs(frac - prob) / sigma
    assert z <= 4.0, f"{name}: {frac:.6f} is {z:.2f} sigma from {prob:.6f}"
    return z


@pytest.mark.parametrize("p", [0.1, 0.5, 0.6, 0.9])
@pytest.mark.parametrize("seed", SEEDS)
def test_mask_statistics(seed, p):
    """On the first 2^20 positions, each within 4 binomial sigma (N = 2^20):
    the kept fraction of 1 - T/2^24; the agreement with the mask of seed + 1,
    with the mask one position on (adjacent heads) and eight positions on
    (adjacent edges at K = 8) of q = p^2 + (1-p)^2, what independent masks
    give.  Fixed seeds: nothing here can flake."""
    keep = D.keep_mask(seed, p, 0, N + 8)
    nxt = D.keep_mask(seed + 1, p, 0, N)
    q = p * p + (1 - p) * (1 - p)
    zs = [_within(keep[:N].mean(), 1 - D.threshold(p) / 2.0**24, "kept"),
          _within((keep[:N] == nxt).mean(), q, "seed + 1"),
          _within((keep[:N] == keep[1:N + 1]).mean(), q, "i, i + 1"),
          _within((keep[:N] == keep[8:N + 8]).mean(), q, "i, i + 8")]
    print(f"seed {seed} p {p}: worst {max(zs):.2f} sigma")


def test_threshold_and_scale():
    assert D.threshold(0.0) == 0 and D.threshold(0.5) == 2**23
    assert D.threshold(0.6) == int(np.rint(np.float32(0.6) * 2.0**24))
    assert D.scale(0.0) == np.float32(1) and D.scale(0.5) == np.float32(2)
    assert D.scale(0.6).dtype == np.float32


# the hand graph: 6 destinations over 6 sources, in-degrees 3, 0, 1, 4, 2, 2
COFF = np.array([0, 3, 3, 4, 8, 10, 12], dtype=np.uint32)
ROWS = np.array([1, 2, 5, 0, 0, 1, 3, 4, 2, 2, 5, 3], dtype=np.uint32)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("with_lrelu", [False, True])
def test_references_against_dense_loops(k, with_lrelu):
    """Forward (alpha, w) and backward of dropout_ref on the 6-vertex hand
    graph, against loops over destinations, edges and columns that apply
    the softmax Jacobian term by term."""
    seed, p, slope = 3, 0.5, 0.2
    e = len(ROWS)
    rng = np.random.default_rng(4)
    x = rng.normal(size=(e, k)).astype(np.float32)
    gw = rng.normal(size=(e, k)).astype(np.float32)
    lin = rng.normal(size=(e, k)).astype(np.float32) if with_lrelu else None
    pre = rng.normal(size=6).astype(np.float32)
    keep = D.keep_edges(seed, p, e, k)
    assert keep.any() and not keep.all()
    alpha, w = D.softmax_forward(COFF, x, keep, p)
    if k == 1:
        v, _, dsum, _ = D.softmax_backward(COFF, gw, alpha, keep, p, lin,
                                           slope, pre)
    else:
        v, _ = D.softmax_backward(COFF, gw, alpha, keep, p, lin, slope)

    sc = float(D.scale(p))
    a_ref, w_ref, v_ref = (np.zeros((e, k)) for _ in range(3))
    d_ref = pre.astype(np.float64)
    for d in range(6):
        rng_e = range(int(COFF[d]), int(COFF[d + 1]))
        for c in range(k):
            den = sum(np.exp(float(x[i, c])) for i in rng_e)
            for i in rng_e:
                a_ref[i, c] = np.exp(float(x[i, c])) / den
                w_ref[i, c] = a_ref[i, c] * sc if keep[i, c] else 0.0
            for i in rng_e:       # dL/dx_i = sum_j dL/dw_j dw_j/dx_i
                t = 0.0
                for j in rng_e:
                    dw_da = sc if keep[j, c] else 0.0
                    da_dx = a_ref[j, c] * ((1.0 if i == j else 0.0)
                                           - a_ref[i, c])
                    t += float(gw[j, c]) * dw_da * da_dx
                if with_lrelu:
                    t *= 1.0 if lin[i, c] > 0 else float(np.float32(slope))
                v_ref[i, c] = t
                if k == 1:
                    d_ref[d] += t
    np.testing.assert_allclose(alpha, a_ref, rtol=1e-13, atol=1e-15)
    np.testing.assert_allclose(w, w_ref, rtol=1e-13, atol=1e-15)
    assert ((w == 0) == ~keep).all()
    np.testing.assert_allclose(v, v_ref, rtol=1e-11, atol=1e-13)
    if k == 1:
        np.testing.assert_allclose(dsum, d_ref, rtol=1e-11, atol=1e-13)
