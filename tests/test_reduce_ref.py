"""tests/reduce_ref.py, the numpy reference of the max / min aggregation,
pinned on hand-written cases (CPU): a tie across positions, an all -inf
column, a +-0 tie, a destination without edges, and the message form."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import reduce_ref as R  # noqa: E402

INF = np.inf
NO = R.NO_EDGE

# three destinations: d0 has edges 0..3 from sources 2, 0, 2, 1; d1 has none;
# d2 has edge 4 from source 1
OFF = np.array([0, 4, 4, 5], dtype=np.uint32)
IDX = np.array([2, 0, 2, 1, 1], dtype=np.uint32)
#              col0  col1   col2   col3
X = np.array([[5.0, -INF, +0.0, -1.0],     # source 0
              [5.0, -INF, 3.0, -7.0],      # source 1
              [1.0, -INF, -0.0, -1.0]],    # source 2
             dtype=np.float32)


def test_max_hand_case():
    y, arg = R.reduce_forward(OFF, IDX, X, "max")
    assert y.dtype == np.float32 and arg.dtype == np.uint32
    # d0 gathers sources (2, 0, 2, 1):
    #   col0 (1, 5, 1, 5): the tie at positions 1 and 3 goes to 1
    #   col1 all -inf: a valid arg, the first edge
    #   col2 (-0, +0, -0, 3): 3 at position 3
    #   col3 (-1, -1, -1, -7): first of three equal
    assert arg[0].tolist() == [1, 0, 3, 0]
    assert y[0].tolist() == [5.0, -INF, 3.0, -1.0]
    assert arg[1].tolist() == [NO] * 4 and y[1].tolist() == [0.0] * 4
    assert arg[2].tolist() == [4] * 4
    assert np.array_equal(y[2], X[1])


def test_min_hand_case_and_zero_tie():
    y, arg = R.reduce_forward(OFF, IDX, X, "min")
    #   col0 (1, 5, 1, 5): tie at 0 and 2 goes to 0
    #   col2 (-0, +0, -0, 3): -0 == +0, so the first, position 0, wins
    #   col3 (-1, -1, -1, -7): -7 at position 3
    assert arg[0].tolist() == [0, 0, 0, 3]
    assert y[0].tolist() == [1.0, -INF, 0.0, -7.0]
    assert np.signbit(y[0, 2])          # the value at the winning position
    # and under max the zero tie goes to the first position too
    x = np.array([[+0.0], [-0.0], [-0.0]], dtype=np.float32)
    off = np.array([0, 3], dtype=np.uint32)
    idx = np.array([1, 0, 2], dtype=np.uint32)
    for op in ("max", "min"):
        y, arg = R.reduce_forward(off, idx, x, op)
        assert arg.tolist() == [[0]] and y[0, 0] == 0.0


def test_src_start_is_subtracted():
    y, arg = R.reduce_forward(OFF, IDX + 10, X, "max", src_start=10)
    y0, arg0 = R.reduce_forward(OFF, IDX, X, "max")
    assert np.array_equal(y, y0) and np.array_equal(arg, arg0)


def test_message_form():
    msg = X[IDX.astype(np.int64)]       # [E, f]: what the edges would carry
    for op in ("max", "min"):
        y, arg = R.reduce_forward(OFF, None, msg, op)
        y0, arg0 = R.reduce_forward(OFF, IDX, X, op)
        assert np.array_equal(y, y0) and np.array_equal(arg, arg0)
    g = np.arange(12, dtype=np.float32).reshape(3, 4) + 1
    gm = R.reduce_backward(arg0, g, None, len(IDX))
    assert gm.shape == (5, 4) and gm.dtype == np.float64
    # every target written at most once: row arg[d, c] holds g[d, c]
    want = np.zeros((5, 4))
    for d in (0, 2):
        for c in range(4):
            want[arg0[d, c], c] = g[d, c]
    assert np.array_equal(gm, want)


def test_backward_sums_collisions_and_skips_no_edge():
    _, arg = R.reduce_forward(OFF, IDX, X, "max")   # [[1,0,3,0],NO,[4]*4]
    g = np.array([[1, 2, 3, 4], [100, 100, 100, 100], [10, 20, 30, 40]],
                 dtype=np.float32)
    gx = R.reduce_backward(arg, g, IDX, 3)
    # d0: col0 -> edge 1 = source 0, col1 -> edge 0 = source 2,
    #     col2 -> edge 3 = source 1, col3 -> edge 0 = source 2
    # d2: every column -> edge 4 = source 1; d1 contributes nothing
    want = np.array([[1, 0, 0, 0],
                     [10, 20, 33, 40],
                     [0, 2, 0, 4]], dtype=np.float64)
    assert np.array_equal(gx, want)
