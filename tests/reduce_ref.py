"""numpy reference of the max / min neighbour aggregation and its backward.

Forward, per destination d: np.argmax / np.argmin over the segment of
gathered rows, column by column.  Both return the FIRST occurrence and compare
with IEEE ==, so the lowest edge position wins a tie and -0 ties +0 — the
reference's serial write_max / write_min (strict <) without its
zero-initialised output.  A destination without in-edges gets 0 and NO_EDGE.
Backward: np.add.at in float64.  Pinned on hand-written cases in
tests/test_reduce_ref.py."""
import numpy as np

NO_EDGE = 0xFFFFFFFF


def _rows(row_indices, e0, e1, src_start):
    if row_indices is None:           # message form: edge e reads row e
        return np.arange(e0, e1)
    return row_indices[e0:e1].astype(np.int64) - src_start


def reduce_forward(column_offset, row_indices, x, op, src_start=0):
    """(y float32 [V, f], arg uint32 [V, f]) for op in {"max", "min"}."""
    pick = {"max": np.argmax, "min": np.argmin}[op]
    off = column_offset.astype(np.int64)
    v, f = len(off) - 1, x.shape[1]
    y = np.zeros((v, f), dtype=np.float32)
    arg = np.full((v, f), NO_EDGE, dtype=np.uint32)
    cols = np.arange(f)
    for d in range(v):
        e0, e1 = off[d], off[d + 1]
        if e1 == e0:
            continue
        seg = x[_rows(row_indices, e0, e1, src_start)]
        k = pick(seg, axis=0)
        y[d] = seg[k, cols]
        arg[d] = e0 + k
    return y, arg


def reduce_backward(arg, grad, row_indices, rows, src_start=0):
    """float64 [rows, f]: grad[d, c] added at the source row of edge
    arg[d, c] (row arg[d, c] itself when row_indices is None)."""
    gx = np.zeros((rows, grad.shape[1]), dtype=np.float64)
    d, c = np.nonzero(arg != NO_EDGE)
    e = arg[d, c].astype(np.int64)
    r = e if row_indices is None else row_indices[e].astype(np.int64) - src_start
    np.add.at(gx, (r, c), grad[d, c].astype(np.float64))
    return gx
