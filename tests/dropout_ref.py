"""Attention dropout: a numpy restatement of the keep mask and float64
references of the dropped edge softmax, forward and backward, built on
tests/edge_ref.py.  A helper module: no tests here.

The mask is written from its definition (include/nts_hip.h), not from the
library's code:

  fmix64(z): z = (z ^ (z >> 33)) * 0xff51afd7ed558ccd
             z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53;  return z ^ (z >> 33)
  base  = fmix64(seed)
  u     = fmix64(base + i) >> 40            24 bits, i = e*K + k
  T     = lrintf(float32(p) * 2^24)
  keep  = u >= T
  scale = float32(1) / (float32(1) - float32(p))
  w     = keep ? alpha * scale : 0

all in uint64 arithmetic modulo 2^64 (numpy arrays wrap silently).
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import edge_ref as R  # noqa: E402

_C1 = np.uint64(0xff51afd7ed558ccd)
_C2 = np.uint64(0xc4ceb9fe1a85ec53)
_S33 = np.uint64(33)


def fmix64(z):
    z = np.atleast_1d(np.asarray(z, dtype=np.uint64))
    z = (z ^ (z >> _S33)) * _C1
    z = (z ^ (z >> _S33)) * _C2
    return z ^ (z >> _S33)


def threshold(p):
    """T: a position drops iff its 24-bit draw is below it."""
    return int(np.rint(np.float32(p) * np.float32(16777216.0)))


def scale(p):
    """float32 1 / (1 - p), the factor of a kept weight."""
    return np.float32(1.0) / (np.float32(1.0) - np.float32(p))


def keep_mask(seed, p, first, count):
    """bool (count,): keep of positions first .. first + count - 1."""
    base = fmix64(np.array([seed], dtype=np.uint64))
    i = np.array([first], dtype=np.uint64) + np.arange(count, dtype=np.uint64)
    u = fmix64(base + i) >> np.uint64(40)
    return u >= np.uint64(threshold(p))


def keep_edges(seed, p, edges, k):
    """bool (edges, k): keep[e, c] of position e*k + c, e the CSC position."""
    return keep_mask(seed, p, 0, edges * k).reshape(edges, k)


def factor(keep, p):
    """float64 (keep ? scale : 0), scale being the float32 value."""
    return np.where(keep, np.float64(scale(p)), 0.0)


def softmax_forward(column_offset, x, keep, p):
    """(alpha, w): the float64 softmax of x (E, K) per destination and
    column, and the dropped weights alpha * (keep ? scale : 0)."""
    alpha = R.softmax_forward(column_offset, x)
    return alpha, alpha * factor(np.asarray(keep).reshape(alpha.shape), p)


def softmax_backward(column_offset, grad_w, alpha, keep, p, lrelu_in=None,
                     slope=0.0, dst_prefill=None):
    """edge_ref.softmax_backward with the gradient of alpha that the dropped
    weights pass on: g = grad_w * (keep ? scale : 0).  Same returns."""
    g = np.asarray(grad_w, dtype=np.float64)
    g = g * factor(np.asarray(keep).reshape(g.shape), p)
    return R.softmax_backward(column_offset, g, alpha, lrelu_in, slope,
                              dst_prefill)
