"""Graph loading, partitioning and chunk construction for the aggregation hot path.

MI355X-native rebuild of the host-side structures behind NeutronStarLite's
neighbor-aggregation path (all citations into /root/reference):

  - Gemini binary edge format: consecutive (src,dst) u32 pairs, 8 B/edge
    (data/reddit/note_for_input.txt; loader core/graph.hpp:1127+).
  - Degrees of the loaded edge list, clamped >=1 (core/graph.hpp:4397-4401),
    feeding nts_norm_degree = 1/sqrt(outdeg(src)*indeg(dst))
    (core/ntsBaseOp.hpp:194-197).
  - Degree-balanced 1-D vertex-range partitioning (core/graph.hpp:1186-1213):
    ranges chosen so owned_edges + alpha*owned_vertices is balanced.
  - Per-source-partition chunks with forward CSC + backward CSR + per-edge
    weights (CSC_segment_pinned, core/GraphSegment.h:52-139, built by
    PartitionedGraph::PartitionToChunks, core/PartitionedGraph.hpp:324-420):
    column_offset local over the owned dst range, row_indices global src ids;
    row_offset local over the chunk's src range, column_indices global dst ids.

This module is pure host-side plumbing (numpy); the compute path is the HIP
extension (csrc/nts_hip.hip behind include/nts_hip.h).
"""
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import List

import numpy as np


def _parallel_blocks(fn, n: int, block: int):
    """Run fn(lo, hi) over [0, n) in `block`-sized pieces on a small thread
    pool (numpy releases the GIL inside its loops)."""
    spans = [(lo, min(lo + block, n)) for lo in range(0, n, block)]
    workers = min(16, len(os.sched_getaffinity(0)), len(spans))
    if workers <= 1:
        for lo, hi in spans:
            fn(lo, hi)
        return
    with ThreadPoolExecutor(workers) as pool:
        for _ in pool.map(lambda s: fn(*s), spans):
            pass


def _take(a: np.ndarray, idx: np.ndarray, dtype=None) -> np.ndarray:
    """a[idx] (optionally cast to dtype), gathered blockwise in parallel."""
    out = np.empty(len(idx), dtype=dtype or a.dtype)

    def block(lo, hi):
        out[lo:hi] = a[idx[lo:hi]]

    _parallel_blocks(block, len(idx), 1 << 22)
    return out


def _stable_order(key: np.ndarray) -> np.ndarray:
    """argsort(key, kind="stable") for u32-ranged integer keys: sort the
    unique composite (key << 32 | position) — one plain u64 sort instead of
    a stable argsort — and take the positions back out."""
    n = len(key)
    assert n < (1 << 32)
    comp = np.empty(n, dtype=np.uint64)
    order = np.empty(n, dtype=np.int64)

    def pack(lo, hi):
        comp[lo:hi] = key[lo:hi]
        comp[lo:hi] <<= np.uint64(32)
        comp[lo:hi] |= np.arange(lo, hi, dtype=np.uint64)

    def unpack(lo, hi):
        order[lo:hi] = comp[lo:hi] & np.uint64(0xFFFFFFFF)

    _parallel_blocks(pack, n, 1 << 22)
    comp.sort()
    _parallel_blocks(unpack, n, 1 << 22)
    return order


def load_gemini_edges(path: str) -> np.ndarray:
    """Read a Gemini binary edge file: (src,dst) u32 pairs, 8 B/edge."""
    raw = np.fromfile(path, dtype=np.uint32)
    assert raw.size % 2 == 0, f"odd u32 count in {path}"
    return raw.reshape(-1, 2)


def rmat_edges(v: int, e: int, seed: int = 7,
               a: float = 0.57, b: float = 0.19, c: float = 0.19,
               add_self_loops: bool = True) -> np.ndarray:
    """Synthetic power-law graph: RMAT (a,b,c,d) with d = 1-a-b-c, plus
    optional self-loops (the BASELINE configs use `.edge.self` inputs).

    Vectorized: for each of ceil(log2(v)) levels, draw one quadrant choice
    per edge. Returns (E',2) u32 with E' = e (+v if self-loops)."""
    scale = int(np.ceil(np.log2(max(v, 2))))
    t0, t1, t2 = np.cumsum([a, b, c])  # quadrant split by one uniform draw
    edges = np.empty((e + (v if add_self_loops else 0), 2), dtype=np.uint32)
    base = np.random.PCG64(seed).state

    # The draws are those of ONE default_rng(seed) stream taken level by
    # level (level L, edge i = draw L*e + i; random() uses one 64-bit draw
    # per double), so blocks of edges are generated independently by
    # advancing a copy of the stream — cache-sized blocks on a thread pool
    # instead of `scale` passes over e-sized temporaries.
    def block(lo, hi):
        src = np.zeros(hi - lo, dtype=np.uint64)
        dst = np.zeros(hi - lo, dtype=np.uint64)
        bg = np.random.PCG64()
        for level in range(scale):
            bg.state = base
            bg.advance(level * e + lo)
            r = np.random.Generator(bg).random(hi - lo)
            bit = np.uint64(1) << np.uint64(scale - 1 - level)
            # quadrant q = #thresholds < r: src bit for q>=2, dst for q in {1,3}
            upper = r > t1
            src += bit * upper
            dst += bit * (((r > t0) & ~upper) | (r > t2))
        src %= np.uint64(v)
        dst %= np.uint64(v)
        edges[lo:hi, 0] = src
        edges[lo:hi, 1] = dst

    _parallel_blocks(block, e, 1 << 18)
    if add_self_loops:
        edges[e:] = np.arange(v, dtype=np.uint32)[:, None]
    return edges


def degrees(edges: np.ndarray, v: int):
    """Out/in degrees of the edge list, clamped >=1 (graph.hpp:4397-4401)."""
    outd = np.bincount(edges[:, 0], minlength=v).astype(np.uint32)
    ind = np.bincount(edges[:, 1], minlength=v).astype(np.uint32)
    np.maximum(outd, 1, out=outd)
    np.maximum(ind, 1, out=ind)
    return outd, ind


def norm_weights(src: np.ndarray, dst: np.ndarray, outd: np.ndarray,
                 ind: np.ndarray) -> np.ndarray:
    """nts_norm_degree per edge (ntsBaseOp.hpp:194-197), fp32."""
    return (1.0 / (np.sqrt(outd[src].astype(np.float32)) *
                   np.sqrt(ind[dst].astype(np.float32)))).astype(np.float32)


def partition_offsets(edges: np.ndarray, v: int, parts: int,
                      alpha_hub: float = 8.0) -> np.ndarray:
    """Degree-balanced 1-D vertex ranges (graph.hpp:1186-1213): split [0,v)
    into `parts` contiguous ranges balancing out_degree + alpha per vertex."""
    if parts == 1:
        return np.array([0, v], dtype=np.uint32)
    outd = np.bincount(edges[:, 0], minlength=v).astype(np.float64)
    load = outd + alpha_hub
    csum = np.cumsum(load)
    total = csum[-1]
    offs = [0]
    for p in range(1, parts):
        target = total * p / parts
        offs.append(int(np.searchsorted(csum, target)))
    offs.append(v)
    # Hub-dominated graphs can make searchsorted return duplicate
    # boundaries; degrade to a valid (unbalanced) partition by nudging each
    # boundary past its predecessor instead of asserting.
    # Requires v >= parts (checked) so every range stays non-empty.
    assert v >= parts, f"{parts} partitions need >= {parts} vertices"
    for p in range(1, parts + 1):
        lo = offs[p - 1] + 1
        hi = v - (parts - p)
        offs[p] = min(max(offs[p], lo), hi)
    offs[parts] = v
    offs = np.array(offs, dtype=np.uint32)
    assert np.all(np.diff(offs.astype(np.int64)) > 0), "empty partition"
    return offs


@dataclass
class Chunk:
    """One per-source-partition graph chunk (CSC_segment_pinned equivalent,
    GraphSegment.h:52-139): forward CSC over the owned dst range, backward CSR
    over the chunk's src range, norm-degree weights on both orderings."""
    src_s: int          # source partition range [src_s, src_e)
    src_e: int
    dst_s: int          # owned destination range [dst_s, dst_e)
    dst_e: int
    column_offset: np.ndarray   # u32 [dst_n+1], local
    row_indices: np.ndarray     # u32 [E_k], global src ids
    edge_weight_forward: np.ndarray   # f32 [E_k], CSC order
    row_offset: np.ndarray      # u32 [src_n+1], local
    column_indices: np.ndarray  # u32 [E_k], global dst ids
    edge_weight_backward: np.ndarray  # f32 [E_k], CSR order

    @property
    def edge_size(self):
        return int(self.row_indices.size)

    @property
    def dst_n(self):
        return self.dst_e - self.dst_s

    @property
    def src_n(self):
        return self.src_e - self.src_s


def _csc(src, dst, w, dst_s, dst_n, key_minor=None):
    order = _stable_order(dst)
    s, wv = _take(src, order), _take(w, order)
    col_off = np.zeros(dst_n + 1, dtype=np.uint32)
    counts = np.bincount((dst - dst_s).astype(np.int64), minlength=dst_n)
    col_off[1:] = np.cumsum(counts).astype(np.uint32)
    return col_off, s, wv


def build_chunks(edges: np.ndarray, weights: np.ndarray, offs: np.ndarray,
                 rank: int) -> List[Chunk]:
    """Build rank `rank`'s chunks: for each source partition k, the chunk of
    edges (src in partition k, dst owned by `rank`), as CSC (forward) and CSR
    (backward) — PartitionedGraph::PartitionToChunks semantics
    (PartitionedGraph.hpp:324-420)."""
    parts = len(offs) - 1
    dst_s, dst_e = int(offs[rank]), int(offs[rank + 1])
    dst_n = dst_e - dst_s
    if parts == 1:
        e_src, e_dst, e_w = edges[:, 0], edges[:, 1], weights
    else:
        owned = (edges[:, 1] >= dst_s) & (edges[:, 1] < dst_e)
        e_src, e_dst, e_w = edges[owned, 0], edges[owned, 1], weights[owned]
    src_part = np.searchsorted(offs[1:-1], e_src, side="right") if parts > 1 \
        else np.zeros(len(e_src), dtype=np.int64)
    chunks = []
    for k in range(parts):
        if parts == 1:
            s, d, w = e_src, e_dst, e_w
        else:
            sel = src_part == k
            s, d, w = e_src[sel], e_dst[sel], e_w[sel]
        src_s, src_e = int(offs[k]), int(offs[k + 1])
        src_n = src_e - src_s
        col_off, rows, wf = _csc(s, d, w, dst_s, dst_n)
        # CSR built as a stable-by-src permutation OF THE CSC ORDER, so that
        # csr_edge[i] == csc_edge[argsort_stable(src_of_csc)[i]] — the
        # edge-valued (GAT) path relies on this to carry per-edge attention
        # weights from CSC to CSR order (gat.py csr_from_csc).
        d_csc = np.repeat(np.arange(dst_s, dst_e, dtype=np.uint32),
                          np.diff(col_off.astype(np.int64)))
        order = _stable_order(rows)
        row_off = np.zeros(src_n + 1, dtype=np.uint32)
        counts = np.bincount((rows - src_s).astype(np.int64), minlength=src_n)
        row_off[1:] = np.cumsum(counts).astype(np.uint32)
        chunks.append(Chunk(
            src_s=src_s, src_e=src_e, dst_s=dst_s, dst_e=dst_e,
            column_offset=col_off,
            row_indices=rows.astype(np.uint32, copy=False),
            edge_weight_forward=wf.astype(np.float32, copy=False),
            row_offset=row_off,
            column_indices=_take(d_csc, order, np.uint32),
            edge_weight_backward=_take(wf, order, np.float32),
        ))
    return chunks


def build_work_items(offset: np.ndarray, split: int = 512):
    """Decompose a CSC/CSR offset array into per-wavefront work items for the
    aggregation kernels: each item covers <= `split` consecutive edges of one
    vertex. Items of a vertex with a single item store directly; multi-item
    vertices accumulate with atomics (flag bit 31 of the vertex word).

    Returns (items_vertex u32, items_start u32, items_count u32) arrays.
    This host-side decomposition is the MI355X answer to the reference's
    power-law load imbalance (its fixed <<<128,512>>> kernels scan
    column_offset in-kernel, ntsCUDAFuseKernel.cuh:186-189)."""
    deg = np.diff(offset.astype(np.int64))
    n_items_per_v = np.maximum((deg + split - 1) // split, 0)
    total = int(n_items_per_v.sum())
    if total == 0:
        return (np.zeros(0, np.uint32),) * 3
    v_for_item = np.repeat(np.arange(len(deg), dtype=np.int64), n_items_per_v)
    item_seq = np.arange(total, dtype=np.int64) - np.repeat(
        np.concatenate([[0], np.cumsum(n_items_per_v)[:-1]]), n_items_per_v)
    starts = offset[:-1].astype(np.int64)[v_for_item] + item_seq * split
    ends = np.minimum(starts + split, offset[1:].astype(np.int64)[v_for_item])
    counts = (ends - starts).astype(np.uint32)
    flags = (n_items_per_v > 1)[v_for_item]
    vtx = v_for_item.astype(np.uint32) | (flags.astype(np.uint32) << 31)
    return vtx, starts.astype(np.uint32), counts
