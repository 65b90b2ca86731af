"""Single-GPU GAT layer over the edge-valued kernel path (BASELINE config #5).

Mirrors the decomposed op chain the reference runs for GAT
(/root/reference/toolkits/GAT_GPU_DIST.hpp:191-215 via the DistGPU*Op classes,
core/ntsDistGPUGraphOp.hpp:145-361), specialized to one partition (the
single-GPU case: every vertex is its own master, mirror_index = identity):

  per layer, with projected features H = X·W (torch, plumbing) and attention
  vectors a_src/a_dst:
    1. s_src[v] = H[v]·a_src, s_dst[v] = H[v]·a_dst          (torch mv)
    2. m_src = scatter_src_mirror_to_msg(s_src)   per-edge scalar  (E×1)
       m_dst = scatter_dst_to_msg(s_dst)                          (E×1)
    3. e = leaky_relu(m_src + m_dst)              (torch, elementwise)
    4. s = edge_softmax_forward(e)                per-dst, cached
    5. y = gather_by_dst_from_src(H, weight=s)    the SpMM hot kernel with
                                                  per-edge attention weights
  backward: edge_softmax_backward, scatter of grads to edges, CSR gather
  with the CSC->CSR-permuted attention weights, and the msg->vertex reducers.

The per-edge attention value is a SCALAR (f=1), matching the exercised
reference config: E×f edge tensors never materialize.

Multi-head attention (GATLayer(..., heads=K), K > 1): the f = K*C columns are
head-major (column c belongs to head c // C), attention scalars are [V, K],
and every per-edge value (softmax, leaky-relu input, gradients) is [E, K]
row-major.  Each head has its own softmax over a destination's in-edges and
its weight scales only that head's C columns; the index lists are read once
per pass and E×f messages still never materialize.  The chain is the one
above through the *_heads entries of include/nts_hip.h, except that the CSR
gather and the per-head edge dot run as two kernels (the fused gather-dot is
single-head).  `attend` wraps forward/backward as a torch.autograd.Function.

GATv2 (GATv2Layer, `attend_v2`): the score is att . leaky_relu(x_l[src] +
x_r[dst]) per head, one f-wide edge pass and two backward walks of their own
(nts_edge_gatv2_score, nts_edge_gatv2_backward); softmax, aggregation and the
gradient with respect to the softmax are the heads entries above.

Attention dropout (`dropout=p, seed=s` of both layers' forward, of `attend`
and `attend_v2`): the gathers weigh with w = keep ? alpha / (1 - p) : 0, the
keep mask a counter hash of (seed, CSC edge position, head) that the softmax's
normalize pass applies while it writes and the softmax backward regenerates
(nts_edge_attention_forward_drop, nts_edge_softmax_forward_drop,
nts_edge_softmax_backward_drop); no mask tensor, no extra launch.

Evaluation (GATLayer.infer, and `attend` under torch.no_grad() with
dropout == 0): one fused entry (nts_gat_forward_fused[_bf16]) reduces the
per-(destination, head) softmax denominators and aggregates with each edge's
weight recomputed in registers from the two scalars; it returns y alone and
allocates nothing of size E.  GATv2Layer has no such form (its score needs
the rows), and there is no dropout in infer.

bfloat16 feature rows: `h` of GATLayer and `x_l` / `x_r` of GATv2Layer may be
torch.bfloat16.  The f-wide passes then read 2-byte rows through the *_bf16
entries (widened exactly in registers); attention scalars, `att`, every
[E, K] value, `y`, `grad_y` and every gradient the layers return stay
float32, and `attend` / `attend_v2` cast the row gradients to the dtype of
the input they belong to.
"""
import numpy as np
import torch

from . import shim
from .graph import Chunk
from .ops import DeviceChunk, _u32_cuda


class _EdgeLayer:
    """What the attention layers on one chunk share: the constructor checks,
    the device chunk, the stream wrappers and the CSC <-> CSR slot maps."""

    def _setup(self, ch: Chunk, v: int, device, heads, stable):
        if not isinstance(heads, int) or heads < 1:
            raise ValueError(f"heads must be a positive int, got {heads!r}")
        if not isinstance(stable, bool):
            raise ValueError(f"stable must be a bool, got {stable!r}")
        self.heads = heads
        self.stable = stable
        self.v = v
        self.np_ch = ch
        self.ch = DeviceChunk(ch, device)
        self.stream = shim.Stream.wrap_torch_current()
        if stable:
            self.stream.edge_softmax_stable(1)
        self.mirror_index = _u32_cuda(np.arange(v, dtype=np.uint32), device)
        self.device = device
        self.E = ch.edge_size
        deg = np.diff(ch.column_offset.astype(np.int64))
        self._dst_of_edge_np = np.repeat(np.arange(ch.dst_n, dtype=np.int64), deg)
        self._src_of_edge_np = ch.row_indices.astype(np.int64) - ch.src_s
        # CSC -> CSR permutation: sort CSC edges by src (stable), which is
        # exactly the CSR construction order (graph.build_chunks builds CSR
        # as the stable-by-src permutation of the CSC order).
        perm = np.argsort(self._src_of_edge_np, kind="stable")
        self.csr_from_csc = torch.from_numpy(perm).to(device)
        self._perm_u32 = torch.from_numpy(
            perm.astype(np.uint32).view(np.int32)).to(device)
        # inverse map (CSC slot -> CSR slot) for the dual-order softmax
        # emission (kernels write out2[pos[e]] while walking CSC items)
        inv = np.empty_like(perm)
        inv[perm] = np.arange(len(perm))
        self._inv_perm_u32 = torch.from_numpy(
            inv.astype(np.uint32).view(np.int32)).to(device)
        self._doe = self._soe = None
        self._ones_dst = self._ones_src = None
        # separate wrapper of the same HIP stream for the scalar (f=1)
        # reductions, so bench roofline tags only see the main f-wide gathers
        self.scalar_stream = shim.Stream.wrap_torch_current()

    @property
    def dst_of_edge(self):
        if self._doe is None:
            self._doe = torch.from_numpy(self._dst_of_edge_np).to(self.device)
        return self._doe

    @property
    def src_of_edge(self):
        if self._soe is None:
            self._soe = torch.from_numpy(self._src_of_edge_np).to(self.device)
        return self._soe

    @staticmethod
    def _drop(dropout, seed):
        """(p, seed) of a forward with attention dropout, None at
        dropout == 0 (today's calls); an invalid pair raises ValueError
        before any launch."""
        shim.check_dropout(dropout, seed)
        return (float(dropout), seed) if dropout > 0 else None

    @staticmethod
    def _check_rows(name, t, rows, cols, bf16_ok=False):
        """The kernels take raw pointers: anything but a contiguous float32
        device matrix of the expected shape raises before a launch.
        bf16_ok: a feature-row operand, which may be bfloat16 instead."""
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name} must be a torch.Tensor")
        if bf16_ok and t.dtype == torch.bfloat16:
            pass
        elif t.dtype != torch.float32:
            raise TypeError(
                f"{name} must be float32{' or bfloat16' if bf16_ok else ''}, "
                f"got {t.dtype}")
        if not t.is_cuda:
            raise TypeError(f"{name} must be a device tensor")
        if tuple(t.shape) != (rows, cols):
            raise ValueError(
                f"{name} must have shape ({rows}, {cols}), got {tuple(t.shape)}")
        if not t.is_contiguous():
            raise ValueError(f"{name} must be contiguous")


class GATLayer(_EdgeLayer):
    """Attention-weighted aggregation on one chunk (whole graph on 1 GPU)."""

    def __init__(self, ch: Chunk, v: int, device, heads: int = 1,
                 stable: bool = False, _heads_path: bool = False):
        """heads = K attention heads over head-major column blocks.  With
        heads == 1 the layer makes exactly the single-head calls.
        stable=True runs the max-subtracted softmax (Stream.
        edge_softmax_stable) on the layer's own stream wrapper, single-head
        and heads path alike; the default is the reference's exp / sum exp,
        which is NaN once a logit passes about 88.  The backward is the same.
        _heads_path (private, for tools/bench_gat_heads.py) runs the heads
        call chain at heads == 1 too: unfused CSR gather + edge dot."""
        self._setup(ch, v, device, heads, stable)
        self._heads_path = heads > 1 or _heads_path

    def forward(self, h: torch.Tensor, s_src: torch.Tensor,
                s_dst: torch.Tensor, negative_slope: float = 0.2,
                dropout: float = 0.0, seed: int = 0):
        """h: [V,f] projected features; s_src/s_dst: [V] attention scalars
        ([V, heads] for a multi-head layer).

        h may be bfloat16 (s_src, s_dst, y and the backward's grad_y and
        results stay float32): the forward gather and the backward's edge dot
        then read bf16 rows.  A single-head layer given a bfloat16 h runs the
        heads call chain ([V] scalars are taken as [V, 1]): the fused
        gather-dot of the single-head backward is float32 only.

        dropout = p in [0, 1): attention dropout for training.  Each softmax
        coefficient alpha[e, k] is dropped with probability p (exactly
        round(p * 2^24) / 2^24) and the kept ones are scaled by 1 / (1 - p);
        the mask is a function of (seed, CSC edge position, head) alone
        (include/nts_hip.h, shim.edge_dropout_keep), regenerated in the
        backward and never stored.  The aggregation and the backward's CSR
        gather weigh with the dropped weights w, `saved` carries alpha (the
        softmax backward's cache), w in CSC and CSR order, p and seed, so the
        layer retains 4*E*K more bytes than without dropout.  A destination
        all of whose in-edges drop gets a zero row.  dropout == 0.0 (the
        default, and what evaluation passes: there is no train/eval flag)
        makes exactly the calls of a layer without the argument.  seed is an
        int in [0, 2**64); an invalid dropout or seed raises ValueError before
        any launch."""
        drop = self._drop(dropout, seed)
        # a single-head layer leaves the fused path for any h that is not
        # float32: the heads chain takes bfloat16 and rejects the rest
        if self._heads_path or (isinstance(h, torch.Tensor)
                                and h.dtype != torch.float32):
            return self._forward_heads(h, s_src, s_dst, negative_slope, drop)
        ch, st, E = self.ch, self.stream, self.E
        dev = h.device
        h = h.contiguous()
        # the layer owns its chunk for its lifetime -> item reuse is safe
        st.items_reuse(1)
        s = torch.empty(E, 1, device=dev)
        s_csr = torch.empty(E, 1, device=dev)
        m_sum = torch.empty(E, 1, device=dev)
        # ONE fused pass computes scatter_src + scatter_dst + leaky_relu +
        # exp + per-dst sums (5 E-sized passes of the decomposed chain);
        # the normalize pass dual-emits the softmax in CSC (s) and CSR
        # (s_csr) edge order.  cache = output (reference convention), so
        # `s` doubles as the backward's cached tensor.
        args = (s.data_ptr(), s_csr.data_ptr(), self._inv_perm_u32.data_ptr(),
                m_sum.data_ptr(), s_src.contiguous().data_ptr(),
                s_dst.contiguous().data_ptr(), ch.row_indices.data_ptr(),
                self.mirror_index.data_ptr(), negative_slope,
                ch.column_offset.data_ptr(), ch.dst_n)
        if drop:
            # the same two passes (one column, host-known edge count): the
            # normalize pass leaves the softmax in alpha, for the backward,
            # and dual-emits the dropped weights into s and s_csr
            alpha = torch.empty(E, 1, device=dev)
            st.edge_attention_forward_drop(*args, E, 1, alpha.data_ptr(),
                                           *drop)
            saved = {"h": h, "alpha": alpha, "w": s, "w_csr": s_csr,
                     "m_sum": m_sum, "p": drop[0], "seed": drop[1]}
        else:
            st.edge_attention_forward(*args)
            saved = {"h": h, "s": s, "s_csr": s_csr, "cached": s,
                     "m_sum": m_sum}
        y = torch.zeros(ch.dst_n, h.shape[1], device=dev)
        st.gather_by_dst_from_src(h.data_ptr(), y.data_ptr(), s.data_ptr(),
                                  ch.row_indices.data_ptr(),
                                  ch.column_offset.data_ptr(),
                                  ch.src_s, ch.src_e, ch.dst_s, ch.dst_e,
                                  E, ch.dst_n, h.shape[1], with_weight=True)
        return y, saved

    def backward(self, grad_y: torch.Tensor, saved,
                 negative_slope: float = 0.2):
        """Returns (grad_h from the aggregation, grad_s_src[V], grad_s_dst[V]);
        the two scalar gradients are [V, heads] for a multi-head layer."""
        if self._heads_path:
            return self._backward_heads(grad_y, saved, negative_slope)
        if saved["h"].dtype == torch.bfloat16:
            # the forward ran the heads chain: so does the backward, and the
            # scalar gradients come back [V] as from the fused path
            grad_h, g_src, g_dst = self._backward_heads(grad_y, saved,
                                                        negative_slope)
            return grad_h, g_src[:, 0], g_dst[:, 0]
        ch, st, E = self.ch, self.stream, self.E
        dev = grad_y.device
        f = grad_y.shape[1]
        grad_y = grad_y.contiguous()
        st.items_reuse(1)
        self.scalar_stream.items_reuse(1)
        # fused CSR gather + edge-dot: grad_h[src] accumulates while the
        # SAME grad_y row bytes produce gs[e] = grad_y[dst(e)].h[src(e)],
        # written straight into CSC slot order (dot_pos = csr->csc map) for
        # the softmax backward.  Replaces the separate k_edge_dot pass
        # (round-1: ~9 ms/step at f=128) and the s permute (dual-order
        # softmax output from forward).  rc=0 -> width not fused (ragged /
        # multi-slab f): the plain gather ran; do the dot separately.
        # after a forward with dropout the gather's weights are the dropped
        # ones (w_csr) and gs is the gradient with respect to them
        dropped = "p" in saved
        s_csr = saved["w_csr"] if dropped else saved["s_csr"]
        gs = torch.empty(E, 1, device=dev)
        grad_h = torch.zeros(ch.src_n, f, device=dev)
        rc = st.gather_by_src_from_dst_dot(
            grad_y.data_ptr(), grad_h.data_ptr(), s_csr.data_ptr(),
            ch.row_offset.data_ptr(), ch.column_indices.data_ptr(),
            ch.dst_s, ch.src_n, E, f, saved["h"].data_ptr(), gs.data_ptr(),
            self._perm_u32.data_ptr())
        if rc == 0:
            st.edge_dot(gs.data_ptr(), grad_y.data_ptr(),
                        saved["h"].data_ptr(), ch.row_indices.data_ptr(),
                        ch.column_offset.data_ptr(), ch.src_s, ch.dst_n, f)
        # softmax backward with the leaky-relu derivative fused in and the
        # result dual-emitted in CSC (ge) and CSR (ge_csr) edge order —
        # replaces the second permute and the torch elementwise mask pass
        ge = torch.empty(E, 1, device=dev)
        ge_csr = torch.empty(E, 1, device=dev)
        g_dst = torch.zeros(ch.dst_n, 1, device=dev)
        if dropped:
            st.edge_softmax_backward_drop(
                ge.data_ptr(), ge_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), gs.data_ptr(),
                saved["alpha"].data_ptr(), saved["m_sum"].data_ptr(),
                negative_slope, ch.column_offset.data_ptr(), ch.dst_n, E, 1,
                saved["p"], saved["seed"], dst_sum=g_dst.data_ptr())
        else:
            st.edge_softmax_backward_fused(
                ge.data_ptr(), ge_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), gs.data_ptr(),
                saved["cached"].data_ptr(),
                saved["m_sum"].contiguous().data_ptr(), negative_slope,
                ch.column_offset.data_ptr(), ch.dst_n, 1,
                dst_sum=g_dst.data_ptr())
        # edge-scalar -> vertex reductions through the load-balanced gather
        # kernel (per-edge values as WEIGHTS over an all-ones input): the
        # direct msg->vertex atomics serialize on power-law hub sources
        # (one address takes every hub edge's atomicAdd — measured 25 ms of
        # a 115 ms step), while the gather's work items split hubs and merge
        # a handful of partials.
        # g_dst came out of the softmax-backward pass itself (dst_sum);
        # g_src is the src-major sum of ge over the CSR — the dedicated
        # weight-sum kernel (full lane occupancy at f=1; the f-wide gather
        # left 15/16 lanes idle, and direct msg->vertex atomics serialize
        # on power-law hub sources — measured 25 ms of a 115 ms step in
        # round 1).  Item splitting keeps hubs bounded here too.
        sst = self.scalar_stream
        g_src = torch.zeros(ch.src_n, 1, device=dev)
        sst.weight_sum(g_src.data_ptr(), ge_csr.data_ptr(),
                       ch.row_offset.data_ptr(), ch.src_n)
        return grad_h, g_src[:, 0], g_dst[:, 0]

    # ---- multi-head path (heads = K > 1) ----
    def _width(self, name, t):
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError(f"{name} must be a 2-d tensor")
        f = int(t.shape[1])
        if f < self.heads or f % self.heads != 0:
            raise ValueError(
                f"{name} has {f} columns, not a multiple of heads={self.heads}")
        return f

    def _forward_heads(self, h, s_src, s_dst, negative_slope, drop=None):
        """h: [V, K*C]; s_src/s_dst: [V, K].  Returns (y[V, K*C], saved).
        drop: None or the (p, seed) of forward's dropout."""
        ch, st, E, K = self.ch, self.stream, self.E, self.heads
        f = self._width("h", h)
        self._check_rows("h", h, ch.src_n, f, bf16_ok=True)
        if not self._heads_path:
            # a single-head layer sent here by a bfloat16 h: [V] as [V, 1]
            s_src, s_dst = (t[:, None] if isinstance(t, torch.Tensor)
                            and t.dim() == 1 else t for t in (s_src, s_dst))
        self._check_rows("s_src", s_src, self.v, K)
        self._check_rows("s_dst", s_dst, ch.dst_n, K)
        bf16 = h.dtype == torch.bfloat16
        dev = h.device
        st.items_reuse(1)
        s = torch.empty(E, K, device=dev)
        s_csr = torch.empty(E, K, device=dev)
        m_sum = torch.empty(E, K, device=dev)
        args = (s.data_ptr(), s_csr.data_ptr(), self._inv_perm_u32.data_ptr(),
                m_sum.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(),
                ch.row_indices.data_ptr(), self.mirror_index.data_ptr(),
                negative_slope, ch.column_offset.data_ptr(), ch.dst_n, E, K)
        if drop:
            # s, s_csr: the dropped weights; alpha: the softmax, for backward
            alpha = torch.empty(E, K, device=dev)
            st.edge_attention_forward_drop(*args, alpha.data_ptr(), *drop)
            saved = {"h": h, "alpha": alpha, "w": s, "w_csr": s_csr,
                     "m_sum": m_sum, "p": drop[0], "seed": drop[1]}
        else:
            st.edge_attention_forward_heads(*args)
            saved = {"h": h, "s": s, "s_csr": s_csr, "cached": s,
                     "m_sum": m_sum}
        y = torch.zeros(ch.dst_n, f, device=dev)
        (st.gather_by_dst_from_src_heads_bf16 if bf16
         else st.gather_by_dst_from_src_heads)(
            h.data_ptr(), y.data_ptr(), s.data_ptr(),
            ch.row_indices.data_ptr(), ch.column_offset.data_ptr(),
            ch.src_s, ch.src_e, ch.dst_s, ch.dst_e, E, ch.dst_n, f, K)
        return y, saved

    def infer(self, h: torch.Tensor, s_src: torch.Tensor,
              s_dst: torch.Tensor, negative_slope: float = 0.2):
        """The forward for evaluation: y of forward(h, s_src, s_dst) and
        nothing else.  One fused entry (Stream.gat_forward_fused) reduces the
        per-(destination, head) softmax denominators and then aggregates with
        each edge's weight computed in registers, so no [E, K] tensor is
        allocated, written or kept; there is no `saved` and no backward.

        h: [V, K*C] float32 or bfloat16; s_src, s_dst: [V, K] float32 ([V] is
        taken as [V, 1] on a single-head layer); y is float32.  Any heads and
        either softmax mode of the layer; no dropout.  Inputs are checked as
        for the heads forward and a bad one raises before any launch.  On a
        destination of at most one work item y is bit-identical to forward's;
        a split destination differs by the order of its fp32 atomics."""
        ch, st, E, K = self.ch, self.stream, self.E, self.heads
        f = self._width("h", h)
        self._check_rows("h", h, ch.src_n, f, bf16_ok=True)
        if K == 1:
            s_src, s_dst = (t[:, None] if isinstance(t, torch.Tensor)
                            and t.dim() == 1 else t for t in (s_src, s_dst))
        self._check_rows("s_src", s_src, self.v, K)
        self._check_rows("s_dst", s_dst, ch.dst_n, K)
        st.items_reuse(1)
        y = torch.zeros(ch.dst_n, f, device=h.device)
        # mirror_index None: the layer's is the identity
        (st.gat_forward_fused_bf16 if h.dtype == torch.bfloat16
         else st.gat_forward_fused)(
            h.data_ptr(), y.data_ptr(), s_src.data_ptr(), s_dst.data_ptr(),
            ch.row_indices.data_ptr(), None, negative_slope,
            ch.column_offset.data_ptr(), ch.src_s, ch.src_e, ch.dst_s,
            ch.dst_e, E, ch.dst_n, f, K)
        return y

    def _backward_heads(self, grad_y, saved, negative_slope):
        """Returns (grad_h[V, K*C], g_src[V, K], g_dst[V, K])."""
        ch, st, E, K = self.ch, self.stream, self.E, self.heads
        f = self._width("grad_y", grad_y)
        self._check_rows("grad_y", grad_y, ch.dst_n, f)
        if tuple(saved["h"].shape) != (ch.src_n, f):
            raise ValueError("grad_y does not match the saved forward input")
        dev = grad_y.device
        st.items_reuse(1)
        self.scalar_stream.items_reuse(1)
        # the fused gather-dot is single-head: the CSR gather (weights in CSR
        # order from the forward's dual emission) and the per-head dot
        # gs[e, k] = grad_y[dst(e), head k] . h[src(e), head k] run apart
        dropped = "p" in saved   # then the weights are w and gs is dL/dw
        s_csr = saved["w_csr"] if dropped else saved["s_csr"]
        grad_h = torch.zeros(ch.src_n, f, device=dev)
        st.gather_by_src_from_dst_heads(
            grad_y.data_ptr(), grad_h.data_ptr(), s_csr.data_ptr(),
            ch.row_offset.data_ptr(), ch.column_indices.data_ptr(),
            ch.src_s, ch.src_e, ch.dst_s, ch.dst_e, E, ch.src_n, f, K)
        gs = torch.empty(E, K, device=dev)
        bf16 = saved["h"].dtype == torch.bfloat16
        (st.edge_dot_heads_bf16 if bf16 else st.edge_dot_heads)(
            gs.data_ptr(), grad_y.data_ptr(), saved["h"].data_ptr(),
            ch.row_indices.data_ptr(), ch.column_offset.data_ptr(), ch.src_s,
            ch.dst_n, E, f, K)
        ge = torch.empty(E, K, device=dev)
        ge_csr = torch.empty(E, K, device=dev)
        if dropped:
            st.edge_softmax_backward_drop(
                ge.data_ptr(), ge_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), gs.data_ptr(),
                saved["alpha"].data_ptr(), saved["m_sum"].data_ptr(),
                negative_slope, ch.column_offset.data_ptr(), ch.dst_n, E, K,
                saved["p"], saved["seed"], dst_sum=None)
        else:
            st.edge_softmax_backward_fused(
                ge.data_ptr(), ge_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), gs.data_ptr(),
                saved["cached"].data_ptr(), saved["m_sum"].data_ptr(),
                negative_slope, ch.column_offset.data_ptr(), ch.dst_n, K,
                dst_sum=None)
        # per-(vertex, head) sums of the edge gradient: by source over the
        # CSR order, by destination over the CSC order (the softmax
        # backward's own dst_sum emission is single-column)
        sst = self.scalar_stream
        g_src = torch.zeros(ch.src_n, K, device=dev)
        sst.weight_sum_heads(g_src.data_ptr(), ge_csr.data_ptr(),
                             ch.row_offset.data_ptr(), ch.src_n, E, K)
        g_dst = torch.zeros(ch.dst_n, K, device=dev)
        sst.weight_sum_heads(g_dst.data_ptr(), ge.data_ptr(),
                             ch.column_offset.data_ptr(), ch.dst_n, E, K)
        return grad_h, g_src, g_dst


class _AttendFn(torch.autograd.Function):
    """torch.autograd bridge over GATLayer.forward/backward (the GAT twin of
    ops._AggregateFn): gradients flow to h, s_src and s_dst."""

    @staticmethod
    def forward(ctx, h, s_src, s_dst, layer, negative_slope, dropout=0.0,
                seed=0):
        y, saved = layer.forward(h.detach().contiguous(),
                                 s_src.detach().contiguous(),
                                 s_dst.detach().contiguous(), negative_slope,
                                 dropout, seed)
        ctx.layer, ctx.saved, ctx.slope = layer, saved, negative_slope
        ctx.scalar_shapes = (s_src.shape, s_dst.shape)
        return y

    @staticmethod
    def backward(ctx, grad_y):
        grad_h, g_src, g_dst = ctx.layer.backward(grad_y.contiguous(),
                                                  ctx.saved, ctx.slope)
        # fp32 out of the kernels; bf16 only if h itself was
        grad_h = grad_h.to(ctx.saved["h"].dtype)
        return (grad_h, g_src.reshape(ctx.scalar_shapes[0]),
                g_dst.reshape(ctx.scalar_shapes[1]), None, None, None, None)


def _draw_seed(dropout, seed):
    """The seed of an attend call: the caller's, or for seed=None a draw from
    torch's default CPU generator (reproducible under torch.manual_seed, no
    device synchronize).  Checked here, so nothing is drawn or launched for
    an invalid pair."""
    shim.check_dropout(dropout, 0 if seed is None else seed)
    if seed is not None:
        return seed
    if dropout == 0:   # nothing to mask: the generator is left alone
        return 0
    return int(torch.randint(0, 2**63 - 1, (1,), dtype=torch.int64))


def attend(h: torch.Tensor, s_src: torch.Tensor, s_dst: torch.Tensor,
           layer: GATLayer, negative_slope: float = 0.2,
           dropout: float = 0.0, seed=None) -> torch.Tensor:
    """Autograd-aware attention-weighted aggregation on `layer`'s graph:
    y = layer.forward(h, s_src, s_dst), differentiable in all three.  The
    projections stay in torch, e.g. for K heads of C columns
    s_src = (h.view(V, K, C) * a_src).sum(-1) with a_src of shape [K, C].
    h may be bfloat16 (GATLayer.forward); h.grad then is bfloat16, the float32
    gradient of the kernels rounded once, and s_src / s_dst stay float32.
    dropout, seed: attention dropout as for GATLayer.forward (pass 0.0 for
    evaluation); seed=None draws one from torch's default CPU generator.
    Under torch.no_grad() with dropout == 0 (evaluation) the call is
    layer.infer: the same y, with no [E, K] tensor allocated or kept."""
    if not torch.is_grad_enabled() and dropout == 0:
        _draw_seed(dropout, seed)   # the same argument checks
        return layer.infer(h.contiguous(), s_src.contiguous(),
                           s_dst.contiguous(), negative_slope)
    return _AttendFn.apply(h, s_src, s_dst, layer, negative_slope, dropout,
                           _draw_seed(dropout, seed))


class GATv2Layer(_EdgeLayer):
    """GATv2 attention (Brody et al., "How Attentive are Graph Attention
    Networks?") on one chunk: the non-linearity sits before the dot with the
    attention vector,

      score[e, k] = att[k] . leaky_relu(x_l[src(e), head k] + x_r[dst(e), head k])
      alpha       = softmax of score over dst(e)'s in-edges, per head
      y[d, c]     = sum_{e into d} alpha[e, c // C] * x_l[src(e), c]

    so the score is no sum of two per-vertex scalars and runs as one f-wide
    edge pass (nts_edge_gatv2_score); its backward is one walk over the CSC
    and one over the CSR (nts_edge_gatv2_backward).  Softmax, aggregation
    and the gradient with respect to alpha are the entries GATLayer's heads
    path uses.  The [E, f] tensor x_l[src] + x_r[dst] never materializes."""

    def __init__(self, ch: Chunk, v: int, device, heads: int = 1,
                 stable: bool = False):
        """heads = K heads over head-major column blocks (heads == 1: C = f);
        stable=True runs the max-subtracted softmax, as for GATLayer."""
        self._setup(ch, v, device, heads, stable)

    def _check_inputs(self, x_l, x_r, att):
        ch, K = self.ch, self.heads
        if not isinstance(x_l, torch.Tensor) or x_l.dim() != 2:
            raise ValueError("x_l must be a 2-d tensor")
        f = int(x_l.shape[1])
        if f < K or f % K != 0:
            raise ValueError(
                f"x_l has {f} columns, not a multiple of heads={K}")
        self._check_rows("x_l", x_l, ch.src_n, f, bf16_ok=True)
        self._check_rows("x_r", x_r, ch.dst_n, f, bf16_ok=True)
        if x_l.dtype != x_r.dtype:
            raise TypeError(
                f"x_l and x_r must have one dtype, got {x_l.dtype} and "
                f"{x_r.dtype}")
        self._check_rows("att", att, K, f // K)
        return f

    def forward(self, x_l: torch.Tensor, x_r: torch.Tensor, att: torch.Tensor,
                negative_slope: float = 0.2, dropout: float = 0.0,
                seed: int = 0):
        """x_l: [src_n, K*C], x_r: [dst_n, K*C], att: [K, C].  Returns
        (y[dst_n, K*C], saved).  x_l and x_r may both be bfloat16 (att, y,
        grad_y and the backward's results stay float32): the score, the
        gather, the edge dot and both backward walks then read bf16 rows.
        dropout, seed: attention dropout exactly as
        for GATLayer.forward — `saved` then carries alpha (the cache), w and
        w_csr (the dropped gather weights), p and seed, 4*E*K more bytes
        than without; dropout == 0.0 makes today's calls."""
        drop = self._drop(dropout, seed)
        ch, st, E, K = self.ch, self.stream, self.E, self.heads
        f = self._check_inputs(x_l, x_r, att)
        dev = x_l.device
        bf16 = x_l.dtype == torch.bfloat16
        st.items_reuse(1)
        score = torch.empty(E, K, device=dev)
        (st.edge_gatv2_score_bf16 if bf16 else st.edge_gatv2_score)(
            score.data_ptr(), x_r.data_ptr(), x_l.data_ptr(), att.data_ptr(),
            negative_slope, ch.row_indices.data_ptr(),
            ch.column_offset.data_ptr(), ch.src_s, ch.dst_n, E, f, K)
        # per-(destination, head) softmax, dual-emitted in CSC (alpha) and
        # CSR (alpha_csr) edge order; cache = output
        alpha = torch.empty(E, K, device=dev)
        saved = {"x_l": x_l, "x_r": x_r, "att": att, "alpha": alpha}
        if drop:
            # alpha stays the softmax; w, w_csr are the dropped weights
            w = torch.empty(E, K, device=dev)
            w_csr = torch.empty(E, K, device=dev)
            st.edge_softmax_forward_drop(
                w.data_ptr(), w_csr.data_ptr(), self._inv_perm_u32.data_ptr(),
                score.data_ptr(), alpha.data_ptr(),
                ch.column_offset.data_ptr(), ch.dst_n, E, K, *drop)
            saved.update(w=w, w_csr=w_csr, p=drop[0], seed=drop[1])
        else:
            w = alpha
            alpha_csr = torch.empty(E, K, device=dev)
            st.edge_softmax_forward_dual(
                alpha.data_ptr(), alpha_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), score.data_ptr(),
                alpha.data_ptr(), ch.column_offset.data_ptr(), ch.dst_n, K)
            saved["alpha_csr"] = alpha_csr
        y = torch.zeros(ch.dst_n, f, device=dev)
        (st.gather_by_dst_from_src_heads_bf16 if bf16
         else st.gather_by_dst_from_src_heads)(
            x_l.data_ptr(), y.data_ptr(), w.data_ptr(),
            ch.row_indices.data_ptr(), ch.column_offset.data_ptr(),
            ch.src_s, ch.src_e, ch.dst_s, ch.dst_e, E, ch.dst_n, f, K)
        return y, saved

    def backward(self, grad_y: torch.Tensor, saved,
                 negative_slope: float = 0.2):
        """Returns (grad_x_l[src_n, K*C], grad_x_r[dst_n, K*C],
        grad_att[K, C])."""
        ch, st, E, K = self.ch, self.stream, self.E, self.heads
        x_l, x_r, att = saved["x_l"], saved["x_r"], saved["att"]
        f = int(x_l.shape[1])
        if not isinstance(grad_y, torch.Tensor) or grad_y.dim() != 2 \
                or int(grad_y.shape[1]) != f:
            raise ValueError("grad_y does not match the saved forward input")
        self._check_rows("grad_y", grad_y, ch.dst_n, f)
        dev = grad_y.device
        bf16 = x_l.dtype == torch.bfloat16
        walk = st.edge_gatv2_backward_bf16 if bf16 else st.edge_gatv2_backward
        st.items_reuse(1)
        # through alpha: the aggregation's own gradient to x_l, and the
        # per-head dot that is the gradient with respect to alpha
        dropped = "p" in saved   # then the weights are w and galpha is dL/dw
        w_csr = saved["w_csr"] if dropped else saved["alpha_csr"]
        grad_xl = torch.zeros(ch.src_n, f, device=dev)
        st.gather_by_src_from_dst_heads(
            grad_y.data_ptr(), grad_xl.data_ptr(),
            w_csr.data_ptr(), ch.row_offset.data_ptr(),
            ch.column_indices.data_ptr(), ch.src_s, ch.src_e, ch.dst_s,
            ch.dst_e, E, ch.src_n, f, K)
        galpha = torch.empty(E, K, device=dev)
        (st.edge_dot_heads_bf16 if bf16 else st.edge_dot_heads)(
            galpha.data_ptr(), grad_y.data_ptr(), x_l.data_ptr(),
            ch.row_indices.data_ptr(), ch.column_offset.data_ptr(), ch.src_s,
            ch.dst_n, E, f, K)
        # softmax backward without a leaky-relu mask (the GATv2 mask is
        # per column, inside the two walks below), dual-emitted
        gscore = torch.empty(E, K, device=dev)
        gscore_csr = torch.empty(E, K, device=dev)
        if dropped:
            st.edge_softmax_backward_drop(
                gscore.data_ptr(), gscore_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), galpha.data_ptr(),
                saved["alpha"].data_ptr(), None, negative_slope,
                ch.column_offset.data_ptr(), ch.dst_n, E, K, saved["p"],
                saved["seed"], dst_sum=None)
        else:
            st.edge_softmax_backward_fused(
                gscore.data_ptr(), gscore_csr.data_ptr(),
                self._inv_perm_u32.data_ptr(), galpha.data_ptr(),
                saved["alpha"].data_ptr(), None, negative_slope,
                ch.column_offset.data_ptr(), ch.dst_n, K, dst_sum=None)
        # CSC walk: own = x_r, nbr = x_l -> grad_x_r and grad_att
        grad_xr = torch.zeros(ch.dst_n, f, device=dev)
        grad_att = torch.zeros(K, f // K, device=dev)
        walk(
            grad_xr.data_ptr(), grad_att.data_ptr(), gscore.data_ptr(),
            x_r.data_ptr(), x_l.data_ptr(), att.data_ptr(), negative_slope,
            ch.column_offset.data_ptr(), ch.row_indices.data_ptr(), ch.src_s,
            ch.dst_n, E, f, K)
        # CSR walk: own = x_l, nbr = x_r, accumulated into grad_x_l
        walk(
            grad_xl.data_ptr(), None, gscore_csr.data_ptr(), x_l.data_ptr(),
            x_r.data_ptr(), att.data_ptr(), negative_slope,
            ch.row_offset.data_ptr(), ch.column_indices.data_ptr(), ch.dst_s,
            ch.src_n, E, f, K)
        return grad_xl, grad_xr, grad_att


class _AttendV2Fn(torch.autograd.Function):
    """torch.autograd bridge over GATv2Layer.forward/backward."""

    @staticmethod
    def forward(ctx, x_l, x_r, att, layer, negative_slope, dropout=0.0,
                seed=0):
        y, saved = layer.forward(x_l.detach(), x_r.detach(), att.detach(),
                                 negative_slope, dropout, seed)
        ctx.layer, ctx.saved, ctx.slope = layer, saved, negative_slope
        return y

    @staticmethod
    def backward(ctx, grad_y):
        grad_xl, grad_xr, grad_att = ctx.layer.backward(
            grad_y.contiguous(), ctx.saved, ctx.slope)
        # fp32 out of the kernels; bf16 only if the rows themselves were
        dt = ctx.saved["x_l"].dtype
        return (grad_xl.to(dt), grad_xr.to(dt), grad_att, None, None, None,
                None)


def attend_v2(x_l: torch.Tensor, x_r: torch.Tensor, att: torch.Tensor,
              layer: GATv2Layer, negative_slope: float = 0.2,
              dropout: float = 0.0, seed=None) -> torch.Tensor:
    """Autograd-aware GATv2 aggregation on `layer`'s graph, differentiable in
    x_l [src_n, K*C], x_r [dst_n, K*C] and att [K, C] (att float32, x_l and
    x_r both float32 or both bfloat16, their gradients in their own dtype;
    contiguous, on the device; anything else raises before a launch).  The
    projections stay in torch: x_l = x @ W_l, x_r = x @ W_r.  Weight sharing
    (x_l is x_r) needs no special case: autograd adds the two gradients.
    dropout, seed: attention dropout as for `attend`."""
    return _AttendV2Fn.apply(x_l, x_r, att, layer, negative_slope, dropout,
                             _draw_seed(dropout, seed))
