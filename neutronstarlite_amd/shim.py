"""ctypes binding of the C-ABI in include/nts_hip.h (the product compute path).

FAILS LOUDLY if the HIP extension is missing: there is no CPU fallback in the
product path — the oracle under oracle/ is test infrastructure only.
"""
import atexit
import ctypes
import os
import weakref

_DIR = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_DIR, "libnts_hip.so")

# kernel-time tags (enum nts_ktag in include/nts_hip.h)
KTAG_FWD = 0
KTAG_BWD = 1
KTAG_DESER = 2
KTAG_AGGMSG = 3
KTAG_ITEMS = 4
KTAG_EDGE = 5

_c = ctypes
_vp = _c.c_void_p
_u32 = _c.c_uint32
_i32 = _c.c_int
_i64 = _c.c_long


class NtsHipMissing(RuntimeError):
    pass


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_SO):
        raise NtsHipMissing(
            f"HIP extension not built: {_SO} missing. Run "
            "`python -m neutronstarlite_amd.build` (or __graft_entry__.build()). "
            "The product path has no CPU fallback.")
    l = ctypes.CDLL(_SO)
    # streams / timing
    l.nts_stream_create.restype = _vp
    l.nts_stream_wrap.restype = _vp
    l.nts_stream_wrap.argtypes = [_vp]
    l.nts_stream_destroy.argtypes = [_vp]
    l.nts_stream_sync.argtypes = [_vp]
    l.nts_stream_handle.restype = _vp
    l.nts_stream_handle.argtypes = [_vp]
    l.nts_stream_timing.argtypes = [_vp, _i32]
    l.nts_stream_timing_reset.argtypes = [_vp]
    l.nts_stream_kernel_ns.restype = _c.c_double
    l.nts_stream_kernel_ns.argtypes = [_vp, _i32]
    l.nts_stream_kernel_launches.restype = _c.c_longlong
    l.nts_stream_kernel_launches.argtypes = [_vp, _i32]
    # memory
    l.nts_malloc_gpu.restype = _vp
    l.nts_malloc_gpu.argtypes = [_i64]
    l.nts_malloc_pinned.restype = _vp
    l.nts_malloc_pinned.argtypes = [_i64]
    l.nts_get_device_pointer.restype = _vp
    l.nts_get_device_pointer.argtypes = [_vp]
    l.nts_free_gpu.argtypes = [_vp]
    l.nts_free_host.argtypes = [_vp]
    l.nts_zero_buffer.argtypes = [_vp, _vp, _i64]
    l.nts_memcpy_h2d.argtypes = [_vp, _vp, _vp, _i64, _i32]
    l.nts_memcpy_d2h.argtypes = [_vp, _vp, _vp, _i64, _i32]
    # hot kernels
    l.nts_gather_by_dst_from_src.argtypes = [_vp] + [_vp] * 5 + [_u32] * 7 + [_i32]
    l.nts_gather_by_src_from_dst.argtypes = [_vp] + [_vp] * 5 + [_u32] * 7 + [_i32]
    l.nts_gather_by_dst_from_src_bf16.argtypes = (
        l.nts_gather_by_dst_from_src.argtypes)
    l.nts_gather_by_src_from_dst_bf16.argtypes = (
        l.nts_gather_by_src_from_dst.argtypes)
    l.nts_items_cache_clear.argtypes = [_vp]
    l.nts_gather_schedule.argtypes = [_vp, _i32, _i32]
    l.nts_gather_schedule_last.argtypes = [_vp, _vp, _vp]
    l.nts_gather_plan.argtypes = [_u32] * 5 + [_i32] * 2 + [_vp] * 6
    l.nts_gather_plan_bf16.argtypes = l.nts_gather_plan.argtypes
    l.nts_gather_staging.argtypes = [_vp, _i32]
    l.nts_gather_staging_last.argtypes = [_vp, _vp, _vp]
    l.nts_gather_stage_plan.argtypes = [_u32] * 7 + [_i32] * 3 + [_vp] * 9
    l.nts_gather_stripes.argtypes = [_vp, _i32]
    l.nts_gather_stripes_run.argtypes = [_vp, _i32]
    l.nts_gather_stripes_last.argtypes = [_vp, _vp, _vp]
    l.nts_gather_stripe_plan.argtypes = [_u32] * 7 + [_i32] * 5 + [_vp] * 14
    l.nts_gather_stripe_task.argtypes = (
        [_u32] * 7 + [_i32] * 5 + [_u32] + [_c.c_ulonglong] * 2 + [_vp] * 3)
    l.nts_gather_stripe_task.restype = _c.c_longlong
    l.nts_deserialize_to_gpu.argtypes = [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _i32]
    l.nts_aggregate_comm_result.argtypes = [_vp, _vp, _vp, _u32, _u32, _u32, _u32, _i32]
    l.nts_gather_rows.argtypes = [_vp, _vp, _vp, _vp, _u32, _u32, _u32]
    l.nts_scatter_rows.argtypes = [_vp, _vp, _vp, _vp, _u32, _u32, _u32]
    l.nts_scatter_add_rows.argtypes = [_vp, _vp, _vp, _vp, _u32, _u32, _u32]
    # edge kernels
    l.nts_scatter_src_mirror_to_msg.argtypes = [_vp] + [_vp] * 5 + [_u32] * 2
    l.nts_gather_msg_to_src_mirror.argtypes = [_vp] + [_vp] * 5 + [_u32] * 2
    l.nts_scatter_dst_to_msg.argtypes = [_vp] + [_vp] * 4 + [_u32] * 2
    l.nts_gather_msg_to_dst.argtypes = [_vp] + [_vp] * 4 + [_u32] * 2
    l.nts_scatter_grad_back_to_message.argtypes = [_vp] + [_vp] * 4 + [_u32] * 2
    l.nts_edge_dot.argtypes = [_vp] + [_vp] * 5 + [_u32] * 3
    l.nts_edge_softmax_forward.argtypes = [_vp] + [_vp] * 5 + [_u32] * 2
    l.nts_edge_softmax_backward.argtypes = [_vp] + [_vp] * 5 + [_u32] * 2
    l.nts_edge_softmax_forward_dual.argtypes = [_vp] + [_vp] * 6 + [_u32] * 2
    l.nts_edge_softmax_backward_fused.argtypes = (
        [_vp] + [_vp] * 6 + [_c.c_float] + [_vp] * 2 + [_u32] * 2)
    l.nts_gather_by_src_from_dst_dot.argtypes = (
        [_vp] + [_vp] * 5 + [_u32] * 4 + [_vp] * 3)
    l.nts_gather_by_src_from_dst_dot.restype = _i32
    l.nts_edge_attention_forward.argtypes = (
        [_vp] + [_vp] * 8 + [_c.c_float] + [_vp] + [_u32])
    # per-head edge weights (multi-head GAT)
    l.nts_gather_by_dst_from_src_heads.argtypes = (
        [_vp] + [_vp] * 5 + [_u32] * 8)
    l.nts_gather_by_src_from_dst_heads.argtypes = (
        l.nts_gather_by_dst_from_src_heads.argtypes)
    l.nts_gather_plan_heads.argtypes = [_u32] * 5 + [_vp] * 3
    l.nts_edge_attention_forward_heads.argtypes = (
        [_vp] + [_vp] * 8 + [_c.c_float] + [_vp] + [_u32] * 3)
    l.nts_edge_dot_heads.argtypes = [_vp] + [_vp] * 5 + [_u32] * 5
    l.nts_weight_sum_heads.argtypes = [_vp] + [_vp] * 3 + [_u32] * 3
    l.nts_heads_dbg_general.argtypes = [_vp, _i32]
    # GATv2 score and backward
    l.nts_edge_gatv2_score.argtypes = (
        [_vp] + [_vp] * 4 + [_c.c_float] + [_vp] * 2 + [_u32] * 5)
    l.nts_edge_gatv2_backward.argtypes = (
        [_vp] + [_vp] * 6 + [_c.c_float] + [_vp] * 2 + [_u32] * 5)
    # bf16 feature rows of the attention passes
    l.nts_gather_by_dst_from_src_heads_bf16.argtypes = (
        l.nts_gather_by_dst_from_src_heads.argtypes)
    l.nts_gather_by_src_from_dst_heads_bf16.argtypes = (
        l.nts_gather_by_dst_from_src_heads.argtypes)
    l.nts_gather_plan_heads_bf16.argtypes = l.nts_gather_plan_heads.argtypes
    l.nts_edge_dot_heads_bf16.argtypes = l.nts_edge_dot_heads.argtypes
    l.nts_edge_gatv2_score_bf16.argtypes = l.nts_edge_gatv2_score.argtypes
    l.nts_edge_gatv2_backward_bf16.argtypes = (
        l.nts_edge_gatv2_backward.argtypes)
    # fused inference forward (no per-edge state)
    l.nts_gat_forward_fused.argtypes = (
        [_vp] + [_vp] * 6 + [_c.c_float] + [_vp] + [_u32] * 8)
    l.nts_gat_forward_fused_bf16.argtypes = l.nts_gat_forward_fused.argtypes
    l.nts_edge_softmax_stable.argtypes = [_vp, _i32]
    l.nts_edge_softmax_stable_last.argtypes = [_vp, _vp]
    # attention dropout
    l.nts_edge_dropout_keep.argtypes = (
        [_c.c_ulonglong, _c.c_float] + [_c.c_ulonglong] * 2 + [_vp])
    l.nts_edge_attention_forward_drop.argtypes = (
        l.nts_edge_attention_forward_heads.argtypes
        + [_vp, _c.c_float, _c.c_ulonglong])
    l.nts_edge_softmax_forward_drop.argtypes = (
        [_vp] + [_vp] * 6 + [_u32] * 3 + [_c.c_float, _c.c_ulonglong])
    l.nts_edge_softmax_backward_drop.argtypes = (
        [_vp] + [_vp] * 6 + [_c.c_float] + [_vp] * 2 + [_u32] * 3
        + [_c.c_float, _c.c_ulonglong])
    # max / min aggregation
    l.nts_reduce_by_dst_from_src.argtypes = (
        [_vp, _i32] + [_vp] * 5 + [_u32] * 7)
    l.nts_reduce_backward.argtypes = [_vp] + [_vp] * 3 + [_u32, _vp] + [_u32] * 2
    l.nts_reduce_plan.argtypes = [_u32] * 4 + [_vp] * 4
    l.nts_items_reuse.argtypes = [_vp, _i32]
    l.nts_weight_sum.argtypes = [_vp, _vp, _vp, _vp, _u32]
    l.nts_permute_f32.argtypes = [_vp, _vp, _vp, _vp, _i64]
    l.nts_sample_reservoir.argtypes = [_vp, _vp, _vp, _vp, _u32, _u32,
                                       _c.c_ulonglong, _vp, _vp]
    l.nts_sample_reservoir_dbg_fallback.argtypes = l.nts_sample_reservoir.argtypes
    l.nts_device_count.restype = _i32
    l.nts_set_device.argtypes = [_i32]
    l.nts_build_arch.restype = _c.c_char_p
    _lib = l
    return l


def _plan(entry, f, alignment, rows, batch, edges, schedule, window):
    names = ("schedule", "window", "lane_group", "vector_width", "grid",
             "blocked")
    out = [_i32(0) for _ in names]
    entry(f, alignment, rows, batch, edges, schedule, window,
          *[_c.byref(o) for o in out])
    plan = {n: o.value for n, o in zip(names, out)}
    plan["blocked"] = bool(plan["blocked"])
    return plan


def gather_plan(f, alignment, rows, batch, edges, schedule=0, window=0):
    """The launch decision a gather of this shape would take (no device
    access): dict of schedule, window, lane_group, vector_width, grid,
    blocked.  (schedule, window) is a request as for Stream.gather_schedule."""
    return _plan(lib().nts_gather_plan, f, alignment, rows, batch, edges,
                 schedule, window)


def gather_plan_bf16(f, alignment, rows, batch, edges, schedule=0, window=0):
    """gather_plan for bfloat16 feature rows: vector_width is in elements per
    lane (8, 4, 2 or 1), window in columns."""
    return _plan(lib().nts_gather_plan_bf16, f, alignment, rows, batch, edges,
                 schedule, window)


def gather_stage_plan(f, in_alignment, out_alignment, rows, batch, edges,
                      schedule=0, window=0, stage=0, elem_bytes=4):
    """gather_plan with the row-staging decision (no device access): the
    gather_plan dict of the launch that runs plus staged, pitch (row pitch
    the gather reads, in elements) and store_width (floats per access of the
    output).  stage is a request as for Stream.gather_staging."""
    names = ("staged", "pitch", "schedule", "window", "lane_group",
             "vector_width", "store_width", "grid", "blocked")
    out = [_i32(0) for _ in names]
    lib().nts_gather_stage_plan(f, elem_bytes, in_alignment, out_alignment,
                                rows, batch, edges, schedule, window, stage,
                                *[_c.byref(o) for o in out])
    plan = {n: o.value for n, o in zip(names, out)}
    plan["staged"] = bool(plan["staged"])
    plan["blocked"] = bool(plan["blocked"])
    return plan


def gather_stripe_plan(f, in_alignment, out_alignment, rows, batch, edges,
                       schedule=0, window=0, stage=0, stripe=0, run=0,
                       elem_bytes=4):
    """gather_stage_plan with the stripe decision (no device access): the
    gather_stage_plan dict of the launch that really runs plus stripe (width
    in floats, 0 = no stripes), stripe_lanes, subgroups (per wave), stripes
    (per window) and tasks_per_wave.  stripe / run are requests as for
    Stream.gather_stripes."""
    names = ("staged", "pitch", "schedule", "window", "lane_group",
             "vector_width", "store_width", "grid", "blocked", "stripe",
             "stripe_lanes", "subgroups", "stripes", "tasks_per_wave")
    out = [_i32(0) for _ in names]
    lib().nts_gather_stripe_plan(f, elem_bytes, in_alignment, out_alignment,
                                 rows, batch, edges, schedule, window, stage,
                                 stripe, run, *[_c.byref(o) for o in out])
    plan = {n: o.value for n, o in zip(names, out)}
    plan["staged"] = bool(plan["staged"])
    plan["blocked"] = bool(plan["blocked"])
    return plan


def gather_stripe_tasks(f, in_alignment, out_alignment, rows, batch, edges,
                        n_items, first_slot, count, schedule=0, window=0,
                        stage=0, stripe=0, run=0, elem_bytes=4):
    """The kernel's task decode on the host (no device access): for the
    plan of gather_stripe_plan's arguments and n_items work items, the tasks
    of `count` wave slots from first_slot on, slot = (workgroup * 4 + wave) *
    tasks_per_wave + run index.  Returns (item, first_column, column_bound)
    as numpy uint32 arrays; first_column >= column_bound is a slot without a
    task."""
    import numpy as np
    arrs = [np.zeros(count, dtype=np.uint32) for _ in range(3)]
    lib().nts_gather_stripe_task(f, elem_bytes, in_alignment, out_alignment,
                                 rows, batch, edges, schedule, window, stage,
                                 stripe, run, n_items, first_slot, count,
                                 *[a.ctypes.data for a in arrs])
    return tuple(arrs)


def check_heads(f, heads):
    """1 <= heads <= f and heads | f, else ValueError — the library itself
    aborts on these, so every heads binding checks before it calls."""
    if not (isinstance(heads, int) and isinstance(f, int)
            and 1 <= heads <= f and f % heads == 0):
        raise ValueError(
            f"heads={heads!r} must be a positive divisor of the width {f!r}")


def _plan_heads(entry, f, heads, alignment, batch, edges):
    check_heads(f, heads)
    names = ("lane_group", "vector_width", "grid")
    out = [_i32(0) for _ in names]
    entry(f, heads, alignment, batch, edges, *[_c.byref(o) for o in out])
    return {n: o.value for n, o in zip(names, out)}


def gather_plan_heads(f, heads, alignment, batch, edges):
    """The launch decision of a heads gather (no device access): dict of
    lane_group, vector_width (4, 2 or 1 dwords per lane) and grid."""
    return _plan_heads(lib().nts_gather_plan_heads, f, heads, alignment,
                       batch, edges)


def gather_plan_heads_bf16(f, heads, alignment, batch, edges):
    """gather_plan_heads for bfloat16 feature rows: vector_width is in
    elements per lane (8, 4, 2 or 1), alignment the common alignment of the
    input and the output in bytes."""
    return _plan_heads(lib().nts_gather_plan_heads_bf16, f, heads, alignment,
                       batch, edges)


def check_dropout(p, seed):
    """p a float (or int) that is in [0, 1) as a float32, seed an int in
    [0, 2**64), else ValueError — the library aborts on such a p, so every
    dropout binding checks before it calls."""
    if (isinstance(p, bool) or not isinstance(p, (float, int))
            or not 0 <= p < 1 or _c.c_float(p).value >= 1.0):
        raise ValueError(
            f"dropout={p!r} must be a float in [0, 1) (as a float32)")
    if (isinstance(seed, bool) or not isinstance(seed, int)
            or not 0 <= seed < 2 ** 64):
        raise ValueError(f"seed={seed!r} must be an int in [0, 2**64)")


def edge_dropout_keep(seed, p, first, count):
    """The attention-dropout keep mask as the kernels compute it (no device
    access; the mask is defined in include/nts_hip.h): a numpy bool array,
    element j for position first + j, position = edge * K + head with the
    edge's chunk-local CSC position."""
    import numpy as np
    check_dropout(p, seed)
    if (not isinstance(first, int) or not isinstance(count, int)
            or first < 0 or count < 0 or first + count > 2 ** 64):
        raise ValueError("first, count must be ints with first + count <= 2**64")
    keep = np.zeros(count, dtype=np.uint8)
    lib().nts_edge_dropout_keep(seed, p, first, count, keep.ctypes.data)
    return keep.astype(bool)


# enum nts_reduce_op and NTS_NO_EDGE in include/nts_hip.h
REDUCE_OPS = {"max": 0, "min": 1}
NO_EDGE = 0xFFFFFFFF


def reduce_op(op):
    """The library's code of a max / min aggregation, else ValueError — the
    library aborts on any other op, so every binding checks before it calls."""
    if not isinstance(op, str) or op not in REDUCE_OPS:
        raise ValueError(f"op={op!r} must be 'max' or 'min'")
    return REDUCE_OPS[op]


def reduce_plan(f, alignment, batch, edges, op="max"):
    """The forward launch decision of a max / min gather (no device access):
    dict of lane_group, vector_width, grid (those of gather_plan for the
    request (0, -1)) and scratch_bytes, the merge scratch for split hubs."""
    reduce_op(op)
    names = ("lane_group", "vector_width", "grid")
    out = [_i32(0) for _ in names]
    scratch = _c.c_ulonglong(0)
    lib().nts_reduce_plan(f, alignment, batch, edges,
                          *[_c.byref(o) for o in out], _c.byref(scratch))
    plan = {n: o.value for n, o in zip(names, out)}
    plan["scratch_bytes"] = scratch.value
    return plan


_live_streams = weakref.WeakSet()


@atexit.register
def _destroy_streams_at_exit():
    # Destroy stream objects (draining events, freeing item caches) while the
    # HIP runtime is still alive; leaking them into runtime teardown can
    # abort the process at exit.
    for s in list(_live_streams):
        try:
            s.destroy()
        except Exception:
            pass


class Stream:
    """Thin RAII wrapper over nts_stream (replaces Cuda_Stream,
    /root/reference/cuda/ntsCUDA.hpp:97-217)."""

    def __init__(self, wrap_hip_stream=None):
        l = lib()
        if wrap_hip_stream is None:
            self.h = l.nts_stream_create()
        else:
            # NOTE: torch's default stream handle is 0 (the HIP null stream);
            # it MUST be wrapped, not replaced — launching on a private
            # non-blocking stream would race torch's fills/copies.
            self.h = l.nts_stream_wrap(_vp(wrap_hip_stream))
        self._lib = l
        _live_streams.add(self)

    @classmethod
    def wrap_torch_current(cls):
        import torch
        return cls(wrap_hip_stream=torch.cuda.current_stream().cuda_stream)

    def sync(self):
        self._lib.nts_stream_sync(self.h)

    def timing(self, enable=True):
        self._lib.nts_stream_timing(self.h, 1 if enable else 0)

    def timing_reset(self):
        self._lib.nts_stream_timing_reset(self.h)

    def kernel_ns(self, tag):
        return self._lib.nts_stream_kernel_ns(self.h, tag)

    def kernel_launches(self, tag):
        return self._lib.nts_stream_kernel_launches(self.h, tag)

    def zero(self, dptr, n_floats):
        self._lib.nts_zero_buffer(self.h, _vp(dptr), n_floats)

    def gather_by_dst_from_src(self, x_ptr, y_ptr, w_ptr, row_indices_ptr,
                               column_offset_ptr, src_s, src_e, dst_s, dst_e,
                               edges, batch, f, with_weight=True):
        self._lib.nts_gather_by_dst_from_src(
            self.h, _vp(x_ptr), _vp(y_ptr), _vp(w_ptr), _vp(row_indices_ptr),
            _vp(column_offset_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, 1 if with_weight else 0)

    def gather_by_src_from_dst(self, g_ptr, y_ptr, w_ptr, row_offset_ptr,
                               column_indices_ptr, src_s, src_e, dst_s, dst_e,
                               edges, batch, f, with_weight=True):
        self._lib.nts_gather_by_src_from_dst(
            self.h, _vp(g_ptr), _vp(y_ptr), _vp(w_ptr), _vp(row_offset_ptr),
            _vp(column_indices_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, 1 if with_weight else 0)

    def gather_by_dst_from_src_bf16(self, x_ptr, y_ptr, w_ptr,
                                    row_indices_ptr, column_offset_ptr, src_s,
                                    src_e, dst_s, dst_e, edges, batch, f,
                                    with_weight=True):
        """gather_by_dst_from_src over bfloat16 input rows (fp32 output)."""
        self._lib.nts_gather_by_dst_from_src_bf16(
            self.h, _vp(x_ptr), _vp(y_ptr), _vp(w_ptr), _vp(row_indices_ptr),
            _vp(column_offset_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, 1 if with_weight else 0)

    def gather_by_src_from_dst_bf16(self, g_ptr, y_ptr, w_ptr, row_offset_ptr,
                                    column_indices_ptr, src_s, src_e, dst_s,
                                    dst_e, edges, batch, f, with_weight=True):
        """gather_by_src_from_dst over bfloat16 input rows (fp32 output)."""
        self._lib.nts_gather_by_src_from_dst_bf16(
            self.h, _vp(g_ptr), _vp(y_ptr), _vp(w_ptr), _vp(row_offset_ptr),
            _vp(column_indices_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, 1 if with_weight else 0)

    def deserialize_to_gpu(self, dense_ptr, msg_ptr, count, f, part_s, part_e,
                           sync=False):
        self._lib.nts_deserialize_to_gpu(self.h, _vp(dense_ptr), _vp(msg_ptr),
                                         count, f, part_s, part_e,
                                         1 if sync else 0)

    def aggregate_comm_result(self, master_ptr, msg_ptr, count, f, part_s,
                              part_e, sync=False):
        self._lib.nts_aggregate_comm_result(self.h, _vp(master_ptr),
                                            _vp(msg_ptr), count, f, part_s,
                                            part_e, 1 if sync else 0)

    def gather_rows(self, dense_ptr, packed_ptr, index_ptr, count, row_start, f):
        self._lib.nts_gather_rows(self.h, _vp(dense_ptr), _vp(packed_ptr),
                                  _vp(index_ptr), count, row_start, f)

    def scatter_rows(self, dense_ptr, packed_ptr, index_ptr, count, row_start, f):
        self._lib.nts_scatter_rows(self.h, _vp(dense_ptr), _vp(packed_ptr),
                                   _vp(index_ptr), count, row_start, f)

    def scatter_add_rows(self, dense_ptr, packed_ptr, index_ptr, count,
                         row_start, f):
        self._lib.nts_scatter_add_rows(self.h, _vp(dense_ptr), _vp(packed_ptr),
                                       _vp(index_ptr), count, row_start, f)

    def scatter_src_mirror_to_msg(self, msg, mirror_feat, row_indices,
                                  column_offset, mirror_index, batch, f):
        self._lib.nts_scatter_src_mirror_to_msg(
            self.h, _vp(msg), _vp(mirror_feat), _vp(row_indices),
            _vp(column_offset), _vp(mirror_index), batch, f)

    def gather_msg_to_src_mirror(self, mirror_feat, msg, row_indices,
                                 column_offset, mirror_index, batch, f):
        self._lib.nts_gather_msg_to_src_mirror(
            self.h, _vp(mirror_feat), _vp(msg), _vp(row_indices),
            _vp(column_offset), _vp(mirror_index), batch, f)

    def scatter_dst_to_msg(self, msg, dst_feat, row_indices, column_offset,
                           batch, f):
        self._lib.nts_scatter_dst_to_msg(self.h, _vp(msg), _vp(dst_feat),
                                         _vp(row_indices), _vp(column_offset),
                                         batch, f)

    def gather_msg_to_dst(self, dst_feat, msg, row_indices, column_offset,
                          batch, f):
        self._lib.nts_gather_msg_to_dst(self.h, _vp(dst_feat), _vp(msg),
                                        _vp(row_indices), _vp(column_offset),
                                        batch, f)

    def edge_dot(self, out, dst_rows, src_rows, row_indices, column_offset,
                 src_start, batch, f):
        self._lib.nts_edge_dot(self.h, _vp(out), _vp(dst_rows), _vp(src_rows),
                               _vp(row_indices), _vp(column_offset),
                               src_start, batch, f)

    def scatter_grad_back_to_message(self, input_grad, msg_grad, row_indices,
                                     column_offset, batch, f):
        self._lib.nts_scatter_grad_back_to_message(
            self.h, _vp(input_grad), _vp(msg_grad), _vp(row_indices),
            _vp(column_offset), batch, f)

    def edge_softmax_forward(self, msg_out, msg_in, msg_cached, row_indices,
                             column_offset, batch, f):
        self._lib.nts_edge_softmax_forward(
            self.h, _vp(msg_out), _vp(msg_in), _vp(msg_cached),
            _vp(row_indices), _vp(column_offset), batch, f)

    def edge_softmax_backward(self, msg_in_grad, msg_out_grad, msg_cached,
                              row_indices, column_offset, batch, f):
        self._lib.nts_edge_softmax_backward(
            self.h, _vp(msg_in_grad), _vp(msg_out_grad), _vp(msg_cached),
            _vp(row_indices), _vp(column_offset), batch, f)

    def permute_f32(self, out, inp, index, n):
        self._lib.nts_permute_f32(self.h, _vp(out), _vp(inp), _vp(index), n)

    def edge_softmax_forward_dual(self, out, out_perm, perm_pos, inp, cached,
                                  column_offset, batch, f):
        self._lib.nts_edge_softmax_forward_dual(
            self.h, _vp(out), _vp(out_perm), _vp(perm_pos), _vp(inp),
            _vp(cached), _vp(column_offset), batch, f)

    def edge_softmax_backward_fused(self, in_grad, in_grad_perm, perm_pos,
                                    out_grad, cached, lrelu_input, slope,
                                    column_offset, batch, f, dst_sum=None):
        self._lib.nts_edge_softmax_backward_fused(
            self.h, _vp(in_grad), _vp(in_grad_perm), _vp(perm_pos),
            _vp(out_grad), _vp(cached), _vp(lrelu_input), slope,
            _vp(dst_sum), _vp(column_offset), batch, f)

    def gather_by_src_from_dst_dot(self, inp, out, weight, row_offset,
                                   column_indices, dst_start, batch, edges, f,
                                   dot_vec, dot_out, dot_pos):
        return self._lib.nts_gather_by_src_from_dst_dot(
            self.h, _vp(inp), _vp(out), _vp(weight), _vp(row_offset),
            _vp(column_indices), dst_start, batch, edges, f, _vp(dot_vec),
            _vp(dot_out), _vp(dot_pos))

    def sample_reservoir(self, column_offset, row_indices, dst_list, n_dst,
                         fanout, seed, out_src, out_cnt):
        self._lib.nts_sample_reservoir(self.h, _vp(column_offset),
                                       _vp(row_indices), _vp(dst_list),
                                       n_dst, fanout, seed, _vp(out_src),
                                       _vp(out_cnt))

    def sample_reservoir_dbg_fallback(self, column_offset, row_indices,
                                      dst_list, n_dst, fanout, seed,
                                      out_src, out_cnt):
        """TEST-ONLY: forces the deterministic tie fallback."""
        self._lib.nts_sample_reservoir_dbg_fallback(
            self.h, _vp(column_offset), _vp(row_indices), _vp(dst_list),
            n_dst, fanout, seed, _vp(out_src), _vp(out_cnt))

    def gather_schedule(self, schedule=0, window_floats=0):
        """Column schedule of the following gathers; (0, 0) = automatic."""
        self._lib.nts_gather_schedule(self.h, schedule, window_floats)

    def gather_schedule_last(self):
        """(schedule, window_floats) the most recent gather ran."""
        sched, window = _i32(0), _i32(0)
        self._lib.nts_gather_schedule_last(self.h, _c.byref(sched),
                                           _c.byref(window))
        return sched.value, window.value

    def gather_staging(self, mode=0):
        """Row staging of the following fp32 gathers: 0 automatic, 1 force,
        -1 never."""
        self._lib.nts_gather_staging(self.h, mode)

    def gather_staging_last(self):
        """(staged, pitch_floats) of the most recent gather; pitch 0 if it
        did not stage."""
        staged, pitch = _i32(0), _i32(0)
        self._lib.nts_gather_staging_last(self.h, _c.byref(staged),
                                          _c.byref(pitch))
        return bool(staged.value), pitch.value

    def gather_stripes(self, stripe_floats=0, tasks_per_wave=0):
        """Stripes of the following staged PHASE gathers: 0 automatic, -1
        never, > 0 that width in floats; tasks_per_wave 0 = the fewest that
        fit the grid cap."""
        self._lib.nts_gather_stripes(self.h, stripe_floats)
        self._lib.nts_gather_stripes_run(self.h, tasks_per_wave)

    def gather_stripes_last(self):
        """(stripe_floats, tasks_per_wave) of the most recent gather; (0, 0)
        if it ran without stripes."""
        sf, run = _i32(0), _i32(0)
        self._lib.nts_gather_stripes_last(self.h, _c.byref(sf), _c.byref(run))
        return sf.value, run.value

    def items_cache_clear(self):
        self._lib.nts_items_cache_clear(self.h)

    def items_reuse(self, enable):
        """Opt-in work-item caching; caller must pin its topology buffers."""
        self._lib.nts_items_reuse(self.h, 1 if enable else 0)

    def weight_sum(self, out, weights, offset, batch):
        self._lib.nts_weight_sum(self.h, _vp(out), _vp(weights), _vp(offset),
                                 batch)

    def edge_attention_forward(self, softmax_out, softmax_out_perm, perm_pos,
                               m_sum_out, s_src_mirror, s_dst, row_indices,
                               mirror_index, slope, column_offset, batch):
        self._lib.nts_edge_attention_forward(
            self.h, _vp(softmax_out), _vp(softmax_out_perm), _vp(perm_pos),
            _vp(m_sum_out), _vp(s_src_mirror), _vp(s_dst), _vp(row_indices),
            _vp(mirror_index), slope, _vp(column_offset), batch)

    # ---- per-head edge weights (multi-head GAT); heads is checked here,
    # the library aborts on an invalid value ----
    def gather_by_dst_from_src_heads(self, x_ptr, y_ptr, w_ptr,
                                     row_indices_ptr, column_offset_ptr,
                                     src_s, src_e, dst_s, dst_e, edges, batch,
                                     f, heads):
        """CSC gather with weights [edges, heads] in CSC edge order."""
        check_heads(f, heads)
        self._lib.nts_gather_by_dst_from_src_heads(
            self.h, _vp(x_ptr), _vp(y_ptr), _vp(w_ptr), _vp(row_indices_ptr),
            _vp(column_offset_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, heads)

    def gather_by_src_from_dst_heads(self, g_ptr, y_ptr, w_ptr,
                                     row_offset_ptr, column_indices_ptr,
                                     src_s, src_e, dst_s, dst_e, edges, batch,
                                     f, heads):
        """CSR gather with weights [edges, heads] in CSR edge order."""
        check_heads(f, heads)
        self._lib.nts_gather_by_src_from_dst_heads(
            self.h, _vp(g_ptr), _vp(y_ptr), _vp(w_ptr), _vp(row_offset_ptr),
            _vp(column_indices_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, heads)

    def edge_attention_forward_heads(self, softmax_out, softmax_out_perm,
                                     perm_pos, m_sum_out, s_src_mirror, s_dst,
                                     row_indices, mirror_index, slope,
                                     column_offset, batch, edges, heads):
        check_heads(heads, heads)
        self._lib.nts_edge_attention_forward_heads(
            self.h, _vp(softmax_out), _vp(softmax_out_perm), _vp(perm_pos),
            _vp(m_sum_out), _vp(s_src_mirror), _vp(s_dst), _vp(row_indices),
            _vp(mirror_index), slope, _vp(column_offset), batch, edges, heads)

    def edge_dot_heads(self, out, dst_rows, src_rows, row_indices,
                       column_offset, src_start, batch, edges, f, heads):
        check_heads(f, heads)
        self._lib.nts_edge_dot_heads(
            self.h, _vp(out), _vp(dst_rows), _vp(src_rows), _vp(row_indices),
            _vp(column_offset), src_start, batch, edges, f, heads)

    def weight_sum_heads(self, out, weights, offset, batch, edges, heads):
        check_heads(heads, heads)
        self._lib.nts_weight_sum_heads(self.h, _vp(out), _vp(weights),
                                       _vp(offset), batch, edges, heads)

    # ---- GATv2: the f-wide per-edge score and its backward ----
    def edge_gatv2_score(self, score, dst_rows, src_rows, att, slope,
                         row_indices, column_offset, src_start, batch, edges,
                         f, heads):
        """score[e, k] = att[head k] . leaky_relu(dst_rows[dst] + src_rows[src])
        over head k's columns, e in CSC order (overwrites)."""
        check_heads(f, heads)
        self._lib.nts_edge_gatv2_score(
            self.h, _vp(score), _vp(dst_rows), _vp(src_rows), _vp(att), slope,
            _vp(row_indices), _vp(column_offset), src_start, batch, edges, f,
            heads)

    def edge_gatv2_backward(self, grad_own, grad_att, grad_score, own_rows,
                            nbr_rows, att, slope, offset, nbr_indices,
                            nbr_start, batch, edges, f, heads):
        """One walk over `offset` (CSC: own = x_r, nbr = x_l; CSR the other
        way round) with grad_score in that order: grad_own += ..., and
        grad_att += ... unless grad_att is None/0."""
        check_heads(f, heads)
        self._lib.nts_edge_gatv2_backward(
            self.h, _vp(grad_own), _vp(grad_att), _vp(grad_score),
            _vp(own_rows), _vp(nbr_rows), _vp(att), slope, _vp(offset),
            _vp(nbr_indices), nbr_start, batch, edges, f, heads)

    # ---- bf16 feature rows of the attention passes: the operands named
    # *_bf16 point at bfloat16 rows, everything else is float32 ----
    def gather_by_dst_from_src_heads_bf16(self, x_bf16, y_ptr, w_ptr,
                                          row_indices_ptr, column_offset_ptr,
                                          src_s, src_e, dst_s, dst_e, edges,
                                          batch, f, heads):
        """gather_by_dst_from_src_heads over bfloat16 input rows."""
        check_heads(f, heads)
        self._lib.nts_gather_by_dst_from_src_heads_bf16(
            self.h, _vp(x_bf16), _vp(y_ptr), _vp(w_ptr), _vp(row_indices_ptr),
            _vp(column_offset_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, heads)

    def gather_by_src_from_dst_heads_bf16(self, g_bf16, y_ptr, w_ptr,
                                          row_offset_ptr, column_indices_ptr,
                                          src_s, src_e, dst_s, dst_e, edges,
                                          batch, f, heads):
        """gather_by_src_from_dst_heads over bfloat16 input rows."""
        check_heads(f, heads)
        self._lib.nts_gather_by_src_from_dst_heads_bf16(
            self.h, _vp(g_bf16), _vp(y_ptr), _vp(w_ptr), _vp(row_offset_ptr),
            _vp(column_indices_ptr), src_s, src_e, dst_s, dst_e, edges, batch,
            f, heads)

    def edge_dot_heads_bf16(self, out, dst_rows, src_rows_bf16, row_indices,
                            column_offset, src_start, batch, edges, f, heads):
        """edge_dot_heads with float32 dst_rows and bfloat16 src_rows;
        heads == 1 runs the row-pair kernels with one head."""
        check_heads(f, heads)
        self._lib.nts_edge_dot_heads_bf16(
            self.h, _vp(out), _vp(dst_rows), _vp(src_rows_bf16),
            _vp(row_indices), _vp(column_offset), src_start, batch, edges, f,
            heads)

    def edge_gatv2_score_bf16(self, score, dst_rows_bf16, src_rows_bf16, att,
                              slope, row_indices, column_offset, src_start,
                              batch, edges, f, heads):
        """edge_gatv2_score with both row operands bfloat16."""
        check_heads(f, heads)
        self._lib.nts_edge_gatv2_score_bf16(
            self.h, _vp(score), _vp(dst_rows_bf16), _vp(src_rows_bf16),
            _vp(att), slope, _vp(row_indices), _vp(column_offset), src_start,
            batch, edges, f, heads)

    def edge_gatv2_backward_bf16(self, grad_own, grad_att, grad_score,
                                 own_rows_bf16, nbr_rows_bf16, att, slope,
                                 offset, nbr_indices, nbr_start, batch, edges,
                                 f, heads):
        """edge_gatv2_backward with both row operands bfloat16 (the
        gradients stay float32)."""
        check_heads(f, heads)
        self._lib.nts_edge_gatv2_backward_bf16(
            self.h, _vp(grad_own), _vp(grad_att), _vp(grad_score),
            _vp(own_rows_bf16), _vp(nbr_rows_bf16), _vp(att), slope,
            _vp(offset), _vp(nbr_indices), nbr_start, batch, edges, f, heads)

    # ---- fused GAT inference forward: attention scores, softmax and
    # aggregation with nothing kept per edge ----
    def gat_forward_fused(self, x_ptr, y_ptr, s_src_mirror, s_dst,
                          row_indices, mirror_index, slope, column_offset,
                          src_s, src_e, dst_s, dst_e, edges, batch, f, heads):
        """y[d, c] += sum over d's in-edges of softmax(leaky_relu(s_src[src]
        + s_dst[d]))[e, c // C] * x[src, c]: edge_attention_forward_heads and
        gather_by_dst_from_src_heads in two passes that allocate and write
        nothing of size edges.  mirror_index None/0: s_src_mirror is indexed
        by the global source id.  Honours edge_softmax_stable."""
        check_heads(f, heads)
        self._lib.nts_gat_forward_fused(
            self.h, _vp(x_ptr), _vp(y_ptr), _vp(s_src_mirror), _vp(s_dst),
            _vp(row_indices), _vp(mirror_index), slope, _vp(column_offset),
            src_s, src_e, dst_s, dst_e, edges, batch, f, heads)

    def gat_forward_fused_bf16(self, x_bf16, y_ptr, s_src_mirror, s_dst,
                               row_indices, mirror_index, slope,
                               column_offset, src_s, src_e, dst_s, dst_e,
                               edges, batch, f, heads):
        """gat_forward_fused over bfloat16 input rows."""
        check_heads(f, heads)
        self._lib.nts_gat_forward_fused_bf16(
            self.h, _vp(x_bf16), _vp(y_ptr), _vp(s_src_mirror), _vp(s_dst),
            _vp(row_indices), _vp(mirror_index), slope, _vp(column_offset),
            src_s, src_e, dst_s, dst_e, edges, batch, f, heads)

    # ---- max / min aggregation; op is checked here, the library aborts on
    # an invalid value ----
    def reduce_by_dst_from_src(self, op, x_ptr, y_ptr, arg_ptr,
                               row_indices_ptr, column_offset_ptr, src_s,
                               src_e, dst_s, dst_e, edges, batch, f):
        """y = max / min over in-edges of x rows, arg = the CSC edge position
        that attains it (NO_EDGE and y = 0 without edges).  Overwrites y and
        arg.  row_indices_ptr None/0: x is [edges, f], edge e reads row e."""
        code = reduce_op(op)
        self._lib.nts_reduce_by_dst_from_src(
            self.h, code, _vp(x_ptr), _vp(y_ptr), _vp(arg_ptr),
            _vp(row_indices_ptr), _vp(column_offset_ptr), src_s, src_e, dst_s,
            dst_e, edges, batch, f)

    def reduce_backward(self, op, grad_y_ptr, arg_ptr, row_indices_ptr, src_s,
                        grad_x_ptr, batch, f):
        """grad_x[row_indices[arg] - src_s] += grad_y where arg != NO_EDGE
        (row_indices_ptr None/0: row arg itself).  The scatter is the same for
        both ops; op is taken so a wrong one fails here, not silently."""
        reduce_op(op)
        self._lib.nts_reduce_backward(
            self.h, _vp(grad_y_ptr), _vp(arg_ptr), _vp(row_indices_ptr),
            src_s, _vp(grad_x_ptr), batch, f)

    def heads_dbg_general(self, enable):
        """TEST/MEASUREMENT hook: the general forms of the heads edge
        kernels even where a faster one exists for the shape."""
        self._lib.nts_heads_dbg_general(self.h, 1 if enable else 0)

    def edge_softmax_stable(self, enable):
        """Max-subtracted softmax in the following edge_softmax_forward,
        edge_softmax_forward_dual, edge_attention_forward,
        edge_attention_forward_heads and *_forward_drop calls of this wrapper
        (default off: the reference's exp / sum exp, NaN past a score of
        about 88)."""
        self._lib.nts_edge_softmax_stable(self.h, 1 if enable else 0)

    def edge_softmax_stable_last(self):
        """1 if the most recent of those calls ran the stable form, else 0."""
        stable = _i32(0)
        self._lib.nts_edge_softmax_stable_last(self.h, _c.byref(stable))
        return stable.value

    # ---- attention dropout; (p, seed) is checked here, the library aborts
    # on an invalid p ----
    def edge_attention_forward_drop(self, softmax_out, softmax_out_perm,
                                    perm_pos, m_sum_out, s_src_mirror, s_dst,
                                    row_indices, mirror_index, slope,
                                    column_offset, batch, edges, heads,
                                    alpha_out, p, seed):
        """edge_attention_forward_heads under dropout: alpha_out gets the
        softmax, softmax_out / softmax_out_perm the dropped weights
        keep ? alpha / (1 - p) : 0.  alpha_out must not alias them."""
        check_heads(heads, heads)
        check_dropout(p, seed)
        self._lib.nts_edge_attention_forward_drop(
            self.h, _vp(softmax_out), _vp(softmax_out_perm), _vp(perm_pos),
            _vp(m_sum_out), _vp(s_src_mirror), _vp(s_dst), _vp(row_indices),
            _vp(mirror_index), slope, _vp(column_offset), batch, edges, heads,
            _vp(alpha_out), p, seed)

    def edge_softmax_forward_drop(self, out, out_perm, perm_pos, inp, cached,
                                  column_offset, batch, edges, f, p, seed):
        """edge_softmax_forward_dual under dropout with a caller-known edge
        count: cached gets the softmax (distinct from out), out / out_perm
        the dropped weights."""
        check_dropout(p, seed)
        self._lib.nts_edge_softmax_forward_drop(
            self.h, _vp(out), _vp(out_perm), _vp(perm_pos), _vp(inp),
            _vp(cached), _vp(column_offset), batch, edges, f, p, seed)

    def edge_softmax_backward_drop(self, in_grad, in_grad_perm, perm_pos,
                                   out_grad, cached, lrelu_input, slope,
                                   column_offset, batch, edges, f, p, seed,
                                   dst_sum=None):
        """edge_softmax_backward_fused where out_grad is the gradient of the
        dropped weights of (p, seed) and cached the undropped softmax."""
        check_dropout(p, seed)
        self._lib.nts_edge_softmax_backward_drop(
            self.h, _vp(in_grad), _vp(in_grad_perm), _vp(perm_pos),
            _vp(out_grad), _vp(cached), _vp(lrelu_input), slope,
            _vp(dst_sum), _vp(column_offset), batch, edges, f, p, seed)

    def destroy(self):
        if self.h:
            self._lib.nts_stream_destroy(self.h)
            self.h = None
