/* nts_hip.h — C-ABI of the MI355X-native aggregation runtime.
 *
 * This is the drop-in kernel boundary of the rebuild: it exports, with plain
 * pointers and sizes (no torch types), the method set of the reference's
 * `Cuda_Stream` host shim (/root/reference/cuda/ntsCUDA.hpp:97-217) and its
 * free allocation functions (ntsCUDA.hpp:25-47), re-implemented from scratch
 * as hand-written HIP for gfx950 (see neutronstarlite_amd/csrc/nts_hip.hip).
 * Each declaration cites the reference interface it replaces (file:line in
 * /root/reference).  The reference-side binding a maintainer would add (a
 * `Cuda_Stream` facade over these entry points) is shown in INTEGRATION.md.
 *
 * Conventions kept from the reference (cuda/cuda_type.h:21, dep/gemini/type.hpp:28-30):
 * vertex ids are u32, values are fp32; indices in CSC/CSR chunks follow
 * CSC_segment_pinned (core/GraphSegment.h:52-139): column_offset/row_offset
 * are local to the chunk's vertex range, row_indices/column_indices hold
 * GLOBAL vertex ids (subtract src_start/dst_start in the kernel).
 * Error culture: abort on HIP errors (reference CHECK macro semantics,
 * cuda/ntsCUDAGraphOP.cu:13-19).  All launches are async on the stream
 * object; the host owns every buffer.
 */
#ifndef NTS_HIP_H
#define NTS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef uint32_t nts_vid;     /* VertexId_CUDA, cuda/cuda_type.h:21 */

/* Opaque stream object — replaces class Cuda_Stream (cuda/ntsCUDA.hpp:97-103).
 * One compute stream per GPU op instance; a second stream carries the RCCL
 * ring exchange (driven from the host layer). */
typedef struct nts_stream nts_stream;

nts_stream *nts_stream_create(void);                 /* Cuda_Stream::Cuda_Stream, ntsCUDAGraphOP.cu:60-67 */
nts_stream *nts_stream_wrap(void *hip_stream);       /* wrap an externally owned hipStream_t (e.g. torch's) */
void nts_stream_destroy(nts_stream *s);              /* Cuda_Stream::destory_Stream */
void nts_stream_sync(nts_stream *s);                 /* Cuda_Stream::CUDA_DEVICE_SYNCHRONIZE, ntsCUDAGraphOP.cu:69-75 */
void *nts_stream_handle(nts_stream *s);              /* raw hipStream_t, for torch.cuda.ExternalStream interop */
void nts_stream_wait_stream(nts_stream *waiter, nts_stream *waitee);
    /* stream-ordered cross-stream dependency (hipEventRecord on waitee +
     * hipStreamWaitEvent on waiter): how the comm stream and compute
     * stream of the overlapped ring synchronize (the reference's
     * PROC_OVERLAP, graph.hpp:3490-3535, is the default here) */

/* Kernel-time accounting with HIP events on the launching stream (feeds
 * bench.py's roofline.achieved; replaces the reference's wall-clock
 * accumulators, core/graph.hpp:210-222). */
enum nts_ktag {
  NTS_KTAG_FWD = 0,       /* forward CSC aggregation */
  NTS_KTAG_BWD = 1,       /* backward CSR aggregation */
  NTS_KTAG_DESER = 2,     /* message unpack */
  NTS_KTAG_AGGMSG = 3,    /* partial-sum merge */
  NTS_KTAG_ITEMS = 4,     /* work-item build */
  NTS_KTAG_EDGE = 5,      /* edge-wise (GAT) kernels */
  NTS_KTAG_COUNT = 6
};
void nts_stream_timing(nts_stream *s, int enable);
void nts_stream_timing_reset(nts_stream *s);
/* Synchronizes the stream, then returns accumulated ns / launch count. */
double nts_stream_kernel_ns(nts_stream *s, int tag);
long long nts_stream_kernel_launches(nts_stream *s, int tag);

/* ---- memory (free functions, cuda/ntsCUDA.hpp:25-47) ---- */
void *nts_malloc_gpu(long bytes);                    /* cudaMallocGPU, ntsCUDAGraphOP.cu:51 */
void *nts_malloc_pinned(long bytes);                 /* cudaMallocPinned, ntsCUDAGraphOP.cu:35 */
void *nts_get_device_pointer(void *pinned);          /* getDevicePointer, ntsCUDAGraphOP.cu:23-27 */
void nts_free_gpu(void *p);                          /* FreeBuffer/FreeEdge */
void nts_free_host(void *p);                         /* ntsFreeHost */
void nts_zero_buffer(nts_stream *s, float *d, long n);  /* zero_buffer, async on stream */
void nts_memcpy_h2d(nts_stream *s, void *d, const void *h, long bytes, int sync);  /* move_bytes_in / move_data_in */
void nts_memcpy_d2h(nts_stream *s, void *h, const void *d, long bytes, int sync);  /* move_result_out (fp32-sized correctly; the reference sizes by sizeof(int), ntsCUDAGraphOP.cu:106-108) */

/* ---- fused aggregation (THE hot kernels) ----
 * Replaces Cuda_Stream::Gather_By_Dst_From_Src[_Optim] (ntsCUDA.hpp:125-138;
 * kernels ntsCUDAFuseKernel.cuh:147-309): forward CSC SpMM
 *   output[d,:] += sum_{e in column_offset[d]..[d+1]} w[e] * input[row_indices[e]-src_start,:]
 * over d in [0, batch_size).  ACCUMULATES into output (caller zeroes once per
 * layer; ring chunks then add in place, graph.hpp:3690-3705 semantics).
 * There is no <=512-feature special case: one kernel handles any
 * feature_size by slab decomposition, and power-law columns are split into
 * bounded work items on device (see nts_hip.hip).  with_weight=0 replaces the
 * _without_weight twins.  input holds src_end - src_start rows (backward:
 * dst_end - dst_start) of feature_size floats; a non-empty range lets the
 * launch decision count the matrix and, for row staging below, copy it.
 * tensor_weight: in these two entries an edge weight is ONE fp32 scalar per
 * edge.  The reference's tensor_weight form, a weight row of feature_size
 * values per edge multiplied element by element (the _tensor_weight kernels
 * of ntsCUDAFuseKernel.cuh, Gather_By_Dst_From_Src(..., tensor_weight=true)),
 * is the heads gather below called with heads == feature_size.  Its cost:
 * the column schedules do not apply (the native launch always runs), and
 * with one column per head the lanes run the 4-strided-dword path with one
 * weight load per element, so an edge reads as many weight bytes as row
 * bytes.  Not measured: no exercised config uses it. */
void nts_gather_by_dst_from_src(nts_stream *s,
    const float *input, float *output, const float *weight_forward,
    const nts_vid *row_indices, const nts_vid *column_offset,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, int with_weight);

/* Backward CSR: Cuda_Stream::Gather_By_Src_From_Dst[_Optim]
 * (ntsCUDA.hpp:139-152; kernels ntsCUDAFuseKernel.cuh:327-487):
 *   output[v,:] += sum_{e in row_offset[v]..[v+1]} w[e] * input[column_indices[e]-dst_start,:] */
void nts_gather_by_src_from_dst(nts_stream *s,
    const float *input, float *output, const float *weight_backward,
    const nts_vid *row_offset, const nts_vid *column_indices,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, int with_weight);

/* ---- bfloat16 feature rows (additive, not in the reference ABI) ----
 * The same two gathers over an input matrix stored as bfloat16: row-major
 * [rows, feature_size] raw uint16_t, row pitch 2*feature_size bytes, 2-byte
 * aligned at least.  Weights, accumulation and output stay fp32, and the
 * output keeps the += contract.  A bf16 value is widened exactly (its bits
 * are the high half of the fp32), and each output element is the same fp32
 * fmaf chain over the item's edges in edge order, so for a vertex that is
 * not split into several work items the result is bit-identical to the fp32
 * entry run on the widened values.  What halves is the dominant term of the
 * traffic, the gathered row: about edges*(2f+8) + rows*8f bytes against
 * edges*(4f+8) + rows*8f.  Lane widths: 8 elements (one 16-byte load;
 * feature_size % 8 == 0, input and output 16-byte aligned), 4 (8-byte;
 * % 4, 8-byte aligned), 2 (4-byte; % 2, 4-byte aligned), else 4 strided
 * 2-byte loads per lane.  Schedules, windows (in columns), NTS_SPLIT, the
 * grid caps, the item cache and the NTS_KTAG_FWD / NTS_KTAG_BWD timing tags
 * are shared with the fp32 entries.  bf16 weights or output, the ring, the
 * row pack entries and the fused gather-dot are fp32 only. */
void nts_gather_by_dst_from_src_bf16(nts_stream *s,
    const uint16_t *input, float *output, const float *weight_forward,
    const nts_vid *row_indices, const nts_vid *column_offset,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, int with_weight);
void nts_gather_by_src_from_dst_bf16(nts_stream *s,
    const uint16_t *input, float *output, const float *weight_backward,
    const nts_vid *row_offset, const nts_vid *column_indices,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, int with_weight);

/* ---- per-head edge weights (additive, not in the reference ABI) ----
 * The same two gathers with a ROW of `heads` fp32 weights per edge (multi-
 * head GAT): K = heads, C = feature_size / heads columns per head, columns
 * head-major (column c belongs to head c / C), weights [edges, K] row-major,
 * in CSC edge order for the forward gather and CSR order for the backward:
 *   output[d,c] += sum_{e in column d} w[e*K + c/C] * input[row_indices[e]-src_start, c]
 *   output[v,c] += sum_{e in row v}    w[e*K + c/C] * input[column_indices[e]-dst_start, c]
 * The += contract, the work items, NTS_SPLIT, the item cache and the
 * NTS_KTAG_FWD / NTS_KTAG_BWD tags are those of the scalar gathers.  Lane
 * width: the widest of 4 / 2 dwords that divides C as well as feature_size
 * and that the pointers' alignment permits (a lane then loads one weight per
 * edge), else 4 strided dwords per lane with the head of each element.
 * Only the native launch runs (nts_gather_schedule requests are ignored,
 * nts_gather_schedule_last reports NTS_SCHED_ITEM): GAT widths sit far below
 * the sizes at which the column schedules engage.  heads == 1 IS the scalar
 * entry with with_weight = 1 (same launch); heads == feature_size is the
 * reference's tensor_weight form.  heads == 0, heads > feature_size or
 * feature_size % heads != 0 aborts.  fp32 rows; the bf16 pair follows. */
void nts_gather_by_dst_from_src_heads(nts_stream *s,
    const float *input, float *output, const float *weight_forward,
    const nts_vid *row_indices, const nts_vid *column_offset,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, nts_vid heads);
void nts_gather_by_src_from_dst_heads(nts_stream *s,
    const float *input, float *output, const float *weight_backward,
    const nts_vid *row_offset, const nts_vid *column_indices,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, nts_vid heads);

/* The launch decision of a heads gather, without touching the device (like
 * nts_gather_plan): lane group, dwords per lane (4, 2 or 1) and grid.  With
 * heads == 1 these are nts_gather_plan's for the request (0, -1). */
void nts_gather_plan_heads(nts_vid feature_size, nts_vid heads,
    unsigned alignment_bytes, nts_vid batch_size, nts_vid edges,
    int *lane_group, int *vector_width, int *grid);

/* The heads gathers over bfloat16 rows (additive): `input` as for the scalar
 * bf16 gathers (raw uint16_t, row pitch 2*feature_size bytes, any 2-byte
 * alignment), weights [edges, K], accumulation and `output` fp32, every other
 * part of the contract that of the fp32 heads pair.  A bf16 value is widened
 * exactly, and each output element is one fp32 fmaf chain over the item's
 * edges in edge order whatever the lane width, so for a vertex that is not
 * split the result is bit-identical to the fp32 heads entry run on the
 * widened rows.  Elements per lane: the widest of 8 / 4 / 2 that divides C as
 * well as feature_size and that the pointers' alignment permits — the input
 * load is 16 / 8 / 4 bytes, and the output is accessed in vectors of half as
 * many floats, so it needs the same 16 / 8 / 4 bytes, the rule of
 * nts_gather_plan_bf16 — else 4 strided 2-byte loads per lane with the head
 * of each element.  Lane group: the smallest power of two in [16, 64] that
 * covers feature_size / (elements per lane); grid: (batch_size + edges /
 * NTS_SPLIT + 1) * slabs * lane group threads in workgroups of 256, under
 * the block cap.  heads == 1 IS the scalar bf16 entry with with_weight = 1. */
void nts_gather_by_dst_from_src_heads_bf16(nts_stream *s,
    const uint16_t *input, float *output, const float *weight_forward,
    const nts_vid *row_indices, const nts_vid *column_offset,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, nts_vid heads);
void nts_gather_by_src_from_dst_heads_bf16(nts_stream *s,
    const uint16_t *input, float *output, const float *weight_backward,
    const nts_vid *row_offset, const nts_vid *column_indices,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, nts_vid heads);

/* nts_gather_plan_heads for bf16 rows: vector_width is in elements per lane
 * (8, 4, 2 or 1), alignment_bytes the common alignment of input and output.
 * With heads == 1 these are nts_gather_plan_bf16's for the request (0, -1). */
void nts_gather_plan_heads_bf16(nts_vid feature_size, nts_vid heads,
    unsigned alignment_bytes, nts_vid batch_size, nts_vid edges,
    int *lane_group, int *vector_width, int *grid);

/* ---- max / min neighbour aggregation (additive, not in the reference ABI) ----
 * The reference has these on the CPU only, over a materialised [E, f] edge
 * tensor: SingleCPUDstAggregateOpMax/Min (core/ntsSingleCPUGraphOp.hpp:206-340)
 * and DistAggregateDstMax/Min (core/ntsDistCPUGraphOp.hpp:306-440), built on
 * nts_max / nts_min / nts_assign (core/ntsBaseOp.hpp:135-165) and write_max /
 * write_min (dep/gemini/atomic.hpp:36-52).  Here it is a fused gather: the
 * source rows are read through the CSC index once, the running best and its
 * edge position stay in registers, and a value row and an arg row are written
 * per destination; no [E, f] message tensor is built.
 *   output[d,c] = max (min) over e in column_offset[d]..[d+1] of
 *                 input[row_indices[e]-src_start, c]
 *   arg[d,c]    = the chunk-local CSC edge position e that attains it
 * Tie rule: the LOWEST e wins (the reference's serial write_max, strict <).
 * The comparison is IEEE > / <, so -0 and +0 tie (a vertex split into several
 * work items reports a zero extremum as +0); +-inf are ordinary values, and a
 * vertex with at least one edge always gets a valid arg (the running best is
 * seeded from the first edge).  NaN inputs are unspecified.  A destination
 * with no in-edges gets output = 0 and arg = NTS_NO_EDGE.  The entry
 * OVERWRITES all batch_size rows of both outputs (no += contract; the caller
 * need not zero them).  NOT replicated: the reference zero-initialises its
 * output and compares against it, so there a max over all-negative inputs
 * yields 0 with no record (and its record array, `new VertexId(N)`, holds one
 * element).
 * row_indices == NULL is the reference's message form: input is [edges, f]
 * and edge e reads row e.  fp32 rows only; arg is u32 [batch_size, f].
 * Work items, NTS_SPLIT, the lane widths (4 / 2 dwords, else 4 strided; the
 * alignment is that of input, output and arg together) and the grid are those
 * of the scalar gather's native launch.  Only that launch runs:
 * nts_gather_schedule requests are ignored and nts_gather_schedule_last
 * reports NTS_SCHED_ITEM, as for the heads gathers.  A vertex split into
 * several work items merges through a 64-bit atomic max on a key (ordered
 * value, ~e) in a stream-owned u64 [batch_size, f] scratch, so the tie rule
 * holds at every NTS_SPLIT and no row is read twice; the scratch is
 * 8 * batch_size * feature_size bytes (about 1.1 GB at V = 232 965, f = 602),
 * grows on demand like the stream's other scratch buffers, and is not
 * allocated when edges <= NTS_SPLIT.  No device-to-host copy, no stream
 * synchronize (but for scratch growth).  Timing tag NTS_KTAG_FWD. */
enum nts_reduce_op { NTS_REDUCE_MAX = 0, NTS_REDUCE_MIN = 1 };
#define NTS_NO_EDGE 0xffffffffu
void nts_reduce_by_dst_from_src(nts_stream *s, int op, const float *input,
    float *output, nts_vid *arg, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size);

/* Its backward, a scatter with one lane per (d, c) element:
 *   grad_input[row_indices[arg[d,c]]-src_start, c] += grad_output[d,c]
 * wherever arg[d,c] != NTS_NO_EDGE; with row_indices == NULL the target row
 * is arg[d,c] itself (the nts_assign message-grad form, no collisions).
 * grad_input is caller-zeroed, as for every other += entry.  The adds are
 * fp32 atomics, so the order of additions into one source element is not
 * fixed.  About 12 * V * f bytes plus V * f atomics, against the 8 * E * f a
 * CSR gather testing arg per edge would stream.  Timing tag NTS_KTAG_BWD. */
void nts_reduce_backward(nts_stream *s, const float *grad_output,
    const nts_vid *arg, const nts_vid *row_indices, nts_vid src_start,
    float *grad_input, nts_vid batch_size, nts_vid feature_size);

/* The forward launch decision without touching the device: lane group,
 * vector width and grid are nts_gather_plan's for the request (0, -1) at
 * rows = batch_size; scratch_bytes is the merge scratch the call needs (0
 * when edges <= NTS_SPLIT: no vertex can then be split). */
void nts_reduce_plan(nts_vid feature_size, unsigned alignment_bytes,
    nts_vid batch_size, nts_vid edges, int *lane_group, int *vector_width,
    int *grid, unsigned long long *scratch_bytes);

/* Column schedule of the gather entry points, fp32 and bf16.  A gather task is (work
 * item, column window of `window_floats` floats); the schedule only changes
 * which task runs when, so for a vertex that is not split into several work
 * items the result is bit-identical under every schedule. */
enum nts_gather_sched {
  NTS_SCHED_ITEM = 0,      /* task = item*windows + window (the default) */
  NTS_SCHED_PHASE = 1,     /* task = window*items + item: one window of all
                              rows is live on the chip at a time */
  NTS_SCHED_XCD = 2        /* workgroups with equal blockIdx.x % 8 (one XCD
                              under round-robin placement) own a stripe of
                              windows/8 windows, so each L2 caches one column
                              stripe; the windows % 8 left over are shared out
                              task by task; with 2 or 4 windows, 8/windows
                              classes share one and split the items.  Needs
                              2, 4 or >= 8 windows and >= 8 workgroups, else
                              NTS_SCHED_ITEM runs */
};

/* Request a schedule for this stream's following gathers.  (0, 0) =
 * automatic: chosen per call from the shape.  (0, w != 0) forces
 * NTS_SCHED_ITEM with window w (w < 0: the native slab, i.e. exactly the
 * pre-window launch).  window_floats = 0 with a non-zero schedule takes that
 * schedule's default width; widths are rounded up to the vector width.
 * Environment, for sweeps, when no request is set: NTS_GATHER_SCHED (forces,
 * 0 included) and NTS_GATHER_WINDOW; NTS_GATHER_BLOCKS caps the grid of the
 * column-blocked launches (default 2^20: one task per lane group up to
 * there, which is what lets NTS_SCHED_PHASE keep one window live).
 * The library reads no other environment than these three, the two of row
 * staging (nts_gather_staging), the two of stripes (nts_gather_stripes),
 * NTS_SPLIT (max
 * edges per work item, 256), NTS_MAX_BLOCKS (grid cap of every other launch,
 * 8192) and NTS_DEBUG_SYNC (synchronize and check after every launch). */
void nts_gather_schedule(nts_stream *s, int schedule, int window_floats);

/* The schedule and window the stream's most recent gather actually ran. */
void nts_gather_schedule_last(nts_stream *s, int *schedule, int *window_floats);

/* The launch decision a gather of this shape would take, without touching
 * the device: feature width, common alignment of the input and output
 * pointers in bytes, rows of the gathered matrix (0 = unknown, as in the
 * fused-dot fallback), offsets (batch_size) and edges, and a request as for
 * nts_gather_schedule; the environment counts as it does for a launch.
 * Returns the schedule and window that run, the lane group, the vector
 * width per lane (4, 2 or 1 dwords), the grid in workgroups, and whether the
 * column-blocked kernel instantiation runs.  Any out pointer may be NULL. */
void nts_gather_plan(nts_vid feature_size, unsigned alignment_bytes,
    nts_vid rows, nts_vid batch_size, nts_vid edges, int schedule_req,
    int window_req, int *schedule, int *window_floats, int *lane_group,
    int *vector_width, int *grid, int *blocked);

/* The same for the bf16 entry points (additive): vector_width is in
 * elements per lane (8, 4, 2 or 1), windows are in columns, and "larger than
 * the Infinity Cache" counts the matrix at 2 bytes per element. */
void nts_gather_plan_bf16(nts_vid feature_size, unsigned alignment_bytes,
    nts_vid rows, nts_vid batch_size, nts_vid edges, int schedule_req,
    int window_req, int *schedule, int *window_floats, int *lane_group,
    int *vector_width, int *grid, int *blocked);

/* ---- row staging of the fp32 gather entry points (additive) ----
 * A gather's time follows lane slots and touched 128-byte lines, not payload
 * bytes.  A matrix whose row pitch is no multiple of 16 bytes (f = 602: 2408
 * bytes) runs narrow lanes and most of its windows straddle one more line.
 * Staging copies the gathered matrix, input[0 .. src_end-src_start) (forward;
 * dst_end-dst_start backward) x feature_size, once per call into a buffer at
 * a row pitch `ld` of whole 128-byte lines (feature_size rounded up to 32
 * floats; kernel k_repitch), and the gather reads that buffer with dwordx4
 * lanes, addressing rows by ld instead of feature_size.  Output rows keep
 * pitch feature_size; their vector width (4, 2 or 1 floats) follows the
 * output's own alignment.  Every output element is still one lane's fmaf
 * chain in edge order: for a vertex that is not split into several work
 * items a staged gather is bit-identical to the unstaged one.
 * The buffer belongs to the stream: it grows on demand, is reused by every
 * later staged gather (all uses are ordered on the stream) and is freed by
 * nts_stream_destroy.  The copy runs inside the gather's timing bracket: the
 * NTS_KTAG_FWD / NTS_KTAG_BWD time includes it and the launch count per
 * gather stays 1.  The copy fills the 4-float vector that holds the last
 * column up with zeros, which is as far as the gather reads; pad columns
 * past it are never read.  With no schedule request, a staged launch that
 * meets the blocked-schedule conditions runs NTS_SCHED_PHASE over 128-float
 * windows (the sweep in profiles/bench_lines.md); requests apply to the
 * staged launch as to any other, windows rounded up to 4 floats.
 * mode 0 = automatic: fp32 rows, row count known (src_end > src_start), ld !=
 * feature_size, the blocked-schedule conditions (matrix beyond the Infinity
 * Cache, more than one native slab), at least 64 edges per gathered row (the
 * copy then costs under 3% of the gather's row bytes), and a staged matrix of
 * at most 4 GiB.  mode 1 forces staging for any width and alignment whenever
 * the row count is known and the 4 GiB cap holds (a view at a 4-byte offset
 * goes from strided dwords to dwordx4); mode -1 never stages.  The bf16,
 * heads (heads > 1), max/min and fused-dot gathers never stage.
 * Environment, for sweeps, when the stream has no request: NTS_GATHER_STAGE
 * (1 / -1) and NTS_GATHER_STAGE_PITCH (the unit in floats the pitch is
 * rounded up to, default 32). */
void nts_gather_staging(nts_stream *s, int mode);

/* Whether the stream's most recent gather staged its rows, and the pitch in
 * floats it staged them at (0 if it did not). */
void nts_gather_staging_last(nts_stream *s, int *staged, int *pitch_floats);

/* nts_gather_plan with the staging decision: element size of the rows (4, or
 * 2 for bf16), alignment of the input and of the output pointer in bytes,
 * and the requests as for nts_gather_schedule and nts_gather_staging.
 * Returns whether the rows are staged, the row pitch the gather reads
 * (feature_size if not), the launch that runs (as nts_gather_plan) and the
 * floats per vector access of the output.  Touches no device; any out pointer
 * may be NULL.  nts_gather_plan itself keeps reporting the unstaged launch. */
void nts_gather_stage_plan(nts_vid feature_size, unsigned elem_bytes,
    unsigned in_alignment_bytes, unsigned out_alignment_bytes, nts_vid rows,
    nts_vid batch_size, nts_vid edges, int schedule_req, int window_req,
    int stage_req, int *staged, int *pitch_floats, int *schedule,
    int *window_floats, int *lane_group, int *vector_width, int *store_width,
    int *grid, int *blocked);

/* ---- stripes of a staged NTS_SCHED_PHASE launch (additive) ----
 * Under NTS_SCHED_PHASE every XCD sweeps the same window, so all eight L2s
 * cache pieces of the same hot rows.  With stripes the window of
 * window_floats is cut into S = window_floats / stripe_floats stripes (S = 1,
 * 2, 4 or 8); workgroups with blockIdx.x % 8 = c (one XCD under round-robin
 * placement) own stripe c % S of every window, and the 8 / S classes of a
 * stripe deal the work items among themselves.  The chip is still on one
 * window at a time, but each L2 holds narrower pieces of S times as many
 * rows.  A stripe is stripe_floats / 4 dwordx4 lanes (4 to 64), so a wave
 * holds P = 256 / stripe_floats sub-groups: they share ONE work item and
 * split its edges (sub-group j takes edges j, j + P, ..., four at a time),
 * their partial sums are added by a fixed xor butterfly across the wave, and
 * one sub-group stores.  A wave takes R consecutive tasks (item, window,
 * stripe) of its class, window-major; R is the fewest that fit the grid cap
 * NTS_GATHER_BLOCKS unless more are asked for.  The stripes of a short last
 * window are dealt out over all eight classes task by task (no affinity in
 * that window).  Kernel: k_gather_spmm_stripe, launched instead of
 * k_gather_spmm inside the same timing bracket; launch counts and tags are
 * unchanged.  nts_gather_schedule_last keeps reporting (NTS_SCHED_PHASE,
 * window) and nts_gather_staging_last the pitch: stripes are an attribute of
 * a PHASE launch, not a schedule of their own.
 * Summation order: the sum of a vertex that is not split into several work
 * items is fixed by (first edge, edge count, P), so it is bit-reproducible
 * from run to run, but it is NOT bit-identical to the unstriped launch any
 * more: P fmaf chains and a tree replace one chain.  Split vertices merge
 * with atomics as before.
 * stripe_floats 0 = automatic: fp32 rows, staged and NTS_SCHED_PHASE both by
 * automatic choice (no schedule, window or staging request on the stream or
 * in the environment), automatic width as recorded in profiles/bench_lines.md
 * (Stripes).  -1 never.  > 0 forces that width on any staged launch that runs
 * NTS_SCHED_PHASE or was asked to (a launch of a single window then keeps the
 * window asked for); a width that does not cut the window into 1, 2, 4 or 8
 * stripes of 4 to 64 lanes runs the unstriped launch.
 * Environment, for sweeps, when the stream has no request:
 * NTS_GATHER_STRIPE (floats; -1 never) and NTS_GATHER_STRIPE_RUN (R). */
void nts_gather_stripes(nts_stream *s, int stripe_floats);

/* Ask for at least this many tasks per wave in striped launches (0 = the
 * fewest that fit the grid cap); a sweep parameter. */
void nts_gather_stripes_run(nts_stream *s, int tasks_per_wave);

/* Stripe width in floats and tasks per wave of the stream's most recent
 * gather (0, 0 if it ran without stripes). */
void nts_gather_stripes_last(nts_stream *s, int *stripe_floats,
    int *tasks_per_wave);

/* nts_gather_stage_plan with the stripe decision: its arguments plus the
 * requests as for nts_gather_stripes and nts_gather_stripes_run.  Returns
 * what that one returns for the launch that really runs (a striped launch
 * reports its own grid, a multiple of 8, and its lanes per stripe as the lane
 * group), plus the stripe width in floats (0 = no stripes), lanes per stripe,
 * sub-groups per wave, stripes per window and tasks per wave.  Touches no
 * device; any out pointer may be NULL.  nts_gather_stage_plan and
 * nts_gather_plan keep reporting the launch without stripes. */
void nts_gather_stripe_plan(nts_vid feature_size, unsigned elem_bytes,
    unsigned in_alignment_bytes, unsigned out_alignment_bytes, nts_vid rows,
    nts_vid batch_size, nts_vid edges, int schedule_req, int window_req,
    int stage_req, int stripe_req, int run_req, int *staged,
    int *pitch_floats, int *schedule, int *window_floats, int *lane_group,
    int *vector_width, int *store_width, int *grid, int *blocked,
    int *stripe_floats, int *stripe_lanes, int *subgroups, int *stripes,
    int *tasks_per_wave);

/* The kernel's task decode, evaluated on the host: for the plan of the same
 * arguments and a launch that finds n_items work items, the tasks of `count`
 * consecutive wave slots from first_slot on, where slot = ((workgroup * 4 +
 * wave in the workgroup) * tasks_per_wave + run index).  item[k],
 * first_column[k], column_bound[k] describe slot first_slot + k; first_column
 * >= column_bound marks a slot without a task (also every slot past the grid,
 * and every slot when the plan has no stripes).  Returns the number of slots
 * that hold a task.  The device runs the very same function, so coverage is
 * checkable without a GPU. */
long long nts_gather_stripe_task(nts_vid feature_size, unsigned elem_bytes,
    unsigned in_alignment_bytes, unsigned out_alignment_bytes, nts_vid rows,
    nts_vid batch_size, nts_vid edges, int schedule_req, int window_req,
    int stage_req, int stripe_req, int run_req, nts_vid n_items,
    unsigned long long first_slot, unsigned long long count, nts_vid *item,
    nts_vid *first_column, nts_vid *column_bound);

/* The two gather entry points decompose (offset, batch) into bounded
 * per-wavefront work items on device, rebuilt on every call into a
 * stream-owned scratch buffer (caching by topology pointer would be unsound
 * when the host frees and reallocates chunk buffers).  This entry point is
 * retained for ABI stability; it now only synchronizes the stream. */
void nts_items_cache_clear(nts_stream *s);

/* ---- message transfer (host-bounce compatibility path) ----
 * Replaces Cuda_Stream::deSerializeToGPU (ntsCUDA.hpp:114-117; kernel
 * ntsCUDATransferKernel.cuh:70-93): unpack `count` records
 * [u32 vid | feature_size x f32] (stride feature_size+1 floats) into dense
 * rows vid-partition_start of gpu_buffer.  On the MI355X path the ring moves
 * dense fp32 rows GPU-to-GPU over RCCL and this kernel only serves the
 * compatibility/bounce path and index-scattering of received blocks. */
void nts_deserialize_to_gpu(nts_stream *s, float *gpu_buffer, const float *msg,
    nts_vid count, nts_vid feature_size, nts_vid partition_start,
    nts_vid partition_end, int sync);

/* Replaces Cuda_Stream::aggregate_comm_result_debug (ntsCUDA.hpp:118-122;
 * live kernel aggregate_data_buffer_debug, ntsCUDATransferKernel.cuh:49-68;
 * the un-suffixed :30-47 kernel is dead legacy and is not ported):
 *   master[vid-partition_start,:] += rec[1:] for each record. */
void nts_aggregate_comm_result(nts_stream *s, float *master, const float *msg,
    nts_vid count, nts_vid feature_size, nts_vid partition_start,
    nts_vid partition_end, int sync);

/* ---- ring exchange over dense rows (additive, not in the reference ABI) ----
 * Gather rows listed in `index` (global ids, minus src_start) from a dense
 * block into a packed send buffer, and scatter/accumulate a packed receive
 * buffer into a dense block.  These replace the reference's per-vertex CPU
 * memcpy packing (NtsGraphCommunicator::emit_buffer, comm/network.cpp:476-495)
 * with on-GPU packing feeding RCCL send/recv over xGMI: indices travel once
 * at setup (mirror lists are static), payloads are dense fp32 rows. */
void nts_gather_rows(nts_stream *s, const float *dense, float *packed,
    const nts_vid *index, nts_vid count, nts_vid row_start, nts_vid feature_size);
void nts_scatter_rows(nts_stream *s, float *dense, const float *packed,
    const nts_vid *index, nts_vid count, nts_vid row_start, nts_vid feature_size);
void nts_scatter_add_rows(nts_stream *s, float *dense, const float *packed,
    const nts_vid *index, nts_vid count, nts_vid row_start, nts_vid feature_size);

/* ---- edge-wise kernels (GAT path, config #5) ----
 * Replace Cuda_Stream::Scatter_Src_Mirror_to_Msg / Gather_Msg_To_Src_Mirror /
 * Scatter_Dst_to_Msg / Gather_Msg_to_Dst (ntsCUDA.hpp:154-170; kernels
 * ntsCUDADistKernel.cuh:23-95): materialize per-edge messages from vertex
 * rows and reduce them back.  mirror_index maps global src id ->
 * compressed mirror row (PartitionedGraph::generateMirrorIndex,
 * PartitionedGraph.hpp:295-305). */
void nts_scatter_src_mirror_to_msg(nts_stream *s, float *message,
    const float *src_mirror_feature, const nts_vid *row_indices,
    const nts_vid *column_offset, const nts_vid *mirror_index,
    nts_vid batch_size, nts_vid feature_size);
void nts_gather_msg_to_src_mirror(nts_stream *s, float *src_mirror_feature,
    const float *message, const nts_vid *row_indices,
    const nts_vid *column_offset, const nts_vid *mirror_index,
    nts_vid batch_size, nts_vid feature_size);
void nts_scatter_dst_to_msg(nts_stream *s, float *message,
    const float *dst_feature, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid feature_size);
void nts_gather_msg_to_dst(nts_stream *s, float *dst_feature,
    const float *message, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid feature_size);

/* Replace Cuda_Stream::Edge_Softmax_Forward_Block / _Backward_Block
 * (ntsCUDA.hpp:172-180; kernels ntsCUDADistKernel.cuh:166-260): per-dst
 * softmax over incident-edge values, feature_size values per edge
 * (f=1 attention scalars in the exercised GAT config).  Forward caches
 * the softmax output in msg_cached; backward computes
 *   g_in[e] = s[e]*g_out[e] - s[e] * sum_{e' in dst} s[e']*g_out[e'].
 * The reference's cub::BlockReduce is replaced by a wavefront shuffle
 * reduction. */
void nts_edge_softmax_forward(nts_stream *s, float *msg_output,
    const float *msg_input, float *msg_cached, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid feature_size);
/* ---- additive GAT fusion entries (no reference twin; they fuse the
 * permute / activation-mask / edge-dot passes the decomposed reference
 * chain runs separately — semantics identical, verified in tests) ---- */

/* Edge softmax ALSO emitted at perm_pos[e] (e.g. the CSC->CSR slot map),
 * replacing a separate nts_permute_f32 pass. */
void nts_edge_softmax_forward_dual(nts_stream *s, float *msg_output,
    float *msg_output_perm, const nts_vid *perm_pos, const float *msg_input,
    float *msg_cached, const nts_vid *column_offset, nts_vid batch_size,
    nts_vid feature_size);

/* Softmax backward with the leaky-relu derivative (lrelu_input[m] > 0 ? 1
 * : slope) fused in, dual-emitted like the forward.  dst_sum (optional,
 * f==1 only, caller-zeroed): ALSO accumulates the per-destination sum of
 * the result — the attention scalar's dst gradient — saving a separate
 * f=1 reduction pass. */
void nts_edge_softmax_backward_fused(nts_stream *s, float *msg_input_grad,
    float *msg_input_grad_perm, const nts_vid *perm_pos,
    const float *msg_output_grad, const float *msg_cached,
    const float *lrelu_input, float slope, float *dst_sum,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid feature_size);

/* Fully fused GAT attention forward (f==1 attention scalars): one pass
 * computes m = s_src_mirror[mirror_index[src]] + s_dst[dst] (stashed to
 * m_sum_out for the backward's activation mask), leaky-relu(slope), exp,
 * and per-destination sums; the normalize pass dual-emits the softmax in
 * CSC (softmax_out) and permuted (softmax_out_perm[perm_pos[e]]) order.
 * Replaces Scatter_Src_Mirror_to_Msg + Scatter_Dst_to_Msg + elementwise
 * add/leaky + Edge_Softmax_Forward_Block of the decomposed reference
 * chain (semantics identical; cache = output, reference convention). */
void nts_edge_attention_forward(nts_stream *s, float *softmax_out,
    float *softmax_out_perm, const nts_vid *perm_pos, float *m_sum_out,
    const float *s_src_mirror, const float *s_dst,
    const nts_vid *row_indices, const nts_vid *mirror_index, float slope,
    const nts_vid *column_offset, nts_vid batch_size);

/* Per-vertex sum of per-edge scalars over an offset array (CSC or CSR):
 * out[v] += sum of weights[e] over v's edges — the f=1 degenerate of the
 * weighted gather, done at full lane occupancy (the GAT attention-scalar
 * source gradient).  out is caller-zeroed. */
void nts_weight_sum(nts_stream *s, float *out, const float *weights,
    const nts_vid *offset, nts_vid batch_size);

/* ---- multi-head GAT edge entries (additive) ----
 * K = heads.  Per-edge values (softmax, m_sum, gradients) are fp32
 * [edges, K] row-major, per-vertex attention scalars fp32 [rows, K]
 * row-major; this is what nts_edge_softmax_forward_dual and
 * nts_edge_softmax_backward_fused read and write with feature_size = K.
 * These three take the host-known edge count, as the gathers do, so they
 * add no device-to-host copy and no stream synchronize.  heads == 1 runs the
 * single-head kernel of the entry named in each comment.  Invalid heads
 * abort as for the heads gathers. */

/* nts_edge_attention_forward for K heads: per edge and head
 * m = s_src_mirror[mirror_index[src]*K + k] + s_dst[dst*K + k] (mirror_index
 * NULL = identity), stored to m_sum_out; leaky-relu(slope), exp without max
 * subtraction, per-(destination, head) sums; the shared normalize pass then
 * dual-emits the softmax at softmax_out[e*K + k] and, with perm_pos, at
 * softmax_out_perm[perm_pos[e]*K + k]. */
void nts_edge_attention_forward_heads(nts_stream *s, float *softmax_out,
    float *softmax_out_perm, const nts_vid *perm_pos, float *m_sum_out,
    const float *s_src_mirror, const float *s_dst,
    const nts_vid *row_indices, const nts_vid *mirror_index, float slope,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid edges,
    nts_vid heads);

/* nts_edge_dot per head: out[e*K + k] = sum_{j<C} dst_rows[d, k*C + j] *
 * src_rows[row_indices[e]-src_start, k*C + j], C = feature_size / heads. */
void nts_edge_dot_heads(nts_stream *s, float *out, const float *dst_rows,
    const float *src_rows, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid batch_size,
    nts_vid edges, nts_vid feature_size, nts_vid heads);

/* nts_weight_sum over K columns: out[v*K + k] += sum of weights[e*K + k]
 * over v's edges (CSC or CSR offsets). */
void nts_weight_sum_heads(nts_stream *s, float *out, const float *weights,
    const nts_vid *offset, nts_vid batch_size, nts_vid edges, nts_vid heads);

/* TEST/MEASUREMENT hook: with enable=1 the three heads edge entries above
 * run their general kernel forms (any K, any C) on this stream even where a
 * faster form exists for the shape (attention forward and weight sum: K a
 * power of two <= 64; edge dot: C a power of two <= 256), so both can be
 * tested and timed on the same input. */
void nts_heads_dbg_general(nts_stream *s, int enable);

/* ---- GATv2 attention (additive): the f-wide per-edge score and its backward
 * GATv2 applies the non-linearity before the dot with the attention vector:
 *   t[e, c]     = x_l[src(e), c] + x_r[dst(e), c]        c < f = K*C, head-major
 *   score[e, k] = sum_{j<C} att[k*C + j] * lrelu(t[e, k*C + j])
 * and the [edges, f] tensor t is never stored.  Everything after the score
 * (nts_edge_softmax_forward_dual at feature_size = K, the heads gathers,
 * nts_edge_dot_heads, nts_edge_softmax_backward_fused with lrelu_input NULL)
 * is generic in its input.  Conventions of both entries:
 *   lrelu(t)  = t > 0 ? t : slope*t
 *   lrelu'(t) = t > 0 ? 1 : slope        (slope at t == 0, the rule of
 *                                          nts_edge_softmax_backward_fused)
 *   t is ONE fp32 add of the two loaded row values, so a caller can rebuild
 *   the mask bit for bit from the float32 inputs.
 * att is fp32 [K, C] row-major, that is f floats indexed by column.  As for
 * nts_edge_dot_heads: item-driven with the host-known edge count (no
 * device-to-host copy, no synchronize), timing tag NTS_KTAG_EDGE, invalid
 * heads abort, heads == 1 means C = f, batch_size == 0 or edges == 0 launches
 * nothing and writes nothing.  Correct for every f, every heads dividing f and
 * any 4-byte alignment of each pointer; the fast forms (score: C a power of
 * two with C / R <= 64 lanes per head; backward: R > 1) hold R = 4 / 2 / 1
 * columns per lane by C and the pointers' common alignment, and
 * nts_heads_dbg_general selects the general forms (score: a wave per (edge,
 * head); backward: one column per lane) on the same input. */

/* score[e*K + k] = sum_{j<C} att[k*C+j] * lrelu(dst_rows[d, k*C+j] +
 * src_rows[row_indices[e]-src_start, k*C+j]), e in CSC order, overwritten.
 * Moves the bytes of nts_edge_dot_heads plus att. */
void nts_edge_gatv2_score(nts_stream *s, float *score, const float *dst_rows,
    const float *src_rows, const float *att, float slope,
    const nts_vid *row_indices, const nts_vid *column_offset, nts_vid src_start,
    nts_vid batch_size, nts_vid edges, nts_vid feature_size, nts_vid heads);

/* One walk over an offset array (CSC: own = x_r, nbr = x_l; CSR: own = x_l,
 * nbr = x_r), grad_score [edges, K] in THAT array's edge order:
 *   grad_own[v, c] += sum_{e in v's range} grad_score[e, c/C] * att[c] *
 *                     lrelu'(own[v,c] + nbr[nbr_indices[e]-nbr_start, c])
 *   grad_att[c]    += sum_v sum_e grad_score[e, c/C] *
 *                     lrelu(own[v,c] + nbr[...])      (grad_att NULL: skipped,
 *                                                      nothing is written)
 * Both outputs keep the += contract (caller-zeroed or pre-filled).  grad_own:
 * a lane sums a vertex's edges in edge order and stores with a plain
 * read-add-write; a vertex split into several work items merges with fp32
 * atomics.  grad_att: a lane group sums its columns over all its work items
 * in registers, a workgroup combines its groups through LDS, and one fp32
 * atomic add per (workgroup, column) reaches memory.  The order of those
 * additions is NOT fixed (work-item slots are handed out by an atomic, as
 * for nts_reduce_backward): grad_att, and grad_own on split vertices, vary
 * in the last bits from launch to launch. */
void nts_edge_gatv2_backward(nts_stream *s, float *grad_own, float *grad_att,
    const float *grad_score, const float *own_rows, const float *nbr_rows,
    const float *att, float slope, const nts_vid *offset,
    const nts_vid *nbr_indices, nts_vid nbr_start, nts_vid batch_size,
    nts_vid edges, nts_vid feature_size, nts_vid heads);

/* ---- bfloat16 feature rows for the attention passes (additive) ----
 * nts_edge_dot_heads, nts_edge_gatv2_score and nts_edge_gatv2_backward with
 * feature rows stored as bfloat16 (raw uint16_t, row pitch 2*feature_size
 * bytes, any 2-byte alignment).  Only the operands typed uint16_t below are
 * bf16; att, grad_score, every [edges, K] value, every accumulator and every
 * output stay fp32.  A bf16 value is widened exactly in registers, so each
 * entry computes what its fp32 twin computes on the widened rows; for the
 * GATv2 pair t is ONE fp32 add of the two widened values.  Error culture,
 * NTS_KTAG_EDGE, the item cache, NTS_SPLIT and nts_heads_dbg_general are the
 * fp32 entries'; batch_size == 0 or edges == 0 launches nothing and writes
 * nothing.
 *   Columns per lane: R = the widest of 4 / 2 / 1 that divides C and that
 * every pointer permits by its own element size: R*4 bytes of alignment for
 * an fp32 operand (and for grad_own), R*2 bytes for a bf16 one.  R = 1 and
 * the general forms take 2-byte loads and run at any element offset.  With
 * the R of the fp32 twin (the same form, and pointers that give the twin the
 * same R, e.g. all 16-byte aligned) a lane sums the same columns in the same
 * order and the segment butterfly is the same: the score entries are then
 * bit-identical to the fp32 entries on the widened rows, and so is grad_own
 * on a vertex that is not split.
 *   nts_edge_dot_heads_bf16: dst_rows fp32 (the attention layers pass
 * grad_y), src_rows bf16.  heads == 1 runs the row-pair forms with K = 1;
 * the wave-per-edge kernel of nts_edge_dot stays fp32 only. */
void nts_edge_dot_heads_bf16(nts_stream *s, float *out, const float *dst_rows,
    const uint16_t *src_rows, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid batch_size,
    nts_vid edges, nts_vid feature_size, nts_vid heads);
void nts_edge_gatv2_score_bf16(nts_stream *s, float *score,
    const uint16_t *dst_rows, const uint16_t *src_rows, const float *att,
    float slope, const nts_vid *row_indices, const nts_vid *column_offset,
    nts_vid src_start, nts_vid batch_size, nts_vid edges,
    nts_vid feature_size, nts_vid heads);
void nts_edge_gatv2_backward_bf16(nts_stream *s, float *grad_own,
    float *grad_att, const float *grad_score, const uint16_t *own_rows,
    const uint16_t *nbr_rows, const float *att, float slope,
    const nts_vid *offset, const nts_vid *nbr_indices, nts_vid nbr_start,
    nts_vid batch_size, nts_vid edges, nts_vid feature_size, nts_vid heads);

/* ---- numerically stable edge softmax (additive) ----
 * A request on the stream, as nts_gather_staging is; it reads no environment.
 * With enable != 0 the stream's following nts_edge_softmax_forward,
 * nts_edge_softmax_forward_dual, nts_edge_attention_forward and
 * nts_edge_attention_forward_heads calls compute, per destination and per
 * column or head,
 *   s[e] = exp(a[e] - M) / sum_e' exp(a[e'] - M),  M = max_e' a[e'],
 * over the destination's in-edges, where a is what each entry exponentiates
 * today: the input score, or leaky_relu(s_src[..] + s_dst[..]).  The default
 * (enable == 0) is the reference's exp(a) / sum exp(a), which is NaN once a
 * score passes about 88.7 or all scores of a destination lie below about
 * -103; with enable == 0 the four entries launch exactly the kernels, with
 * the arguments, they launched before this request existed.
 * Everything else the entries promise holds in both modes: m_sum_out (one
 * fp32 add), msg_cached and its aliasing, the dual emission through
 * perm_pos, mirror_index NULL, heads == 1 running the single-head kernel,
 * nts_heads_dbg_general, item reuse, the NTS_KTAG_EDGE tag, no device-to-host
 * copy or synchronize beyond the default's, and destinations without edges
 * writing nothing.  The two passes move the same bytes as the default's; the
 * per-destination state is a (max, sum) pair in a scratch of the stream.  A
 * destination that is one work item stores it without an atomic; one split
 * into several merges the maxima with a 32-bit atomic max, and a third
 * launch, which skips every unsplit item, re-reads the split items' stash
 * and adds their sums with fp32 atomics as the default does.  The
 * backward entries work from the cached softmax output and are not affected.
 * Scores must be finite, except that -inf on a strict subset of a
 * destination's edges gives exactly +0.0f there and the softmax of the rest
 * elsewhere.  A destination whose scores are all -inf, or that has a +inf or
 * a NaN score, is unspecified. */
void nts_edge_softmax_stable(nts_stream *s, int enable);   /* default 0 */
/* Whether the most recent of those four calls ran the stable form (a call
 * that had no edge to work on counts, with the mode it was made in). */
void nts_edge_softmax_stable_last(nts_stream *s, int *stable);

/* ---- attention dropout, fused into the edge softmax (additive) ----
 * Training-time dropout of attention coefficients, per edge and head
 * (GATConv(dropout=), attn_drop): the gathers weigh with
 *   w[e, k] = keep[e, k] ? alpha[e, k] * scale : +0.0f
 * instead of the softmax alpha.  The mask is a function of (seed, e, k)
 * alone and is regenerated wherever it is needed; none is stored.
 *   fmix64(z): z = (z ^ (z >> 33)) * 0xff51afd7ed558ccd;
 *              z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53;  return z ^ (z >> 33);
 *   i     = e*K + k, 64-bit; e the chunk-local CSC edge position, k the head
 *           (or softmax column), K = heads or feature_size
 *   base  = fmix64(seed)                     (once, on the host)
 *   u     = fmix64(base + i) >> 40           (24 bits)
 *   T     = (uint32) lrintf(p * 16777216.0f) (p as fp32, 0 <= p < 1)
 *   keep  = u >= T                           (drops with probability T / 2^24)
 *   scale = 1.0f / (1.0f - p)                (fp32; one fp32 multiply per w)
 * The seed is mixed before the position is added, so seeds s and s + 1 do not
 * give shifted copies of one mask.  p == 0 keeps everything and w equals alpha
 * bit for bit.  The mask does not depend on work-item boundaries, the split,
 * the grid, the lane layout or the softmax mode, and the permuted emission
 * carries the value of the CSC one.  A destination all of whose in-edges drop
 * has only zero weights: its aggregated row is zero.
 * The three stream entries take the host-known edge count (no device-to-host
 * copy, no synchronize), honour nts_edge_softmax_stable (both modes; the
 * forward ones are reported by nts_edge_softmax_stable_last) and launch the
 * kernels of their twins under NTS_KTAG_EDGE: pass 1, the split-sum pass when
 * stable, normalize — no mask pass and no apply pass.  batch_size == 0 or
 * edges == 0 launches nothing.  p outside [0, 1) aborts, as invalid heads do. */

/* The device's own keep decision on the host (touches no device):
 * keep[j] = 1/0 for position first + j, j < count. */
void nts_edge_dropout_keep(unsigned long long seed, float p,
    unsigned long long first, unsigned long long count, uint8_t *keep);

/* nts_edge_attention_forward_heads under dropout.  alpha_out[e*K + k] gets
 * the undropped softmax (what the backward caches: pass 1 stashes into it
 * and the normalize pass finishes it), softmax_out[e*K + k] and, with
 * perm_pos, softmax_out_perm[perm_pos[e]*K + k] get w.  alpha_out must not
 * alias the two weight outputs.  heads == 1 is the one-column layout with
 * the caller-known edge count.  m_sum_out, mirror_index NULL,
 * nts_heads_dbg_general and item reuse as for the heads entry. */
void nts_edge_attention_forward_drop(nts_stream *s, float *softmax_out,
    float *softmax_out_perm, const nts_vid *perm_pos, float *m_sum_out,
    const float *s_src_mirror, const float *s_dst,
    const nts_vid *row_indices, const nts_vid *mirror_index, float slope,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid edges,
    nts_vid heads, float *alpha_out, float p, unsigned long long seed);

/* nts_edge_softmax_forward_dual under dropout, K = feature_size (the GATv2
 * path): msg_cached gets alpha and must be distinct from msg_output;
 * msg_output and, with perm_pos, msg_output_perm get w. */
void nts_edge_softmax_forward_drop(nts_stream *s, float *msg_output,
    float *msg_output_perm, const nts_vid *perm_pos, const float *msg_input,
    float *msg_cached, const nts_vid *column_offset, nts_vid batch_size,
    nts_vid edges, nts_vid feature_size, float p, unsigned long long seed);

/* nts_edge_softmax_backward_fused under dropout: msg_output_grad is the
 * gradient with respect to w in CSC order, and pass 1 uses
 * g = msg_output_grad * (keep ? scale : 0) where the fused entry uses
 * msg_output_grad, the mask regenerated from (seed, e, k).  msg_cached is
 * alpha; lrelu_input / slope, the dual emission and dst_sum (feature_size ==
 * 1 only) as for the fused entry. */
void nts_edge_softmax_backward_drop(nts_stream *s, float *msg_input_grad,
    float *msg_input_grad_perm, const nts_vid *perm_pos,
    const float *msg_output_grad, const float *msg_cached,
    const float *lrelu_input, float slope, float *dst_sum,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid edges,
    nts_vid feature_size, float p, unsigned long long seed);

/* ---- fused GAT inference forward (additive): no per-edge state ----
 * The forward of nts_edge_attention_forward_heads followed by
 * nts_gather_by_dst_from_src_heads[_bf16] for a caller that needs only the
 * aggregated rows (evaluation): per edge e into destination d and head k
 *   t = s_src_mirror[row(e)*K + k] + s_dst[d*K + k]
 *       row(e) = mirror_index ? mirror_index[row_indices[e]] : row_indices[e]
 *   a = lrelu(t, slope)
 *   w = exp(a) / S[d, k]                default, S = sum_e' exp(a[e'])
 *   w = exp(a - M[d, k]) / S[d, k]      under nts_edge_softmax_stable,
 *                                       M = max a, S = sum exp(a - M)
 *   output[d, c] += sum_e w[e, c / C] * input[row_indices[e]-src_start, c]
 * in two passes over the work items of column_offset.  Pass 1 (NTS_KTAG_EDGE)
 * reduces S, or the (M, S) pairs, into the softmax's stream-owned
 * [batch_size, K] scratch and stores nothing per edge; when stable, the short
 * split-sum pass over split destinations follows and recomputes exp(a - M)
 * from the scalars.  Pass 2 (NTS_KTAG_FWD) is the heads gather with w
 * computed in registers from the s_src value fetched next to the source row.
 * Nothing sized by `edges` is allocated, read or written besides row_indices.
 *   output keeps the gathers' += contract: rows without edges are untouched,
 * the caller zeroes.  input is [src_end-src_start, feature_size] fp32 (or
 * bf16 as raw uint16_t, widened exactly), K = heads, C = feature_size / heads,
 * columns head-major; scalars and output are fp32.  mirror_index NULL means
 * identity.  The softmax mode is the stream's (nts_edge_softmax_stable), with
 * the default's NaNs and the stable mode's -inf handling, and the call is
 * recorded for nts_edge_softmax_stable_last.  Invalid heads abort as for the
 * heads gathers; heads == 1 runs the same kernels at K = 1.  batch_size == 0
 * or edges == 0 launches nothing.  The edge count is the caller's: no
 * device-to-host copy and no synchronize.  Lane geometry is the heads
 * gather's for the same (feature_size, heads, alignment of input | output,
 * element size): nts_gather_plan_heads[_bf16] reports it, and
 * nts_heads_dbg_general picks pass 1's lane layout as for the attention
 * forward.  The item cache and NTS_SPLIT apply as everywhere.
 *   On a destination that is one work item, S (or M, S) is reduced in the
 * order of the attention forward's pass 1, w is the expression its normalize
 * pass evaluates (a true division), and each output element is one lane's
 * fmaf chain in edge order: the result is bit-identical to the two-entry
 * chain.  A split destination merges by fp32 atomics, as there. */
void nts_gat_forward_fused(nts_stream *s, const float *input, float *output,
    const float *s_src_mirror, const float *s_dst,
    const nts_vid *row_indices, const nts_vid *mirror_index, float slope,
    const nts_vid *column_offset, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, nts_vid heads);
void nts_gat_forward_fused_bf16(nts_stream *s, const uint16_t *input,
    float *output, const float *s_src_mirror, const float *s_dst,
    const nts_vid *row_indices, const nts_vid *mirror_index, float slope,
    const nts_vid *column_offset, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, nts_vid heads);

/* Opt-in work-item reuse: with enable=1 the stream caches its two most
 * recent item decompositions keyed on (offset pointer, batch, edges) and
 * skips identical rebuilds.  ONLY safe while the caller keeps those
 * topology buffers live and unchanged (e.g. a layer pinning its chunk);
 * nts_items_cache_clear drops the cache. */
void nts_items_reuse(nts_stream *s, int enable);

/* CSR backward gather that ALSO emits the per-edge dot
 * dot_out[dot_pos[e]] = dot(input[column_indices[e]-dst_start], dot_vec[src])
 * from the same streamed row bytes (the GAT attention-scalar gradient).
 * Returns 1 if the fused kernel ran; 0 if the width forced the plain
 * gather (caller must then run nts_edge_dot).  dot_pos NULL = identity. */
int nts_gather_by_src_from_dst_dot(nts_stream *s, const float *input,
    float *output, const float *weight_backward, const nts_vid *row_offset,
    const nts_vid *column_indices, nts_vid dst_start, nts_vid batch_size,
    nts_vid edges, nts_vid feature_size, const float *dot_vec, float *dot_out,
    const nts_vid *dot_pos);

void nts_edge_softmax_backward(nts_stream *s, float *msg_input_grad,
    const float *msg_output_grad, const float *msg_cached,
    const nts_vid *row_indices, const nts_vid *column_offset,
    nts_vid batch_size, nts_vid feature_size);

/* Per-edge dot product (additive entry point): for each edge e of dst d,
 *   out[e] = dot(dst_rows[d,:], src_rows[row_indices[e]-src_start,:]).
 * The GAT backward needs d y/d s[e] = grad_y[dst(e)] . h[src(e)]
 * (ntsDistGPUGraphOp.hpp's chain materializes E x f edge tensors for this;
 * here the dot is fused so only E scalars ever exist). */
void nts_edge_dot(nts_stream *s, float *out, const float *dst_rows,
    const float *src_rows, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid batch_size,
    nts_vid feature_size);

/* Replaces Cuda_Stream::Scatter_Grad_Back_To_Message (ntsCUDA.hpp:193-198;
 * kernel scatter_grad_back_to_messaage, ntsCUDAFuseKernel.cuh:492-506):
 *   message_grad[e,:] += input_grad[d,:] for each edge e of dst d. */
void nts_scatter_grad_back_to_message(nts_stream *s, const float *input_grad,
    float *message_grad, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid batch_size, nts_vid feature_size);

/* ---- GPU-resident neighbor sampling (additive) ----
 * Reservoir fan-out selection on device over the whole-graph CSC
 * (reference semantics: Sampler::reservoir_sample, ntsSampler.hpp:113-166 —
 * keep the first `fanout` edge slots of a column, then slot j >= fanout
 * replaces a uniformly chosen earlier slot with probability fanout/(j+1)).
 * For each of the `n_dst` destinations: writes min(deg, fanout) sampled
 * GLOBAL source ids into out_src[d*fanout ..] and the count into
 * out_cnt[d].  Deterministic in (seed, column content): the per-step RNG is
 * a counter hash of (seed, dst, step).  Compaction into a sampCSC-style
 * local subgraph is host-layer plumbing (torch unique/searchsorted on
 * device — see neutronstarlite_amd/sampler_gpu.py). */
void nts_sample_reservoir(nts_stream *s, const nts_vid *column_offset,
    const nts_vid *row_indices, const nts_vid *dst_list, nts_vid n_dst,
    nts_vid fanout, unsigned long long seed, nts_vid *out_src,
    nts_vid *out_cnt);
/* TEST-ONLY twin: forces the deterministic 64-bit (key,slot) tie fallback
 * so GPU tests can exercise it; results must equal nts_sample_reservoir. */
void nts_sample_reservoir_dbg_fallback(nts_stream *s,
    const nts_vid *column_offset, const nts_vid *row_indices,
    const nts_vid *dst_list, nts_vid n_dst, nts_vid fanout,
    unsigned long long seed, nts_vid *out_src, nts_vid *out_cnt);

/* gather-permute (additive): out[i] = in[index[i]] for f32 values and u32
 * indices — carries per-edge values between CSC and CSR edge order (e.g.
 * attention weights for the backward gather) without host round trips. */
void nts_permute_f32(nts_stream *s, float *out, const float *in,
    const nts_vid *index, long n);

/* Device info for the host layer / bench. */
int nts_device_count(void);
void nts_set_device(int dev);
const char *nts_build_arch(void);   /* "gfx950" */

#ifdef __cplusplus
}
#endif
#endif /* NTS_HIP_H */
