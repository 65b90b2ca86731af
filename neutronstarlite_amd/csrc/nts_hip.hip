/* nts_hip.hip — MI355X-native (gfx950) kernels + C-ABI shim for the
 * NeutronStarLite neighbor-aggregation hot path.
 *
 * Implements include/nts_hip.h.  This is a from-scratch CDNA4 design, not a
 * port of the reference's CUDA kernels (/root/reference/cuda/*.cuh semantics
 * are cited in the header; their fixed <<<128,512>>> geometry, LDS-atomic
 * staging and f<=512 dispatch split are deliberately NOT reproduced):
 *
 *  - The aggregation is HBM-bandwidth-bound gather/scatter (no dense
 *    contraction), so the design maximizes coalesced row traffic: one
 *    64-lane wavefront group reads a source row slab per edge as wide
 *    vector loads (dwordx4 / dwordx2 / 4x strided dword chosen from the
 *    feature width and pointer alignment) and accumulates in REGISTERS —
 *    no LDS staging, no per-element shared-memory atomics.  The gathered
 *    rows may be stored as bfloat16 (half the bytes per edge): the same
 *    kernel, loading 16 / 8 / 4 bytes per lane and widening in registers;
 *    weights, accumulators and output stay fp32.
 *  - Row staging: a large, much re-read fp32 matrix whose row pitch is not
 *    whole 128-byte lines (f = 602) is first copied into a stream-owned
 *    buffer at such a pitch (k_repitch, ~1% of the gather); the gather reads
 *    that with dwordx4 lanes (row pitch `ld` apart from the width f).
 *  - Stripes: such a staged launch cuts each column window into stripes
 *    owned by XCD classes (blockIdx.x % 8), so the eight L2s stop caching
 *    the same rows; the sub-groups of a wave share one work item, split its
 *    edges and add their partial sums in a fixed butterfly, and a wave takes
 *    a contiguous run of tasks (k_gather_spmm_stripe).  Unsplit vertices
 *    stay bit-reproducible but are not bit-identical to k_gather_spmm.
 *  - Power-law load balance: columns are decomposed on device into bounded
 *    work items of <= NTS_SPLIT consecutive edges of one vertex (rebuilt
 *    per call into a stream scratch buffer — two launches, ~0.05% of a
 *    gather); single-item vertices do plain read-modify-write stores,
 *    split (hub) vertices merge with device-scope fp32 atomics.
 *  - Max / min aggregation is the same gather with compare-and-select in
 *    place of fmaf and an edge position carried beside each running best;
 *    split vertices merge through 64-bit atomic-max keys (k_gather_reduce).
 *  - Launches are grid-stride with ~2048 blocks of 256 threads (4 waves),
 *    plenty to fill 256 CUs across 8 XCDs; occupancy (8 waves/SIMD at this
 *    register budget) hides HBM latency.
 *
 * Verified against the CPU oracle (oracle/oracle.c) in tests/test_gpu_parity.py.
 */
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/nts_hip.h"

#define NTS_CHECK(cmd)                                                        \
  do {                                                                        \
    hipError_t e_ = (cmd);                                                    \
    if (e_ != hipSuccess) {                                                   \
      fprintf(stderr, "nts_hip: %s failed: %s (%s:%d)\n", #cmd,               \
              hipGetErrorString(e_), __FILE__, __LINE__);                     \
      abort(); /* reference CHECK culture, ntsCUDAGraphOP.cu:13-19 */         \
    }                                                                         \
  } while (0)

namespace {
constexpr int NTS_BLOCK = 256;        /* 4 waves */

/* Tunables (defaults chosen by measurement on gfx950; env-overridable for
 * sweeps: NTS_SPLIT = max edges per work item, NTS_MAX_BLOCKS = grid cap). */
uint32_t env_u32(const char *name, uint32_t dflt) {
  const char *e = getenv(name);
  if (!e || !*e) return dflt;
  long v = atol(e);
  return v > 0 ? (uint32_t)v : dflt;
}
uint32_t nts_split() {
  static uint32_t v = env_u32("NTS_SPLIT", 256);
  return v;
}
uint32_t nts_max_blocks() {
  static uint32_t v = env_u32("NTS_MAX_BLOCKS", 8192);
  return v;
}
/* grid cap of the column-blocked gather launches: they run faster the less
 * a workgroup strides (profiles/README.md round3), so theirs is set apart
 * from NTS_MAX_BLOCKS.  < 2^24 keeps blockIdx.x * blockDim.x in 32 bits. */
uint32_t nts_gather_blocks() {
  static uint32_t v = min(env_u32("NTS_GATHER_BLOCKS", 1u << 20), 1u << 23);
  return v;
}
#define NTS_SPLIT nts_split()
#define NTS_MAX_BLOCKS nts_max_blocks()

struct ItemsBuf {
  uint4 *items = nullptr;
  uint32_t *counter = nullptr;  /* device: n_items after build */
  uint64_t cap = 0;
  /* opt-in reuse key (see nts_items_reuse): valid only while the caller
   * guarantees the offset buffer is live and unchanged */
  const uint32_t *key_off = nullptr;
  uint32_t key_batch = 0, key_edges = 0;
  bool valid = false;
};
}  // namespace

struct nts_stream {
  hipStream_t stream = nullptr;
  bool owned = false;
  bool timing = false;
  struct Rec { hipEvent_t a, b; int tag; };
  std::vector<Rec> pending;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> freeev;
  double acc_ns[NTS_KTAG_COUNT] = {};
  long long acc_n[NTS_KTAG_COUNT] = {};
  ItemsBuf items_scratch[2]; /* work-item buffers (stream-ordered); two
                                slots so CSC and CSR topologies of one
                                op-chain can both stay cached under
                                nts_items_reuse */
  int items_rr = 0;          /* which slot the next build replaces */
  bool items_reuse = false;  /* opt-in caching (nts_items_reuse) */
  int sched_req = 0, window_req = 0;   /* nts_gather_schedule; 0,0 = auto */
  int sched_last = 0, window_last = 0; /* what the last gather ran */
  float *sums_ws = nullptr;  /* per-dst reduction scratch (softmax) */
  uint64_t sums_cap = 0;
  unsigned long long *pairs_ws = nullptr; /* per-dst (max, sum) pairs (stable
                                             softmax) */
  uint64_t pairs_cap = 0;
  bool softmax_stable = false;      /* nts_edge_softmax_stable */
  bool softmax_stable_last = false; /* what the last softmax forward ran */
  unsigned long long *keys_ws = nullptr; /* hub merge keys (max/min gather) */
  uint64_t keys_cap = 0;
  float *stage_ws = nullptr; /* gathered rows re-pitched (row staging) */
  uint64_t stage_cap = 0;    /* in floats */
  int stage_req = 0;         /* nts_gather_staging: 0 auto, 1 force, -1 never */
  bool staged_last = false;  /* whether the last gather staged its rows ... */
  uint32_t stage_ld_last = 0; /* ... and at which pitch (floats) */
  bool heads_general = false; /* nts_heads_dbg_general: no heads fast paths */
  int stripe_req = 0;        /* nts_gather_stripes: 0 auto, -1 never, > 0 floats */
  int stripe_run_req = 0;    /* nts_gather_stripes_run: 0 = from the grid cap */
  uint32_t stripe_last = 0, stripe_run_last = 0; /* what the last gather ran */
};

namespace {
struct Tic {
  nts_stream *s;
  int tag;
  hipEvent_t a = nullptr, b = nullptr;
  Tic(nts_stream *s_, int tag_) : s(s_), tag(tag_) {
    if (!s->timing) return;
    if (!s->freeev.empty()) {
      a = s->freeev.back().first;
      b = s->freeev.back().second;
      s->freeev.pop_back();
    } else {
      NTS_CHECK(hipEventCreate(&a));
      NTS_CHECK(hipEventCreate(&b));
    }
    NTS_CHECK(hipEventRecord(a, s->stream));
  }
  ~Tic() {
    if (!s->timing || !a) return;
    NTS_CHECK(hipEventRecord(b, s->stream));
    s->pending.push_back({a, b, tag});
  }
};

void drain_timing(nts_stream *s) {
  if (s->pending.empty()) return;
  NTS_CHECK(hipStreamSynchronize(s->stream));
  for (auto &r : s->pending) {
    float ms = 0.f;
    NTS_CHECK(hipEventElapsedTime(&ms, r.a, r.b));
    s->acc_ns[r.tag] += (double)ms * 1e6;
    s->acc_n[r.tag] += 1;
    s->freeev.push_back({r.a, r.b});
  }
  s->pending.clear();
}

/* ------------------------------------------------------------------ */
/* Work-item decomposition: one item = (vertex | shared-flag, first    */
/* edge, edge count <= NTS_SPLIT).  Built on device, no host sync.     */
/* ------------------------------------------------------------------ */
__global__ void k_build_items(const uint32_t *__restrict__ offset,
                              uint32_t batch, uint32_t split,
                              uint4 *__restrict__ items,
                              uint32_t *__restrict__ counter) {
  for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < batch;
       v += gridDim.x * blockDim.x) {
    const uint32_t e0 = offset[v];
    const uint32_t deg = offset[v + 1] - e0;
    if (!deg) continue;
    const uint32_t n = (deg + split - 1) / split;
    const uint32_t base = atomicAdd(counter, n);
    const uint32_t flag = (n > 1) ? 0x80000000u : 0u;
    for (uint32_t j = 0; j < n; ++j) {
      items[base + j] = make_uint4(v | flag, e0 + j * split,
                                   min(split, deg - j * split), 0u);
    }
  }
}

/* ---- device helpers shared by the item-driven kernels ---- */
struct Item {
  uint32_t v;   /* vertex (row of the offset array) */
  bool shared;  /* vertex split into several items: merge with atomics */
  uint32_t e0, cnt;
};
__device__ __forceinline__ Item load_item(const uint4 *__restrict__ items,
                                          uint32_t it) {
  const uint4 x = items[it];
  return Item{x.x & 0x7fffffffu, (x.x >> 31) != 0, x.y, x.z};
}

/* wave-per-item loops: for (it = w.wave; it < n_items; it += w.n_waves) */
struct WaveId { uint32_t wave, lane, n_waves; };
__device__ __forceinline__ WaveId wave_id() {
  return WaveId{(blockIdx.x * blockDim.x + threadIdx.x) >> 6,
                threadIdx.x & 63u, (gridDim.x * blockDim.x) >> 6};
}

/* 64-lane butterfly sum, xor 32..1 in that order (every lane gets it) */
template <typename T>
__device__ __forceinline__ T wave_sum(T x) {
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) x += __shfl_xor(x, w, 64);
  return x;
}
/* same butterfly, keeping the smallest candidate and where it sits */
__device__ __forceinline__ void wave_min(unsigned long long &best,
                                         uint32_t &pos) {
#pragma unroll
  for (int w = 32; w >= 1; w >>= 1) {
    const unsigned long long ob = __shfl_xor(best, w, 64);
    const uint32_t op = __shfl_xor(pos, w, 64);
    if (ob < best) { best = ob; pos = op; }
  }
}

template <int N>
using fvec = float __attribute__((ext_vector_type(N)));  /* dwordxN access */

/* o[0..nv) += acc: plain read-modify-write for an exclusive vertex (vector
 * accesses of OV floats when the lane is full: one, or ELEM/OV where o is
 * only known to be aligned to OV floats), atomicAdd for a split one */
template <int ELEM, int OV = ELEM>
__device__ __forceinline__ void store_acc(float *o, const float (&acc)[ELEM],
                                          int nv, bool shared) {
  static_assert(ELEM % OV == 0, "whole vector accesses");
  if (shared) {
    for (int j = 0; j < nv; ++j) atomicAdd(&o[j], acc[j]);
  } else if (nv == ELEM) {
    fvec<OV> y[ELEM / OV];
#pragma unroll
    for (int c = 0; c < ELEM / OV; ++c)
      y[c] = reinterpret_cast<fvec<OV> *>(o)[c];
#pragma unroll
    for (int j = 0; j < ELEM; ++j) y[j / OV][j % OV] += acc[j];
#pragma unroll
    for (int c = 0; c < ELEM / OV; ++c)
      reinterpret_cast<fvec<OV> *>(o)[c] = y[c];
  } else {
    for (int j = 0; j < nv; ++j) o[j] += acc[j];
  }
}
/* strided twin: element j at o[j*G], live while col + j*G < fend */
template <int NSTR>
__device__ __forceinline__ void store_strided(float *o,
                                              const float (&acc)[NSTR],
                                              uint32_t G, uint32_t col,
                                              uint32_t fend, bool shared) {
  if (!shared) {
#pragma unroll
    for (int j = 0; j < NSTR; ++j)
      if (col + j * G < fend) o[j * G] += acc[j];
  } else {
#pragma unroll
    for (int j = 0; j < NSTR; ++j)
      if (col + j * G < fend) atomicAdd(&o[j * G], acc[j]);
  }
}

/* Column scheduling (BLOCKED): a task is (work item, column window of wf */
/* floats, tile of the lane group inside the window).  The schedules    */
/* only permute which task a group runs when — each output element is   */
/* still one lane's fmaf chain over the item's edges in edge order — so */
/* results are bit-identical across schedules for unsplit vertices.     */
/*   ITEM       t = item*windows + window      (the pre-window order)    */
/*   PHASE      t = window*items + item: the chip sweeps one window of   */
/*              all rows at a time (V*wf*4 B live instead of V*f*4)      */
/*   XCD        workgroups of class blockIdx.x%8 (one XCD under         */
/*              round-robin placement) own a stripe of windows/8         */
/*              windows and stride over all items, so each L2 caches one */
/*              column stripe; the windows%8 left over are shared out    */
/*              task by task, which keeps the classes balanced.  With 2  */
/*              or 4 windows, 8/windows classes share a window and deal  */
/*              the items out among themselves                           */
/* Coverage depends only on blockIdx/gridDim, never on placement.       */
/* BLOCKED=false is the one-tile-per-window ITEM order, bound f.        */
struct GatherPlan {
  uint32_t sched;     /* nts_gather_sched */
  uint32_t wf;        /* window width in floats (multiple of ELEM) */
  uint32_t n_windows; /* ceil(f / wf); 2, 4 or >= 8 for the XCD schedule */
  uint32_t tiles;     /* lane-group tiles per window: ceil(wf / tilef) */
};

/* XCD schedule: what the workgroups of class blockIdx.x % 8 own */
struct XcdClass {
  uint32_t cls = 0;     /* blockIdx.x % 8 */
  uint32_t cpw = 0;     /* classes per window when there are 2 or 4, else 0 */
  uint32_t stripe = 0;  /* tasks per item in a class's own windows/8 stripe */
  uint32_t rest = 0;    /* tasks per item in the windows%8 left over */
  uint64_t striped = 0; /* this class's tasks inside its stripe */
};
struct TaskRange { uint64_t t0, stride, total; };
struct Task { uint32_t it, fbase, fend; };

/* XCD: a group's first task, stride and task count among the workgroups of
 * its class; fills xc for decode_task */
__device__ __forceinline__ TaskRange xcd_range(const GatherPlan &pl,
                                               uint32_t n_items, uint32_t G,
                                               XcdClass &xc) {
  const uint32_t gpb = NTS_BLOCK / G;
  xc.cls = blockIdx.x & 7u;
  xc.stripe = (pl.n_windows >> 3) * pl.tiles;
  xc.rest = (pl.n_windows & 7u) * pl.tiles;
  TaskRange r;
  r.t0 = (uint64_t)(blockIdx.x >> 3) * gpb + threadIdx.x / G;
  r.stride = (uint64_t)((gridDim.x - xc.cls + 7u) >> 3) * gpb;
  if (pl.n_windows >= 8) {
    xc.striped = (uint64_t)n_items * xc.stripe;
    const uint64_t shared = (uint64_t)n_items * xc.rest;
    r.total =
        xc.striped + (shared > xc.cls ? (shared - xc.cls + 7u) >> 3 : 0u);
  } else {
    /* 2 or 4 windows: 8/windows classes share one, items dealt round */
    xc.cpw = 8u / pl.n_windows;
    const uint32_t sub = xc.cls % xc.cpw;
    r.total = n_items > sub
                  ? (uint64_t)((n_items - sub + xc.cpw - 1) / xc.cpw) * pl.tiles
                  : 0u;
  }
  return r;
}

/* task index -> (work item, first column, column bound); fbase >= fend
 * marks a tile past a short last window */
template <bool BLOCKED>
__device__ __forceinline__ Task decode_task(const GatherPlan &pl,
                                            const XcdClass &xc, uint64_t t,
                                            uint32_t n_items, uint32_t f,
                                            uint32_t tilef) {
  const uint32_t per_item = pl.n_windows * pl.tiles;
  if constexpr (!BLOCKED) {
    return Task{(uint32_t)(t / per_item), (uint32_t)(t % per_item) * tilef, f};
  } else {
    uint32_t it, win, tile;
    if (pl.sched == NTS_SCHED_ITEM) {
      it = (uint32_t)(t / per_item);
      const uint32_t r = (uint32_t)(t % per_item);
      win = r / pl.tiles;
      tile = r % pl.tiles;
    } else if (pl.sched == NTS_SCHED_PHASE) {
      const uint64_t per_win = (uint64_t)n_items * pl.tiles;
      win = (uint32_t)(t / per_win);
      const uint64_t r = t % per_win;
      it = (uint32_t)(r / pl.tiles);
      tile = (uint32_t)(r % pl.tiles);
    } else if (xc.cpw) { /* NTS_SCHED_XCD, a window shared by cpw classes */
      it = xc.cls % xc.cpw + xc.cpw * (uint32_t)(t / pl.tiles);
      win = xc.cls / xc.cpw;
      tile = (uint32_t)(t % pl.tiles);
    } else if (t < xc.striped) { /* NTS_SCHED_XCD, own stripe */
      it = (uint32_t)(t / xc.stripe);
      const uint32_t r = xc.cls * xc.stripe + (uint32_t)(t % xc.stripe);
      win = r / pl.tiles;
      tile = r % pl.tiles;
    } else { /* NTS_SCHED_XCD, every 8th task of the left-over windows */
      const uint64_t r = xc.cls + 8u * (t - xc.striped);
      it = (uint32_t)(r / xc.rest);
      const uint32_t j = 8u * xc.stripe + (uint32_t)(r % xc.rest);
      win = j / pl.tiles;
      tile = j % pl.tiles;
    }
    return Task{it, win * pl.wf + tile * tilef, min(f, (win + 1) * pl.wf)};
  }
}

/* Row element types of the gathered matrix: fp32, or bfloat16 held as raw
 * uint16_t.  bits << 16 is the exact fp32 of a bf16 (normals, subnormals,
 * zeros, infinities, NaNs), so a bf16 gather runs the very fmaf chain of the
 * fp32 gather on the upcast values. */
__device__ __forceinline__ float to_f32(float x) { return x; }
__device__ __forceinline__ float to_f32(uint16_t bits) {
  return __uint_as_float((uint32_t)bits << 16);
}

/* one lane's ELEM consecutive row elements as fp32, in one access: dwordxELEM
 * for fp32 rows; ELEM/2 dwords (16, 8 or 4 bytes) for bf16 rows, unpacked in
 * registers — element 2i is the low half of dword i, 2i+1 the high half */
template <int ELEM>
__device__ __forceinline__ void load_lane(const float *p, float (&x)[ELEM]) {
  const fvec<ELEM> v = *reinterpret_cast<const fvec<ELEM> *>(p);
#pragma unroll
  for (int j = 0; j < ELEM; ++j) x[j] = v[j];
}
template <int ELEM>
__device__ __forceinline__ void load_lane(const uint16_t *p,
                                          float (&x)[ELEM]) {
  static_assert(ELEM % 2 == 0, "bf16 lanes load whole dwords");
  uint32_t d[ELEM / 2];
  if constexpr (ELEM == 2) {
    d[0] = *reinterpret_cast<const uint32_t *>(p);
  } else {
    using uvec = uint32_t __attribute__((ext_vector_type(ELEM / 2)));
    const uvec v = *reinterpret_cast<const uvec *>(p);
#pragma unroll
    for (int j = 0; j < ELEM / 2; ++j) d[j] = v[j];
  }
#pragma unroll
  for (int j = 0; j < ELEM / 2; ++j) {
    x[2 * j] = __uint_as_float(d[j] << 16);
    x[2 * j + 1] = __uint_as_float(d[j] & 0xffff0000u);
  }
}

/* the gathered side of one launch */
template <typename T>
struct GatherSrc {
  const uint32_t *nbr;
  const float *ew;
  const T *in;
  uint32_t nbr_start, f;
  uint32_t ld; /* row pitch of `in` in elements: f, or wider for staged rows */
};

/* acc += w[k] * row k for K full vector lanes; fmaf order edge-major,
 * element-minor, all K loads issued before the first fmaf */
template <int ELEM, int K, typename T>
__device__ __forceinline__ void fma_vec(float (&acc)[ELEM],
                                        const T *const (&p)[K],
                                        const float (&wv)[K]) {
  float x[K][ELEM];
#pragma unroll
  for (int k = 0; k < K; ++k) load_lane<ELEM>(p[k], x[k]);
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < ELEM; ++j) acc[j] = fmaf(wv[k], x[k][j], acc[j]);
}
/* strided twin (one dword, or one 2-byte bf16, per access): element j at
 * p[k][j*G], live while col + j*G < fend */
template <int NSTR, int K, typename T>
__device__ __forceinline__ void fma_strided(float (&acc)[NSTR],
                                            const T *const (&p)[K],
                                            const float (&wv)[K], uint32_t G,
                                            uint32_t col, uint32_t fend) {
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < NSTR; ++j)
      if (col + j * G < fend)
        acc[j] = fmaf(wv[k], to_f32(p[k][j * G]), acc[j]);
}

/* K consecutive edges from e on, this lane's columns from col on */
template <int ELEM, bool WITH_W, int K, int N, typename T>
__device__ __forceinline__ void accum_edges(float (&acc)[N],
                                            const GatherSrc<T> &g, uint32_t e,
                                            uint32_t col, uint32_t G,
                                            uint32_t fend) {
  const T *p[K];
  float wv[K];
#pragma unroll
  for (int k = 0; k < K; ++k) {
    p[k] = g.in + (uint64_t)(g.nbr[e + k] - g.nbr_start) * g.ld + col;
    wv[k] = WITH_W ? g.ew[e + k] : 1.0f;
  }
  if constexpr (ELEM == 1) fma_strided<N, K>(acc, p, wv, G, col, fend);
  else fma_vec<ELEM, K>(acc, p, wv);
}

/* one item's edges for a full lane: 4 at a time — 4 independent row loads
 * in flight per wave (one dependent load per iteration leaves HBM latency
 * exposed) — then the tail one by one */
template <int ELEM, bool WITH_W, int N, typename T>
__device__ __forceinline__ void accum_item(float (&acc)[N],
                                           const GatherSrc<T> &g,
                                           const Item &im, uint32_t col,
                                           uint32_t G, uint32_t fend) {
  uint32_t e = im.e0;
  const uint32_t e_end = im.e0 + im.cnt;
  for (; e + 4 <= e_end; e += 4)
    accum_edges<ELEM, WITH_W, 4>(acc, g, e, col, G, fend);
  for (; e < e_end; ++e) accum_edges<ELEM, WITH_W, 1>(acc, g, e, col, G, fend);
}

/* ------------------------------------------------------------------ */
/* THE aggregation kernel. One lane GROUP of G<=64 lanes processes    */
/* one (work item, feature slab): loops the item's edges, vector-loads */
/* the neighbor row slab coalesced, fma-accumulates in registers, then */
/* stores once (RMW for exclusive vertices, atomicAdd for split hubs). */
/* T = row element type of `in`: float, or uint16_t for bfloat16 rows  */
/* (weights, accumulators and `out` are fp32 either way).              */
/* ELEM = elements per lane.  fp32: 4 (dwordx4), 2 (dwordx2), or 1     */
/* with NSTR=4 strided dwords (any f, any 4-byte alignment).  bf16: 8  */
/* (16-byte load), 4 (8-byte), 2 (4-byte), or 1 with NSTR=4 strided    */
/* 2-byte loads (any f, any 2-byte alignment).                         */
/* ld = row pitch of `in` in elements (>= f): f itself, or the pitch of */
/* the stream's staging buffer; rows of `out` always have pitch f.     */
/* OV = floats per vector access of `out` (ELEM % OV == 0): the lane   */
/* width follows `in` (its alignment and ld), OV follows `out` (its    */
/* alignment and f).  The default is their common alignment, which is  */
/* all an unstaged launch can use; a staged launch runs ELEM = 4 with  */
/* OV = 4, 2 or 1.                                                     */
/* Forward CSC:  nbr = row_indices   (global src),  out rows = dst.    */
/* Backward CSR: nbr = column_indices (global dst), out rows = src.    */
/* ------------------------------------------------------------------ */
constexpr int common_ov(int elem, int elem_bytes) {
  return elem * elem_bytes >= 4 ? elem * elem_bytes / 4 : 1;
}
template <typename T, int ELEM, bool WITH_W, bool BLOCKED,
          int OV = common_ov(ELEM, (int)sizeof(T))>
__global__ __launch_bounds__(NTS_BLOCK) void k_gather_spmm(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    const uint32_t *__restrict__ nbr, const float *__restrict__ ew,
    const T *__restrict__ in, float *__restrict__ out, uint32_t nbr_start,
    uint32_t f, uint32_t ld, uint32_t G, GatherPlan pl) {
  constexpr int NSTR = (ELEM == 1) ? 4 : 1;  /* strided sub-elements */
  const uint32_t n_items = *n_items_p;
  const uint32_t glane = threadIdx.x & (G - 1);
  const uint32_t tilef = G * ELEM * NSTR;
  const GatherSrc<T> g{nbr, ew, in, nbr_start, f, ld};
  /* group index and stride: over the whole grid, or (XCD-affine) over the
   * workgroups of this block's class (every launch is NTS_BLOCK wide) */
  XcdClass xc;
  TaskRange r;
  if (BLOCKED && pl.sched == NTS_SCHED_XCD) {
    r = xcd_range(pl, n_items, G, xc);
  } else {
    r.t0 = (blockIdx.x * NTS_BLOCK + threadIdx.x) / G;
    r.stride = (gridDim.x * NTS_BLOCK) / G;
    r.total = (uint64_t)n_items * (pl.n_windows * pl.tiles);
  }

  for (uint64_t t = r.t0; t < r.total; t += r.stride) {
    const Task tk = decode_task<BLOCKED>(pl, xc, t, n_items, f, tilef);
    if (BLOCKED && tk.fbase >= tk.fend) continue;
    const Item im = load_item(items, tk.it);
    float acc[ELEM * NSTR] = {};
    const uint32_t col = tk.fbase + glane * ELEM;
    if constexpr (ELEM == 1) {
      if (col < tk.fend) {
        accum_item<1, WITH_W>(acc, g, im, col, G, tk.fend);
        store_strided(out + (uint64_t)im.v * f + col, acc, G, col, tk.fend,
                      im.shared);
      }
    } else {
      const int nv = (col + ELEM <= tk.fend)
                         ? ELEM : (col < tk.fend ? (int)(tk.fend - col) : 0);
      /* A ragged last lane (nv < ELEM, staged rows of a width that ELEM does
       * not divide) still loads whole vectors while they lie inside the row
       * pitch: k_repitch fills the vector that holds column f - 1 up with
       * zeros, and store_acc drops the elements past nv.  Taking the scalar
       * loop instead makes its wave run every edge twice, the second time
       * one dependent load at a time (measured under PHASE 256 at the
       * headline shape: 75.9 ms/step against 50.3). */
      if (nv > 0 && col + ELEM <= ld) {
        accum_item<ELEM, WITH_W>(acc, g, im, col, G, tk.fend);
      } else if (nv > 0) { /* ragged last lane: scalar columns */
        for (uint32_t e = im.e0; e < im.e0 + im.cnt; ++e) {
          const float w = WITH_W ? ew[e] : 1.0f;
          const T *p = in + (uint64_t)(nbr[e] - nbr_start) * ld + col;
          for (int j = 0; j < nv; ++j) acc[j] = fmaf(w, to_f32(p[j]), acc[j]);
        }
      }
      /* OV floats of `out` per vector access (bf16 ELEM=8: two dwordx4) */
      if (nv > 0)
        store_acc<ELEM, OV>(out + (uint64_t)im.v * f + col, acc, nv,
                            im.shared);
    }
  }
}

/* ---- row staging: the gathered matrix at a wider row pitch ---- */
/* dst[r*ld + c] = src[r*f + c] for r < rows, c < f.  dst is 16-byte aligned
 * and ld % 4 == 0, so every row of dst starts on a 16-byte boundary whatever
 * f and the alignment of src are.  A wave per row, grid-stride: each lane
 * moves 4 consecutive floats per step, so a wave reads 1 KiB of one source
 * row and writes 1 KiB of one staged row, contiguous on both sides; the
 * store is one dwordx4, the load 4/SV accesses of SV floats (SV = 4, 2 or 1
 * from the alignment of src and f).  The vector that holds column f - 1 is
 * filled up with zeros, which is as far as the gather reads (its lanes are
 * vectors of 4 starting below f); pad columns past that vector are left
 * unwritten and never read. */
template <int SV>
__global__ __launch_bounds__(NTS_BLOCK) void k_repitch(
    const float *__restrict__ src, float *__restrict__ dst, uint32_t rows,
    uint32_t f, uint32_t ld) {
  const WaveId w = wave_id();
  for (uint32_t r = w.wave; r < rows; r += w.n_waves) {
    const float *s = src + (uint64_t)r * f;
    float *d = dst + (uint64_t)r * ld;
    for (uint32_t c = w.lane * 4; c < f; c += 64 * 4) {
      fvec<4> v;
      if (c + 4 <= f) {
#pragma unroll
        for (int k = 0; k < 4 / SV; ++k) {
          const fvec<SV> x = *reinterpret_cast<const fvec<SV> *>(s + c + k * SV);
#pragma unroll
          for (int j = 0; j < SV; ++j) v[k * SV + j] = x[j];
        }
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = (c + j < f) ? s[c + j] : 0.f;
      }
      *reinterpret_cast<fvec<4> *>(d + c) = v;
    }
  }
}

/* ---- stripes: edge-parallel waves over XCD-owned column stripes ---- */
/* Sibling of k_gather_spmm<float, 4, WITH_W, true, OV> for staged rows under
 * PHASE, on the same helpers (load_item, load_lane, store_acc, GatherSrc).
 * A window of wf floats is cut into S = wf / sf stripes of sf floats; a
 * stripe is GS = sf / ELEM lanes and a wave holds P = 64 / GS sub-groups.
 * One wave runs one task = (work item, window, stripe) at a time: sub-group j
 * takes the item's edges e0 + j, e0 + j + P, ... four at a time, so a wave
 * step issues the index, weight and row loads of 4 P consecutive edges before
 * its first fmaf.  The P partial sums are combined by an xor butterfly over
 * the lane bits above log2(GS) (xor 32 first, GS last) and sub-group 0 stores
 * once.  The order of the sum is fixed by (e0, cnt, P): unsplit vertices are
 * bit-reproducible run to run, but NOT bit-identical to k_gather_spmm, whose
 * output element is one fmaf chain.
 * Workgroups of class blockIdx.x % 8 (one XCD under round-robin placement)
 * own stripe class % S of every window, so that XCD's L2 caches sf-float
 * pieces of wf / sf times as many rows as under plain PHASE; the 8 / S
 * classes of a stripe deal the items among themselves.  Inside a class the
 * tasks run window-major and every wave takes a contiguous run of R tasks,
 * so launch order is task order and the whole chip stays on one window. */
struct StripePlan {
  uint32_t wf;        /* window width in floats */
  uint32_t sf;        /* stripe width in floats: 4 * GS */
  uint32_t S;         /* stripes per window: 1, 2, 4 or 8 */
  uint32_t R;         /* consecutive tasks of its class per wave */
  uint32_t n_windows; /* ceil(f / wf) */
  uint32_t n_full;    /* leading windows in which all S stripes are live */
  uint32_t last_live; /* live stripes of a short last window, else 0 */
};

/* a / b and a % b; the tasks of a class nearly always fit 32 bits */
__host__ __device__ inline void stripe_divmod(uint64_t a, uint32_t b,
                                              uint64_t &q, uint32_t &r) {
  if (a <= 0xffffffffu) {
    q = (uint32_t)a / b;
    r = (uint32_t)a % b;
  } else {
    q = a / b;
    r = (uint32_t)(a % b);
  }
}

/* The task of (workgroup, wave in the workgroup, run index), or fbase >= fend
 * for none.  Class c = block % 8 owns stripe c % S and, among the 8 / S
 * classes of that stripe, the items c / S, c / S + 8 / S, ...: its tasks are
 * window-major over the n_full full windows.  The tasks of a short last
 * window (item-major over its live stripes) follow, dealt out over all eight
 * classes task by task.  Depends on block and grid alone, never on
 * placement; every live (item, window, stripe) comes out exactly once when
 * grid / 8 * 4 * R covers the largest class (plan_stripe sees to that). */
__host__ __device__ inline Task stripe_task(uint32_t grid, uint32_t n_items,
                                            uint32_t f, const StripePlan &sp,
                                            uint32_t block, uint32_t wave,
                                            uint32_t run) {
  const Task none{0u, 0u, 0u};
  if (block >= grid || run >= sp.R) return none;
  const uint32_t cls = block & 7u, cpw = 8u / sp.S;
  const uint32_t stripe = cls % sp.S, sub = cls / sp.S;
  const uint64_t t =
      ((uint64_t)(block >> 3) * (NTS_BLOCK / 64) + wave) * sp.R + run;
  const uint32_t ni = n_items > sub ? (n_items - sub + cpw - 1) / cpw : 0u;
  const uint64_t own = (uint64_t)sp.n_full * ni;
  uint32_t it, win, st;
  if (t < own) {
    uint64_t w;
    uint32_t slot;
    stripe_divmod(t, ni, w, slot);
    win = (uint32_t)w;
    it = sub + cpw * slot;
    st = stripe;
  } else {
    if (!sp.last_live) return none;
    const uint64_t u = cls + 8u * (t - own);
    if (u >= (uint64_t)n_items * sp.last_live) return none;
    uint64_t q;
    stripe_divmod(u, sp.last_live, q, st);
    it = (uint32_t)q;
    win = sp.n_windows - 1;
  }
  const uint32_t fbase = win * sp.wf + st * sp.sf;
  const uint32_t fend = fbase + sp.sf;
  return Task{it, fbase, fend < f ? fend : f};
}

/* one wave step: 4 edges per sub-group, P apart.  FULL: all 4 P edges from
 * eb on exist.  Otherwise the step is the item's tail: an edge slot past
 * e_end reads the item's last edge instead (a valid address) and is left
 * out of the sum */
template <int ELEM, bool WITH_W, bool FULL>
__device__ __forceinline__ void stripe_edges(float (&acc)[ELEM],
                                             const GatherSrc<float> &g,
                                             uint32_t eb, uint32_t e_end,
                                             uint32_t sub, uint32_t P,
                                             uint32_t col) {
  uint32_t idx[4];
  float wv[4];
  bool live[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    uint32_t e = eb + k * P + sub;
    live[k] = FULL || e < e_end;
    if (!FULL) e = min(e, e_end - 1);
    idx[k] = g.nbr[e];
    wv[k] = WITH_W ? g.ew[e] : 1.0f;
  }
  float x[4][ELEM];
#pragma unroll
  for (int k = 0; k < 4; ++k)
    load_lane<ELEM>(g.in + (uint64_t)(idx[k] - g.nbr_start) * g.ld + col,
                    x[k]);
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (live[k]) {
#pragma unroll
      for (int j = 0; j < ELEM; ++j) acc[j] = fmaf(wv[k], x[k][j], acc[j]);
    }
}

template <int ELEM, bool WITH_W, int OV, int GS>
__global__ __launch_bounds__(NTS_BLOCK) void k_gather_spmm_stripe(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    const uint32_t *__restrict__ nbr, const float *__restrict__ ew,
    const float *__restrict__ in, float *__restrict__ out, uint32_t nbr_start,
    uint32_t f, uint32_t ld, StripePlan sp) {
  static_assert(GS >= 4 && GS <= 64 && (GS & (GS - 1)) == 0, "lanes a stripe");
  constexpr uint32_t P = 64 / GS;
  const uint32_t n_items = *n_items_p;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t sub = lane / GS, glane = lane % GS;
  const uint32_t wave = threadIdx.x >> 6;
  const GatherSrc<float> g{nbr, ew, in, nbr_start, f, ld};
  for (uint32_t run = 0; run < sp.R; ++run) {
    const Task tk =
        stripe_task(gridDim.x, n_items, f, sp, blockIdx.x, wave, run);
    if (tk.fbase >= tk.fend) continue; /* the same for the whole wave */
    const Item im = load_item(items, tk.it);
    const uint32_t col = tk.fbase + glane * ELEM;
    const int nv = (col + ELEM <= tk.fend)
                       ? ELEM : (col < tk.fend ? (int)(tk.fend - col) : 0);
    float acc[ELEM] = {};
    /* col and ld are multiples of ELEM and col < f <= ld: a live lane's
     * vector lies inside the row pitch, and k_repitch has filled the vector
     * that holds column f - 1 up with zeros (the ragged last lane) */
    if (nv > 0) {
      const uint32_t e_end = im.e0 + im.cnt;
      uint32_t eb = im.e0;
      for (; eb + 4 * P <= e_end; eb += 4 * P)
        stripe_edges<ELEM, WITH_W, true>(acc, g, eb, e_end, sub, P, col);
      if (eb < e_end)
        stripe_edges<ELEM, WITH_W, false>(acc, g, eb, e_end, sub, P, col);
    }
    /* whole-wave butterfly (lanes past the stripe's columns add zeros) */
#pragma unroll
    for (int w = 32; w >= GS; w >>= 1)
#pragma unroll
      for (int j = 0; j < ELEM; ++j) acc[j] += __shfl_xor(acc[j], w, 64);
    if (sub == 0 && nv > 0)
      store_acc<ELEM, OV>(out + (uint64_t)im.v * f + col, acc, nv, im.shared);
  }
}

/* ---- multi-head gather: a row of K weights per edge ---- */
/* Sibling of k_gather_spmm<float, ELEM, true, false> on the same helpers
 * (decode_task, fma_vec, store_acc, store_strided): a lane group per (work
 * item, slab), four row loads in flight, register accumulation, one store.
 * Columns are head-major, C per head, and edge e scales column c by
 * ew[e*K + c/C].  ELEM = 4 or 2 is chosen to divide C as well as f, so a
 * lane's vector never straddles two heads and the lane loads ONE weight per
 * edge (f % ELEM == 0: every live lane is full, there is no ragged lane);
 * ELEM = 1 runs 4 strided dwords per lane with the head of each element.
 * T = row element type of `in`, as for k_gather_spmm: with uint16_t (bf16)
 * rows ELEM is 8, 4 or 2 (one 16-, 8- or 4-byte load; `out` is accessed in
 * vectors of ELEM/2 floats), or 1 with 4 strided 2-byte loads, which is the
 * form for any 2-byte alignment of `in`.  Weights, accumulators and `out` are
 * fp32, and each output element is the fp32 instantiation's fmaf chain on
 * the widened values whatever the lane width. */
template <int ELEM, int NE, typename T>
__device__ __forceinline__ void heads_edges_vec(float (&acc)[ELEM],
                                                const GatherSrc<T> &g,
                                                uint32_t e, uint32_t col,
                                                uint32_t K, uint32_t head) {
  const T *p[NE];
  float wv[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    p[k] = g.in + (uint64_t)(g.nbr[e + k] - g.nbr_start) * g.ld + col;
    wv[k] = g.ew[(uint64_t)(e + k) * K + head];
  }
  fma_vec<ELEM, NE>(acc, p, wv);
}
/* strided twin: element j at column col + j*G, head hd[j], live while
 * col + j*G < f */
template <int NSTR, int NE, typename T>
__device__ __forceinline__ void heads_edges_strided(
    float (&acc)[NSTR], const GatherSrc<T> &g, uint32_t e, uint32_t col,
    uint32_t G, uint32_t K, const uint32_t (&hd)[NSTR]) {
  const T *p[NE];
  const float *wrow[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    p[k] = g.in + (uint64_t)(g.nbr[e + k] - g.nbr_start) * g.ld + col;
    wrow[k] = g.ew + (uint64_t)(e + k) * K;
  }
#pragma unroll
  for (int k = 0; k < NE; ++k)
#pragma unroll
    for (int j = 0; j < NSTR; ++j)
      if (col + j * G < g.f)
        acc[j] = fmaf(wrow[k][hd[j]], to_f32(p[k][j * G]), acc[j]);
}

template <int ELEM, typename T = float>
__global__ __launch_bounds__(NTS_BLOCK) void k_gather_spmm_heads(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    const uint32_t *__restrict__ nbr, const float *__restrict__ ew,
    const T *__restrict__ in, float *__restrict__ out, uint32_t nbr_start,
    uint32_t f, uint32_t G, uint32_t n_slabs, uint32_t K, uint32_t C) {
  constexpr int NSTR = (ELEM == 1) ? 4 : 1;
  const uint32_t n_items = *n_items_p;
  const uint32_t glane = threadIdx.x & (G - 1);
  const uint32_t tilef = G * ELEM * NSTR;
  const GatherSrc<T> g{nbr, ew, in, nbr_start, f, f};
  const GatherPlan pl{NTS_SCHED_ITEM, tilef, n_slabs, 1u};
  const XcdClass xc;
  const uint64_t total = (uint64_t)n_items * n_slabs;
  const uint64_t stride = (gridDim.x * NTS_BLOCK) / G;
  for (uint64_t t = (blockIdx.x * NTS_BLOCK + threadIdx.x) / G; t < total;
       t += stride) {
    const Task tk = decode_task<false>(pl, xc, t, n_items, f, tilef);
    const uint32_t col = tk.fbase + glane * ELEM;
    if (col >= f) continue;
    const Item im = load_item(items, tk.it);
    const uint32_t e_end = im.e0 + im.cnt;
    uint32_t e = im.e0;
    float acc[ELEM * NSTR] = {};
    float *o = out + (uint64_t)im.v * f + col;
    if constexpr (ELEM == 1) {
      uint32_t hd[NSTR];
#pragma unroll
      for (int j = 0; j < NSTR; ++j)
        hd[j] = (col + j * G < f) ? (col + j * G) / C : 0u;
      for (; e + 4 <= e_end; e += 4)
        heads_edges_strided<NSTR, 4>(acc, g, e, col, G, K, hd);
      for (; e < e_end; ++e)
        heads_edges_strided<NSTR, 1>(acc, g, e, col, G, K, hd);
      store_strided(o, acc, G, col, f, im.shared);
    } else {
      const uint32_t head = col / C;
      for (; e + 4 <= e_end; e += 4)
        heads_edges_vec<ELEM, 4>(acc, g, e, col, K, head);
      for (; e < e_end; ++e) heads_edges_vec<ELEM, 1>(acc, g, e, col, K, head);
      store_acc<ELEM, common_ov(ELEM, (int)sizeof(T))>(o, acc, ELEM,
                                                       im.shared);
    }
  }
}

/* ---- max / min gather with an arg record ---- */
/* Sibling of k_gather_spmm<float, ELEM, false, false> on the same helpers
 * (decode_task, load_item, load_lane): a lane group per (work item, slab),
 * four row loads in flight.  fmaf becomes compare-and-select: each lane keeps
 * best[] and the edge position bestE[] that attained it, seeded from the
 * item's first edge and updated with a strict compare in edge order, so the
 * lowest position wins a tie and -0 ties +0.  MSG: edge e reads row e (the
 * message form, nbr == NULL).  An exclusive vertex stores its value and arg rows; a
 * split one merges with a 64-bit atomic max on reduce_key (below). */
template <bool IS_MIN>
__device__ __forceinline__ bool reduce_beats(float x, float best) {
  return IS_MIN ? x < best : x > best;
}

/* (ordered value << 32) | ~e: the monotone float -> uint map (flip all bits
 * of a negative, set the sign bit of the rest; complemented for min) above
 * the complemented edge position, so a 64-bit max picks the better value and,
 * among equal ones, the lowest e.  -0 is folded onto +0 first, so the two tie
 * as they do under the register path's IEEE compare.  Every key of a real
 * edge is > 0: the high word of a non-NaN is, and so is ~e for e < 2^32 - 1. */
template <bool IS_MIN>
__device__ __forceinline__ unsigned long long reduce_key(float x, uint32_t e) {
  uint32_t u = __float_as_uint(x);
  if (u == 0x80000000u) u = 0u;
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
  if (IS_MIN) u = ~u;
  return ((unsigned long long)u << 32) | (0xffffffffu - e);
}
template <bool IS_MIN>
__device__ __forceinline__ void reduce_unkey(unsigned long long key, float &x,
                                             uint32_t &e) {
  uint32_t u = (uint32_t)(key >> 32);
  if (IS_MIN) u = ~u;
  u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
  x = __uint_as_float(u);
  e = 0xffffffffu - (uint32_t)key;
}

/* MSG (the message form) is a template parameter, not a test of g.nbr: a
 * conditional index load inside the edge loop compiles to a branch and a full
 * wait per edge, which serializes the four index loads of a batch */
template <bool MSG>
__device__ __forceinline__ const float *reduce_row(const GatherSrc<float> &g,
                                                   uint32_t e, uint32_t col) {
  const uint32_t row = MSG ? e : g.nbr[e] - g.nbr_start;
  return g.in + (uint64_t)row * g.ld + col;
}

/* K consecutive edges from e on, this lane's columns from col on: all K row
 * loads issued before the first compare; SEED assigns instead (the item's
 * first edge).  ELEM == 1: element j at p[j*G], live while col + j*G < fend
 * (a dead element compares zeros and is never stored). */
template <int ELEM, int K, bool IS_MIN, bool MSG, bool SEED, int N>
__device__ __forceinline__ void reduce_edges(float (&best)[N],
                                             uint32_t (&bestE)[N],
                                             const GatherSrc<float> &g,
                                             uint32_t e, uint32_t col,
                                             uint32_t G, uint32_t fend) {
  const float *p[K];
  float x[K][N];
#pragma unroll
  for (int k = 0; k < K; ++k) p[k] = reduce_row<MSG>(g, e + k, col);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    if constexpr (ELEM == 1) {
#pragma unroll
      for (int j = 0; j < N; ++j)
        x[k][j] = (col + j * G < fend) ? p[k][j * G] : 0.f;
    } else {
      load_lane<ELEM>(p[k], x[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k)
#pragma unroll
    for (int j = 0; j < N; ++j)
      if (SEED || reduce_beats<IS_MIN>(x[k][j], best[j])) {
        best[j] = x[k][j];
        bestE[j] = e + k;
      }
}

template <int ELEM, bool IS_MIN, bool MSG, int N>
__device__ __forceinline__ void reduce_item(float (&best)[N],
                                            uint32_t (&bestE)[N],
                                            const GatherSrc<float> &g,
                                            const Item &im, uint32_t col,
                                            uint32_t G, uint32_t fend) {
  uint32_t e = im.e0;
  const uint32_t e_end = im.e0 + im.cnt;
  reduce_edges<ELEM, 1, IS_MIN, MSG, true>(best, bestE, g, e, col, G, fend);
  for (++e; e + 4 <= e_end; e += 4)
    reduce_edges<ELEM, 4, IS_MIN, MSG, false>(best, bestE, g, e, col, G, fend);
  for (; e < e_end; ++e)
    reduce_edges<ELEM, 1, IS_MIN, MSG, false>(best, bestE, g, e, col, G, fend);
}

template <int ELEM, bool IS_MIN, bool MSG>
__global__ __launch_bounds__(NTS_BLOCK) void k_gather_reduce(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    const uint32_t *__restrict__ nbr, const float *__restrict__ in,
    float *__restrict__ out, uint32_t *__restrict__ arg,
    unsigned long long *__restrict__ keys, uint32_t nbr_start, uint32_t f,
    uint32_t G, uint32_t n_slabs) {
  constexpr int NSTR = (ELEM == 1) ? 4 : 1;
  constexpr int N = ELEM * NSTR;
  using uvec = uint32_t __attribute__((ext_vector_type(ELEM)));
  const uint32_t n_items = *n_items_p;
  const uint32_t glane = threadIdx.x & (G - 1);
  const uint32_t tilef = G * N;
  const GatherSrc<float> g{nbr, nullptr, in, nbr_start, f, f};
  const GatherPlan pl{NTS_SCHED_ITEM, tilef, n_slabs, 1u};
  const XcdClass xc;
  const uint64_t total = (uint64_t)n_items * n_slabs;
  const uint64_t stride = (gridDim.x * NTS_BLOCK) / G;
  for (uint64_t t = (blockIdx.x * NTS_BLOCK + threadIdx.x) / G; t < total;
       t += stride) {
    const Task tk = decode_task<false>(pl, xc, t, n_items, f, tilef);
    const uint32_t col = tk.fbase + glane * ELEM;
    if (col >= f) continue;
    const Item im = load_item(items, tk.it);
    const uint64_t o = (uint64_t)im.v * f + col;
    float best[N];
    uint32_t bestE[N];
    if constexpr (ELEM == 1) {
      reduce_item<1, IS_MIN, MSG>(best, bestE, g, im, col, G, f);
#pragma unroll
      for (int j = 0; j < N; ++j) {
        if (col + j * G >= f) continue;
        if (im.shared) {
          atomicMax(&keys[o + j * G], reduce_key<IS_MIN>(best[j], bestE[j]));
        } else {
          out[o + j * G] = best[j];
          arg[o + j * G] = bestE[j];
        }
      }
    } else {
      const int nv = (col + ELEM <= f) ? ELEM : (int)(f - col);
      if (nv == ELEM) {
        reduce_item<ELEM, IS_MIN, MSG>(best, bestE, g, im, col, G, f);
      } else { /* ragged last lane: scalar columns */
        for (uint32_t e = im.e0; e < im.e0 + im.cnt; ++e) {
          const float *p = reduce_row<MSG>(g, e, col);
          for (int j = 0; j < nv; ++j) {
            const float x = p[j];
            if (e == im.e0 || reduce_beats<IS_MIN>(x, best[j])) {
              best[j] = x;
              bestE[j] = e;
            }
          }
        }
      }
      if (im.shared) {
        for (int j = 0; j < nv; ++j)
          atomicMax(&keys[o + j], reduce_key<IS_MIN>(best[j], bestE[j]));
      } else if (nv == ELEM) {
        fvec<ELEM> y;
        uvec a;
#pragma unroll
        for (int j = 0; j < ELEM; ++j) {
          y[j] = best[j];
          a[j] = bestE[j];
        }
        *reinterpret_cast<fvec<ELEM> *>(out + o) = y;
        *reinterpret_cast<uvec *>(arg + o) = a;
      } else {
        for (int j = 0; j < nv; ++j) {
          out[o + j] = best[j];
          arg[o + j] = bestE[j];
        }
      }
    }
  }
}

/* The row passes around k_gather_reduce, one wave per vertex.  Before it
 * (DECODE = false): a vertex with no edges gets out = 0 and arg =
 * NTS_NO_EDGE, a split one (degree > split, as in k_build_items) gets its key
 * row zeroed — key 0 is below every real key.  After it (DECODE = true): the
 * split vertices' key rows are decoded into out and arg. */
template <bool DECODE, bool IS_MIN>
__global__ void k_reduce_rows(const uint32_t *__restrict__ offset,
                              uint32_t batch, uint32_t split,
                              float *__restrict__ out,
                              uint32_t *__restrict__ arg,
                              unsigned long long *__restrict__ keys,
                              uint32_t f) {
  const WaveId w = wave_id();
  for (uint32_t v = w.wave; v < batch; v += w.n_waves) {
    const uint32_t deg = offset[v + 1] - offset[v];
    const uint64_t o = (uint64_t)v * f;
    if (DECODE) {
      if (deg <= split) continue;
      for (uint32_t c = w.lane; c < f; c += 64)
        reduce_unkey<IS_MIN>(keys[o + c], out[o + c], arg[o + c]);
    } else if (!deg) {
      for (uint32_t c = w.lane; c < f; c += 64) {
        out[o + c] = 0.f;
        arg[o + c] = NTS_NO_EDGE;
      }
    } else if (keys && deg > split) {
      for (uint32_t c = w.lane; c < f; c += 64) keys[o + c] = 0ull;
    }
  }
}

/* backward of the max / min gather: one lane per (d, c) element scatters its
 * gradient to the source row its arg names (idx == NULL: row arg itself) */
__global__ void k_reduce_backward(const float *__restrict__ grad_out,
                                  const uint32_t *__restrict__ arg,
                                  const uint32_t *__restrict__ idx,
                                  uint32_t idx_start, float *grad_in,
                                  uint64_t n, uint32_t f) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint32_t a = arg[i];
    if (a == NTS_NO_EDGE) continue;
    const uint32_t row = idx ? idx[a] - idx_start : a;
    atomicAdd(&grad_in[(uint64_t)row * f + i % f], grad_out[i]);
  }
}

/* Fused CSR gather + per-edge dot (GAT backward): while the
 * backward gather streams grad_y[dst(e)] row slabs to accumulate
 * grad_h[src] = sum_e s[e]*grad_y[dst(e)], the SAME row bytes also feed
 * gs[e] = dot(grad_y[dst(e)], h[src]) — the attention-scalar gradient the
 * separate k_edge_dot kernel re-reads ~E*f floats to compute (9 ms of the
 * 34 ms round-1 GAT step at Reddit scale).  h[src] is loaded once per
 * (item, lane) into registers.  The per-edge dot is reduced across the lane
 * group through LDS: lanes stash their per-edge partials for a batch of
 * NTS_DOT_B edges into padded LDS, then NTS_DOT_B lanes each sum one edge's
 * G partials with conflict-free stride-(G+1) reads — ~2 LDS ops per lane
 * per edge and the reads pipeline, where a log2(G)-step shuffle chain per
 * edge pays ds_permute latency on every edge (3.1 ms/step slower, DESIGN
 * section 3).  The sum goes to dot_pos[e] (the CSR->CSC slot map, so the
 * softmax backward consumes it without a permute pass).
 * Clean-case kernel: f % ELEM == 0 and f <= G*ELEM (one slab) — the
 * launcher falls back to the unfused pair otherwise. */
constexpr uint32_t NTS_DOT_B = 16; /* edges per LDS transpose batch */

template <int ELEM>
__global__ __launch_bounds__(NTS_BLOCK) void k_gather_spmm_dot_lds(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    const uint32_t *__restrict__ nbr, const float *__restrict__ ew,
    const float *__restrict__ in, float *__restrict__ out, uint32_t nbr_start,
    const float *__restrict__ dot_vec, float *__restrict__ dot_out,
    const uint32_t *__restrict__ dot_pos, uint32_t f, uint32_t G) {
  /* per-group LDS: NTS_DOT_B rows of (G+1) floats (pad kills bank
   * conflicts); groups tile the block back to back.  Sized for the worst
   * case G=16 (most groups per block: 16 x 16x17 floats). */
  __shared__ float lds[NTS_DOT_B * (16 + 1) * (NTS_BLOCK / 16)];
  const uint32_t n_items = *n_items_p;
  const uint32_t tid = blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t glane = threadIdx.x & (G - 1);
  const uint32_t n_groups = (gridDim.x * blockDim.x) / G;
  float *gl = lds + (threadIdx.x / G) * NTS_DOT_B * (G + 1);
  for (uint32_t it = tid / G; it < n_items; it += n_groups) {
    const Item im = load_item(items, it);
    const uint32_t v = im.v, e0 = im.e0, cnt = im.cnt;
    const uint32_t off = glane * ELEM;
    const bool act = off + ELEM <= f; /* f%ELEM==0: lane is full or idle */
    float acc[ELEM] = {};
    float hreg[ELEM] = {};
    if (act) {
      const float *hp = dot_vec + (uint64_t)v * f + off;
#pragma unroll
      for (int j = 0; j < ELEM; ++j) hreg[j] = hp[j];
    }
    for (uint32_t b = 0; b < cnt; b += NTS_DOT_B) {
      const uint32_t nb = min(NTS_DOT_B, cnt - b);
      uint32_t k = 0;
      for (; k + 4 <= nb; k += 4) {
        const uint32_t e = e0 + b + k;
        float dp[4] = {};
        if (act) {
          const float *p[4];
          float wv[4];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            p[q] = in + (uint64_t)(nbr[e + q] - nbr_start) * f + off;
            wv[q] = ew[e + q];
          }
#pragma unroll
          for (int q = 0; q < 4; ++q) {
#pragma unroll
            for (int j = 0; j < ELEM; ++j) {
              const float x = p[q][j];
              acc[j] = fmaf(wv[q], x, acc[j]);
              dp[q] = fmaf(hreg[j], x, dp[q]);
            }
          }
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) gl[(k + q) * (G + 1) + glane] = dp[q];
      }
      for (; k < nb; ++k) {
        const uint32_t e = e0 + b + k;
        float dp = 0.f;
        if (act) {
          const float w = ew[e];
          const float *p = in + (uint64_t)(nbr[e] - nbr_start) * f + off;
#pragma unroll
          for (int j = 0; j < ELEM; ++j) {
            const float x = p[j];
            acc[j] = fmaf(w, x, acc[j]);
            dp = fmaf(hreg[j], x, dp);
          }
        }
        gl[k * (G + 1) + glane] = dp;
      }
      __builtin_amdgcn_wave_barrier(); /* group lives in one wave (G<=64) */
      if (glane < nb) {
        float sum = 0.f;
        const float *row = gl + glane * (G + 1);
        for (uint32_t j = 0; j < G; ++j) sum += row[j];
        const uint32_t e = e0 + b + glane;
        dot_out[dot_pos ? dot_pos[e] : e] = sum;
      }
      __builtin_amdgcn_wave_barrier();
    }
    if (act) store_acc<ELEM>(out + (uint64_t)v * f + off, acc, ELEM, im.shared);
  }
}

/* ---- GPU-resident fan-out sampling ----
 * One wave per destination.  Contract of Sampler::reservoir_sample
 * (ntsSampler.hpp:113-166): min(deg, fanout) uniformly chosen in-edge
 * slots per destination.  Realized wave-parallel as "the fanout smallest
 * per-edge-slot hash keys" (identical distribution to a reservoir walk,
 * same scheme as the host sampler's random keys, deterministic in
 * (seed, edge slot)); a lane-0 sequential reservoir would serialize
 * power-law hubs (measured 133 ms/step on layer-2 batches). */
__device__ __forceinline__ uint32_t k_hash_u32(unsigned long long seed,
                                               uint32_t d, uint32_t j) {
  unsigned long long z = seed ^ ((unsigned long long)d << 32) ^ j;
  z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdULL;
  z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ULL;
  return (uint32_t)(z ^ (z >> 33));
}

constexpr uint32_t NTS_MAX_FANOUT = 1024;

/* Selection: out[pick] = src[slot] for the k smallest (key, slot) of the m
 * candidates one wave holds in LDS, smallest first.  The slot in the low
 * bits makes tie-breaks deterministic in the edge slot.  A taken candidate
 * is overwritten with all-ones, so it reads as ~0ULL and a genuine max-key
 * candidate can never be shadowed. */
__device__ __forceinline__ void select_smallest(
    uint32_t *s_key, uint32_t *s_slot, uint32_t m, uint32_t k, uint32_t lane,
    uint32_t *__restrict__ out, const uint32_t *__restrict__ src) {
  for (uint32_t pick = 0; pick < k; ++pick) {
    unsigned long long best = ~0ULL;
    uint32_t bp = 0;
    for (uint32_t p = lane; p < m; p += 64) {
      const unsigned long long cand =
          ((unsigned long long)s_key[p] << 32) | s_slot[p];
      if (cand < best) { best = cand; bp = p; }
    }
    wave_min(best, bp);
    if (lane == 0) {
      out[pick] = src[s_slot[bp]];
      s_key[bp] = 0xFFFFFFFFu;
      s_slot[bp] = 0xFFFFFFFFu;
    }
    __builtin_amdgcn_wave_barrier();
  }
}

template <bool FORCE_FALLBACK /* test hook: skip the 32-bit search */>
__global__ void k_sample_reservoir(const uint32_t *__restrict__ column_offset,
                                   const uint32_t *__restrict__ row_indices,
                                   const uint32_t *__restrict__ dst_list,
                                   uint32_t n_dst, uint32_t fanout,
                                   unsigned long long seed,
                                   uint32_t *__restrict__ out_src,
                                   uint32_t *__restrict__ out_cnt) {
  /* survivors of the key-threshold filter: (key, slot) pairs per wave */
  constexpr uint32_t CAP = 1024;
  __shared__ uint32_t s_key[4][CAP];
  __shared__ uint32_t s_slot[4][CAP];
  const uint32_t wib = threadIdx.x >> 6;
  const WaveId w = wave_id();
  const uint32_t lane = w.lane;
  for (uint32_t i = w.wave; i < n_dst; i += w.n_waves) {
    const uint32_t d = dst_list[i];
    const uint32_t e0 = column_offset[d];
    const uint32_t deg = column_offset[d + 1] - e0;
    const uint32_t k = deg < fanout ? deg : fanout;
    if (deg <= fanout) {
      for (uint32_t j = lane; j < k; j += 64)
        out_src[(uint64_t)i * fanout + j] = row_indices[e0 + j];
      if (lane == 0) out_cnt[i] = k;
      continue;
    }
    /* uniform subset = the `fanout` smallest per-edge-slot hash keys (the
     * same scheme as the host sampler's random keys).  Wave-parallel:
     * binary-search a threshold whose survivor count lands in
     * [fanout, CAP], collect survivors to LDS, then select the fanout
     * smallest among them. */
    const uint32_t cap = CAP < 4 * fanout ? CAP : 4 * fanout;
    if (deg > CAP && fanout <= 64 && !FORCE_FALLBACK) {
      /* HUB destinations: any scan-based scheme is O(deg) on ONE wave —
       * the layer-2 frontier is degree-biased and its biggest hub
       * (in-degree ~814k at Reddit scale) serialized the whole launch
       * (~3 ms measured, profiles/round2).  Same contract ("min(deg,
       * fanout) uniformly chosen slots", ntsSampler.hpp:113-166 — whose
       * own reservoir uses rand_r()%i), delivered in O(fanout):
       * rejection sampling without replacement, slot_p = hash(seed, d,
       * pick | attempt<<10) % deg; duplicates against earlier picks
       * re-roll.  Deterministic in (seed, dst, pick): no scan, no
       * atomic order, bias <= deg/2^32 (way under the reference's
       * rand()%i bias). */
      const bool active = lane < fanout;
      uint32_t attempt = 0;
      uint32_t slot = active
          ? k_hash_u32(seed, d, lane | (attempt << 10)) % deg : 0xFFFFFFFFu;
      for (int round = 0; round < 100; ++round) {
        s_slot[wib][lane] = slot;
        __builtin_amdgcn_wave_barrier();
        bool dup = false;
        if (active) {
          for (uint32_t q = 0; q < lane; ++q)
            if (s_slot[wib][q] == slot) { dup = true; break; }
        }
        __builtin_amdgcn_wave_barrier();
        if (__ballot(dup) == 0) break;
        if (dup) {
          ++attempt;
          slot = k_hash_u32(seed, d, lane | (attempt << 10)) % deg;
        }
      }
      if (active) out_src[(uint64_t)i * fanout + lane] = row_indices[e0 + slot];
      if (lane == 0) out_cnt[i] = fanout;
      continue;
    }
    if (deg <= CAP && !FORCE_FALLBACK) {
      /* every candidate fits the collection buffer: skip the threshold
       * search entirely and store DIRECTLY at the slot index — no LDS
       * counter (a single atomicAdd counter serialized all 64 lanes and
       * was the kernel's hot spot: 65 % of the sampled-step GPU time,
       * profiles/round2) */
      for (uint32_t j = lane; j < deg; j += 64) {
        s_key[wib][j] = k_hash_u32(seed, 0, e0 + j);
        s_slot[wib][j] = j;
      }
      __builtin_amdgcn_wave_barrier();
      select_smallest(s_key[wib], s_slot[wib], deg, k, lane,
                      out_src + (uint64_t)i * fanout, row_indices + e0);
      if (lane == 0) out_cnt[i] = k;
      continue;
    }
    unsigned long long lo = 0, hi = 0x100000000ULL;
    unsigned long long T =
        (unsigned long long)(2.0 * fanout / deg * 4294967296.0) + 1;
    bool landed = false;
    for (int it = 0; it < 36 && !landed && !FORCE_FALLBACK; ++it) {
      uint32_t cnt = 0;
      for (uint32_t j = lane; j < deg; j += 64)
        cnt += (k_hash_u32(seed, 0, e0 + j) < T) ? 1u : 0u;
      cnt = wave_sum(cnt);
      if (cnt >= fanout && cnt <= cap) landed = true;
      else if (cnt < fanout) { lo = T; T = (T + hi + 1) / 2; }
      else { hi = T; T = (lo + T) / 2; }
    }
    unsigned long long T64 = 0;
    if (landed) {
      /* (key,slot) candidates below T<<32 == keys below T.  T can exceed
       * 2^32 when deg < 2*fanout (the initial threshold over-covers and
       * lands immediately): clamp to all-ones instead of overflowing the
       * shift to zero (which collected nothing and read garbage slots). */
      T64 = (T >= 0x100000000ULL) ? ~0ULL : (T << 32);
    } else {
      /* Massive key ties: the 32-bit survivor count jumps over the
       * [fanout, cap] window.  Search the 64-bit candidate (key<<32)|slot
       * instead — slots are unique within the column, so candidates are
       * all distinct, the count is unit-step monotone in the threshold,
       * and the bisection ALWAYS lands.  Deterministic in (seed, slot):
       * no atomic-order dependence, no truncation (round-1 fallback
       * collected in atomic race order and capped — VERDICT/ADVICE r01). */
      unsigned long long lo64 = 0, hi64 = ~0ULL;
      T64 = 0x8000000000000000ULL;
      for (int it = 0; it < 70; ++it) {
        uint32_t cnt = 0;
        for (uint32_t j = lane; j < deg; j += 64) {
          const unsigned long long cand =
              ((unsigned long long)k_hash_u32(seed, 0, e0 + j) << 32) | j;
          cnt += (cand < T64) ? 1u : 0u;
        }
        cnt = wave_sum(cnt);
        if (cnt >= fanout && cnt <= cap) break;
        if (cnt < fanout) { lo64 = T64; T64 = T64 + (hi64 - T64) / 2 + 1; }
        else { hi64 = T64; T64 = lo64 + (T64 - lo64) / 2; }
      }
    }
    /* ballot-compacted collection: survivors land slot-ordered with no
     * LDS atomics (the old per-lane atomicAdd counter serialized the
     * wave; placement is now also deterministic by construction) */
    uint32_t base = 0;
    for (uint32_t j0 = 0; j0 < deg; j0 += 64) {
      const uint32_t j = j0 + lane;
      bool pred = false;
      uint32_t key = 0;
      if (j < deg) {
        key = k_hash_u32(seed, 0, e0 + j);
        pred = (((unsigned long long)key << 32) | j) < T64;
      }
      const unsigned long long bmask = __ballot(pred);
      if (pred) {
        const uint32_t p =
            base + (uint32_t)__popcll(bmask & ((1ULL << lane) - 1));
        if (p < CAP) { s_key[wib][p] = key; s_slot[wib][p] = j; }
      }
      base += (uint32_t)__popcll(bmask);
    }
    __builtin_amdgcn_wave_barrier();
    select_smallest(s_key[wib], s_slot[wib], base < CAP ? base : CAP, k, lane,
                    out_src + (uint64_t)i * fanout, row_indices + e0);
    if (lane == 0) out_cnt[i] = k;
  }
}

/* message unpack: records [u32 vid | f x f32], stride f+1 floats */
__global__ void k_deserialize(const float *__restrict__ msg, uint32_t count,
                              uint32_t part_start, float *__restrict__ dense,
                              uint32_t f) {
  const uint64_t total = (uint64_t)count * f;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = i / f;
    const uint32_t r = (uint32_t)(i - k * f);
    const float *rec = msg + k * (f + 1);
    uint32_t vid = *reinterpret_cast<const uint32_t *>(rec);
    dense[(uint64_t)(vid - part_start) * f + r] = rec[1 + r];
  }
}

/* partial-sum merge: master[vid-part_start,:] += rec[1:] */
__global__ void k_agg_msg(float *__restrict__ master,
                          const float *__restrict__ msg, uint32_t count,
                          uint32_t part_start, uint32_t f) {
  const uint64_t total = (uint64_t)count * f;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = i / f;
    const uint32_t r = (uint32_t)(i - k * f);
    const float *rec = msg + k * (f + 1);
    uint32_t vid = *reinterpret_cast<const uint32_t *>(rec);
    atomicAdd(&master[(uint64_t)(vid - part_start) * f + r], rec[1 + r]);
  }
}

/* gather-permute: out[i] = in[index[i]] (f32, u32 indices) — carries
 * per-edge values between CSC and CSR edge order without torch's int64
 * index machinery */
__global__ void k_permute_f32(float *__restrict__ out,
                              const float *__restrict__ in,
                              const uint32_t *__restrict__ index,
                              uint64_t n) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    out[i] = in[index[i]];
}

/* dense-row pack/unpack for the RCCL ring (indices static, payload dense) */
enum RowOp { ROW_GATHER, ROW_SCATTER, ROW_SCATTER_ADD };
template <RowOp OP>
__global__ void k_rows(float *__restrict__ dense, float *__restrict__ packed,
                       const uint32_t *__restrict__ index, uint32_t count,
                       uint32_t row_start, uint32_t f) {
  const uint64_t total = (uint64_t)count * f;
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < total;
       i += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t k = i / f;
    const uint32_t r = (uint32_t)(i - k * f);
    const uint64_t d = (uint64_t)(index[k] - row_start) * f + r;
    if (OP == ROW_GATHER) packed[i] = dense[d];
    else if (OP == ROW_SCATTER) dense[d] = packed[i];
    else atomicAdd(&dense[d], packed[i]);
  }
}

/* ---------------- edge-wise (GAT) kernels ---------------- */
/* All edge kernels are driven by the same bounded work items as the
 * gather (<= NTS_SPLIT edges of one destination per item): a wave-per-
 * destination scheme would serialize power-law hubs (a 1M-edge hub costs
 * one wave seconds).  Lanes stride the item's (edges x f) elements. */
enum EdgeOp { E_SCATTER_SRC, E_GATHER_SRC, E_SCATTER_DST, E_GATHER_DST,
              E_SCATTER_GRAD };
template <EdgeOp OP>
__global__ void k_edge_items(const uint4 *__restrict__ items,
                             const uint32_t *__restrict__ n_items_p,
                             float *__restrict__ message,
                             float *__restrict__ vertex_feat,
                             const uint32_t *__restrict__ row_indices,
                             const uint32_t *__restrict__ mirror_index,
                             uint32_t f) {
  const uint32_t n_items = *n_items_p;
  const WaveId w = wave_id();
  for (uint32_t it = w.wave; it < n_items; it += w.n_waves) {
    const Item im = load_item(items, it);
    const uint32_t d = im.v, e0 = im.e0;
    const uint64_t nel = (uint64_t)im.cnt * f;
    for (uint64_t i = w.lane; i < nel; i += 64) {
      const uint32_t e = e0 + (uint32_t)(i / f);
      const uint32_t r = (uint32_t)(i % f);
      uint64_t vrow;
      if (OP == E_SCATTER_SRC || OP == E_GATHER_SRC)
        vrow = (uint64_t)mirror_index[row_indices[e]] * f + r;
      else
        vrow = (uint64_t)d * f + r;
      const uint64_t m = (uint64_t)e * f + r;
      if (OP == E_SCATTER_SRC || OP == E_SCATTER_DST) message[m] = vertex_feat[vrow];
      else if (OP == E_SCATTER_GRAD) atomicAdd(&message[m], vertex_feat[vrow]);
      else atomicAdd(&vertex_feat[vrow], message[m]);
    }
  }
}

/* t > 0 ? t : slope*t;  lrelu'(t) = t > 0 ? 1 : slope (slope at t == 0) */
__device__ __forceinline__ float lrelu(float t, float slope) {
  return t > 0.f ? t : slope * t;
}

/* ---- attention dropout: the keep decision of one (edge, head) ---- */
/* Position i = e*K + k, e the chunk-local CSC edge, as a 64-bit value; the
 * finalizer is k_hash_u32's.  keep = (fmix64(base + i) >> 40) >= T with
 * base = fmix64(seed) mixed once on the host (seeds s and s + 1 give no
 * shifted copies of one mask) and T = lrintf(p * 2^24): a position drops with
 * probability T / 2^24.  A function of (seed, e, k) alone, so every pass and
 * the host (nts_edge_dropout_keep) regenerate the mask and none stores it. */
__host__ __device__ inline unsigned long long drop_fmix64(
    unsigned long long z) {
  z = (z ^ (z >> 33)) * 0xff51afd7ed558ccdULL;
  z = (z ^ (z >> 33)) * 0xc4ceb9fe1a85ec53ULL;
  return z ^ (z >> 33);
}
struct DropMask {
  unsigned long long base; /* fmix64(seed) */
  uint32_t T;              /* keep iff the 24-bit draw >= T */
  float scale;             /* 1 / (1 - p) */
};
__host__ __device__ inline bool drop_keep(const DropMask &dm,
                                          unsigned long long i) {
  return (uint32_t)(drop_fmix64(dm.base + i) >> 40) >= dm.T;
}

/* ---- per-destination reductions over an item's [cnt, K] values ---- */
/* Per-edge values are [E, K] row-major, per-vertex ones [rows, K]: K is the
 * softmax's f, the attention's heads, 1 for one scalar per edge.  A wave
 * takes an item and reduces each of its K columns.  Every such pass is
 * k_edge_reduce over a lane layout, a value rule (what an edge's value is)
 * and a reduce rule (what is kept per value and left per column).
 *
 * Lane layouts.  Strided, any K: column by column, lanes stride the item's
 * edges, a 64-lane butterfly, lane 0 owns column k.  FLAT, K a power of two
 * <= 64: lanes stride the item's cnt*K values in memory order (coalesced);
 * 64 % K == 0, so a lane stays on column lane % K, the butterfly steps
 * xor 32..K leave column k's result on lanes == k mod K, and lanes < K own
 * column `lane`.  At one column the two are the same walk (lanes stride the
 * edges, xor 32..1, lane 0 owns); it runs as the strided one at a
 * compile-time K of 1 (KC), whose column loop and K-scaled indices fold
 * away and whose edge counter is 32-bit — the registers of a hand-written
 * scalar kernel (FLAT at K = 1 costs 5 to 8 VGPRs more for its 64-bit
 * counter).
 *
 * The strided butterfly is the FLAT one at a span of 1: xor 32..1. */
__device__ __forceinline__ float heads_lane_sum(float x, uint32_t K) {
  for (uint32_t w = 32; w >= K; w >>= 1) x += __shfl_xor(x, w, 64);
  return x;
}
__device__ __forceinline__ float heads_lane_max(float x, uint32_t K) {
  for (uint32_t w = 32; w >= K; w >>= 1) x = fmaxf(x, __shfl_xor(x, w, 64));
  return x;
}

/* val.column(slot) once per (item, column), slot = v*K + k; val(e, K, k, m)
 * per value, m = e*K + k; red.add per value; red.put(acc, span, owner, slot,
 * shared) per column, span the butterfly's last step */
template <bool FLAT, int KC, class Value, class Reduce>
__device__ __forceinline__ void reduce_item(const WaveId &w, const Item &im,
                                            uint32_t K_run, Value &val,
                                            const Reduce &red) {
  const uint32_t K = KC ? (uint32_t)KC : K_run;
  const uint64_t slot0 = (uint64_t)im.v * K;
  if constexpr (FLAT) {
    const uint32_t k = w.lane & (K - 1);
    const uint32_t lgk = 31u - (uint32_t)__clz(K);
    const uint64_t m0 = (uint64_t)im.e0 * K;
    const uint64_t nel = (uint64_t)im.cnt * K;
    val.column(slot0 + k);
    typename Reduce::Acc acc = Reduce::empty();
    for (uint64_t i = w.lane; i < nel; i += 64)
      red.add(acc, val(im.e0 + (uint32_t)(i >> lgk), K, k, m0 + i), m0 + i,
              im.shared);
    red.put(acc, K, w.lane < K, slot0 + w.lane, im.shared);
  } else {
    for (uint32_t k = 0; k < K; ++k) {
      val.column(slot0 + k);
      typename Reduce::Acc acc = Reduce::empty();
      for (uint32_t j = w.lane; j < im.cnt; j += 64) {
        const uint32_t e = im.e0 + j;
        const uint64_t m = (uint64_t)e * K + k;
        red.add(acc, val(e, K, k, m), m, im.shared);
      }
      red.put(acc, 1u, w.lane == 0, slot0 + k, im.shared);
    }
  }
}

/* ---- value rules ---- */
/* in[m]: a softmax score, or a weight to sum */
struct EdgeIn {
  const float *__restrict__ in;
  __device__ void column(uint64_t) {}
  __device__ float operator()(uint32_t, uint32_t, uint32_t, uint64_t m) const {
    return in[m];
  }
};
/* softmax backward: g * s */
struct EdgeInCached {
  const float *__restrict__ in, *__restrict__ cached;
  __device__ void column(uint64_t) {}
  __device__ float operator()(uint32_t, uint32_t, uint32_t, uint64_t m) const {
    return in[m] * cached[m];
  }
};
/* softmax backward under attention dropout: in is the gradient of the
 * dropped weights w = keep ? s * scale : 0, so the gradient of s is
 * in * (keep ? scale : 0), the mask regenerated from m (never loaded).
 * Both loads stand before the hash: its two 64-bit multiplies (four 32-bit
 * multiplies each, quarter rate) run under the loads' latency. */
struct EdgeInCachedDrop {
  const float *__restrict__ in, *__restrict__ cached;
  DropMask dm;
  __device__ void column(uint64_t) {}
  __device__ float operator()(uint32_t, uint32_t, uint32_t, uint64_t m) const {
    const float g = in[m], c = cached[m];
    return g * (drop_keep(dm, m) ? dm.scale : 0.f) * c;
  }
};
/* Fused GAT attention score: per edge and head
 *   t = s_src[mirror_index[src], k] + s_dst[dst, k],
 * stashes t (the leaky-relu input the backward mask needs) and applies the
 * activation — replacing the separate scatter_src_mirror_to_msg +
 * scatter_dst_to_msg kernels and the torch add/leaky elementwise passes (5
 * full E-sized passes, with the exp and the sums of the reduce rule) by one. */
struct EdgeScore {
  float *__restrict__ m_sum_out;
  const float *__restrict__ s_src, *__restrict__ s_dst;
  const uint32_t *__restrict__ row_indices, *__restrict__ mirror_index;
  float slope;
  float sd;
  __device__ void column(uint64_t slot) { sd = s_dst[slot]; }
  __device__ float operator()(uint32_t e, uint32_t K, uint32_t k,
                              uint64_t m) const {
    const uint32_t src = row_indices[e];
    const uint64_t row = mirror_index ? mirror_index[src] : src;
    const float t = s_src[row * K + k] + sd;
    m_sum_out[m] = t;
    return lrelu(t, slope);
  }
};

/* ---------------- stable (max-subtracted) edge softmax ---------------- */
/* nts_edge_softmax_stable: the same two item-driven passes over the same
 * bytes as the default.  Pass 1 stashes the activation a (not exp a) in out
 * and leaves, per (destination, column or head), the pair (M, S) = (max a,
 * sum exp(a - M)) in a stream-owned scratch; pass 2 writes exp(a - M) / S.
 *
 * A pair is one 64-bit word: reduce_key's ordered-uint map of M in the low
 * half, S in the high half; the all-zero word of the memset is below every
 * real key and is a sum of 0.
 * An unsplit destination (one item): a lane keeps a running pair over the
 * values it strides (one exp per value, nothing re-read at any NTS_SPLIT or
 * K); M is a butterfly max, every lane rescales its sum to M once, S is the
 * butterfly sum, and the pair is stored with a plain store, no atomic.
 * A split destination: its items reduce their maxima in pass 1 and merge
 * them with a u32 atomicMax on the key; the split-sum pass, which skips
 * every unsplit item, then re-reads the split items' stash and adds
 * sum exp(a - M) with the default's fp32 atomicAdd.  (A 64-bit
 * compare-and-swap merge of whole pairs in pass 1 was measured and removed:
 * DESIGN section 3.)  A score of -inf adds nothing anywhere, and an item of
 * nothing but -inf leaves the slot alone (no exp(-inf + inf)). */
struct MaxSum { float m, s; }; /* s = sum of exp(a - m); (-inf, 0) = nothing */

__device__ __forceinline__ void ms_add(MaxSum &p, float a) {
  if (a > p.m) {
    p.s = p.s * __expf(p.m - a) + 1.f; /* first value: 0 * exp(-inf) + 1 */
    p.m = a;
  } else if (a > -INFINITY) {
    p.s += __expf(a - p.m);
  }
}
/* a lane's sum rescaled to the item's maximum (0 from a lane or an item that
 * saw nothing but -inf) */
__device__ __forceinline__ float ms_rescaled(const MaxSum &p, float Mi) {
  return (p.m > -INFINITY) ? p.s * __expf(p.m - Mi) : 0.f;
}

/* reduce_key's monotone float -> uint map (never 0 for a non-NaN) */
__device__ __forceinline__ uint32_t ms_key(float x) {
  const uint32_t u = __float_as_uint(x);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float ms_unkey(uint32_t u) {
  return __uint_as_float((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
__device__ __forceinline__ unsigned long long ms_pack(float M, float S) {
  return ((unsigned long long)__float_as_uint(S) << 32) | ms_key(M);
}
__device__ __forceinline__ MaxSum ms_unpack(unsigned long long x) {
  return MaxSum{ms_unkey((uint32_t)x), __uint_as_float((uint32_t)(x >> 32))};
}

/* a value into a lane's pair; an item of a split destination needs the
 * maximum only (its sum is the split-sum pass's) */
__device__ __forceinline__ void ms_add(MaxSum &p, float a, bool maxonly) {
  if (maxonly) p.m = fmaxf(p.m, a);
  else ms_add(p, a);
}

/* one item's result into its destination's slot: the whole pair of an
 * unsplit destination, the maximum of a split one's item */
__device__ __forceinline__ void ms_put(unsigned long long *slot, float Mi,
                                       float Si, bool shared) {
  if (!(Mi > -INFINITY)) return;
  if (shared) atomicMax(reinterpret_cast<uint32_t *>(slot), ms_key(Mi));
  else *slot = ms_pack(Mi, Si);
}

/* the split-sum pass's value: exp(stash - M), M the destination's merged
 * maximum */
struct EdgeStashExp {
  const float *out;
  const unsigned long long *pairs;
  float M;
  __device__ void column(uint64_t slot) { M = ms_unkey((uint32_t)pairs[slot]); }
  __device__ float operator()(uint32_t, uint32_t, uint32_t, uint64_t m) const {
    return __expf(out[m] - M);
  }
};

/* ---- reduce rules ---- */
/* Default softmax pass 1: stash v = exp(a) (forward) or a (backward) in out
 * for pass 2, item-partial sums reduced once into sums[slot] by fp32
 * atomics.  No max subtraction: reference semantics,
 * ntsCUDADistKernel.cuh:192. */
template <bool EXP>
struct SumToSums {
  float *__restrict__ out, *__restrict__ sums;
  using Acc = float;
  __device__ static Acc empty() { return 0.f; }
  __device__ static bool wants(const Item &) { return true; }
  __device__ void add(Acc &part, float a, uint64_t m, bool) const {
    const float v = EXP ? __expf(a) : a;
    out[m] = v;
    part += v;
  }
  __device__ void put(Acc part, uint32_t span, bool owner, uint64_t slot,
                      bool) const {
    part = heads_lane_sum(part, span);
    if (owner) atomicAdd(&sums[slot], part);
  }
};
/* stable pass 1: stash a, leave the (M, S) pair (the maximum alone from an
 * item of a split destination) */
struct MaxSumToPairs {
  float *__restrict__ out;
  unsigned long long *__restrict__ pairs;
  using Acc = MaxSum;
  __device__ static Acc empty() { return MaxSum{-INFINITY, 0.f}; }
  __device__ static bool wants(const Item &) { return true; }
  __device__ void add(Acc &p, float a, uint64_t m, bool shared) const {
    out[m] = a;
    ms_add(p, a, shared);
  }
  __device__ void put(const Acc &p, uint32_t span, bool owner, uint64_t slot,
                      bool shared) const {
    const float Mi = heads_lane_max(p.m, span);
    const float Si = heads_lane_sum(ms_rescaled(p, Mi), span);
    if (owner) ms_put(&pairs[slot], Mi, Si, shared);
  }
};
/* between the stable passes: a split destination's items add their sums to
 * its S */
struct SplitSumToPairs {
  unsigned long long *pairs;
  using Acc = float;
  __device__ static Acc empty() { return 0.f; }
  __device__ static bool wants(const Item &im) { return im.shared; }
  __device__ void add(Acc &part, float v, uint64_t, bool) const { part += v; }
  __device__ void put(Acc part, uint32_t span, bool owner, uint64_t slot,
                      bool) const {
    part = heads_lane_sum(part, span);
    if (owner && part > 0.f)
      atomicAdd(reinterpret_cast<float *>(&pairs[slot]) + 1, part);
  }
};
/* out[v*K + k] += the column's sum.  With EdgeIn this is the per-vertex sum
 * of per-edge weights — the f=1 "aggregate an all-ones input with weights w"
 * reduction (GAT's attention-scalar source gradient) done natively: lanes
 * stride the item's edges and wave-reduce, instead of the f-wide gather
 * kernel where 15/16 lanes idle at f=1 (measured 1.9 ms -> this shape
 * streams w + offsets only).  Hub items merge by fp32 atomics like the
 * gather. */
struct SumToOut {
  float *__restrict__ out;
  using Acc = float;
  __device__ static Acc empty() { return 0.f; }
  __device__ static bool wants(const Item &) { return true; }
  __device__ void add(Acc &part, float v, uint64_t, bool) const { part += v; }
  __device__ void put(Acc part, uint32_t span, bool owner, uint64_t slot,
                      bool shared) const {
    part = heads_lane_sum(part, span);
    if (owner) {
      if (shared) atomicAdd(&out[slot], part);
      else out[slot] += part;
    }
  }
};

template <bool FLAT, int KC, class Value, class Reduce>
__global__ void k_edge_reduce(const uint4 *__restrict__ items,
                              const uint32_t *__restrict__ n_items_p,
                              Value val, const Reduce red, uint32_t K) {
  const uint32_t n_items = *n_items_p;
  const WaveId w = wave_id();
  for (uint32_t it = w.wave; it < n_items; it += w.n_waves) {
    const Item im = load_item(items, it);
    if (!Reduce::wants(im)) continue;
    reduce_item<FLAT, KC>(w, im, K, val, red);
  }
}

/* ---- fused GAT inference forward: no per-edge state ---- */
/* GAT's score is a function of two per-vertex scalars, so a forward that
 * needs only y keeps nothing per edge.  Pass 1 is k_edge_reduce under the
 * rules below — the training rules minus their per-edge stores — and leaves
 * the per-(destination, head) sums, or (M, S) pairs, where the softmax leaves
 * them; pass 2, k_gather_att_heads, recomputes each edge's weight in
 * registers.  An unsplit destination's denominator is reduced in the order
 * of the training pass 1, and a weight is the expression the normalize pass
 * evaluates on the stash, so both have the training forward's bits. */

/* EdgeScore without the m_sum stash */
struct EdgeScoreOnly {
  const float *__restrict__ s_src, *__restrict__ s_dst;
  const uint32_t *__restrict__ row_indices, *__restrict__ mirror_index;
  float slope;
  float sd;
  __device__ void column(uint64_t slot) { sd = s_dst[slot]; }
  __device__ float operator()(uint32_t e, uint32_t K, uint32_t k,
                              uint64_t) const {
    const uint32_t src = row_indices[e];
    const uint64_t row = mirror_index ? mirror_index[src] : src;
    return lrelu(s_src[row * K + k] + sd, slope);
  }
};
/* EdgeStashExp without the stash: the split-sum pass recomputes the
 * activation from the scalars */
struct EdgeScoreExp {
  EdgeScoreOnly score;
  const unsigned long long *pairs;
  float M;
  __device__ void column(uint64_t slot) {
    score.column(slot);
    M = ms_unkey((uint32_t)pairs[slot]);
  }
  __device__ float operator()(uint32_t e, uint32_t K, uint32_t k,
                              uint64_t m) const {
    const float a = score(e, K, k, m);
    return __expf(a - M);
  }
};
/* SumToSums<true> without the exp stash */
struct ExpSumToSums {
  float *__restrict__ sums;
  using Acc = float;
  __device__ static Acc empty() { return 0.f; }
  __device__ static bool wants(const Item &) { return true; }
  __device__ void add(Acc &part, float a, uint64_t, bool) const {
    part += __expf(a);
  }
  __device__ void put(Acc part, uint32_t span, bool owner, uint64_t slot,
                      bool) const {
    part = heads_lane_sum(part, span);
    if (owner) atomicAdd(&sums[slot], part);
  }
};
/* MaxSumToPairs without the activation stash */
struct MaxSumOnlyToPairs {
  unsigned long long *__restrict__ pairs;
  using Acc = MaxSum;
  __device__ static Acc empty() { return MaxSum{-INFINITY, 0.f}; }
  __device__ static bool wants(const Item &) { return true; }
  __device__ void add(Acc &p, float a, uint64_t, bool shared) const {
    ms_add(p, a, shared);
  }
  __device__ void put(const Acc &p, uint32_t span, bool owner, uint64_t slot,
                      bool shared) const {
    const float Mi = heads_lane_max(p.m, span);
    const float Si = heads_lane_sum(ms_rescaled(p, Mi), span);
    if (owner) ms_put(&pairs[slot], Mi, Si, shared);
  }
};

/* what pass 2 reads in place of a weight array: the scalars and pass 1's
 * per-(destination, head) slots (float sums, or packed pairs when STABLE) */
struct AttSrc {
  const float *__restrict__ s_src, *__restrict__ s_dst;
  const uint32_t *__restrict__ mirror_index;
  const void *__restrict__ slots;
  float slope;
};
/* one (destination, head): loaded once per (item, lane) */
struct AttDen { float sd, M, S; };
template <bool STABLE>
__device__ __forceinline__ AttDen att_den(const AttSrc &at, uint64_t slot) {
  AttDen q;
  q.sd = at.s_dst[slot];
  if constexpr (STABLE) {
    const MaxSum p =
        ms_unpack(static_cast<const unsigned long long *>(at.slots)[slot]);
    q.M = p.m;
    q.S = p.s;
  } else {
    q.M = 0.f;
    q.S = static_cast<const float *>(at.slots)[slot];
  }
  return q;
}
/* the weight of an edge whose source scalar is ss: the normalize pass's
 * expression on the value pass 1 would have stashed.  A true division (a
 * reciprocal taken once per item rounds differently), and no contraction of
 * the activation's multiply into the subtraction: the stash was rounded. */
template <bool STABLE>
__device__ __forceinline__ float att_weight(float ss, const AttDen &q,
                                            float slope) {
#pragma clang fp contract(off)
  const float t = ss + q.sd;
  const float a = lrelu(t, slope);
  if constexpr (STABLE) return __expf(a - q.M) / q.S;
  else return __expf(a) / q.S;
}
/* MIRROR is a template parameter, not a test of the pointer in the edge loop:
 * tested per edge it compiles to a branch and a full wait around every index
 * load, and the four index loads of an unrolled step run one after the other
 * (read in the ISA, as for k_gather_reduce's message form) */
template <bool MIRROR>
__device__ __forceinline__ const float *att_src_row(const AttSrc &at,
                                                    uint32_t src, uint32_t K) {
  const uint64_t row = MIRROR ? at.mirror_index[src] : src;
  return at.s_src + row * K;
}

/* NE consecutive edges for a full vector lane: the NE source scalars are
 * loaded with the NE rows' addresses, before the first row load is consumed */
template <int ELEM, int NE, bool STABLE, bool MIRROR, typename T>
__device__ __forceinline__ void att_edges_vec(float (&acc)[ELEM],
                                              const GatherSrc<T> &g,
                                              const AttSrc &at, uint32_t e,
                                              uint32_t col, uint32_t K,
                                              uint32_t head,
                                              const AttDen &q) {
  const T *p[NE];
  float ss[NE], wv[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const uint32_t src = g.nbr[e + k];
    p[k] = g.in + (uint64_t)(src - g.nbr_start) * g.ld + col;
    ss[k] = att_src_row<MIRROR>(at, src, K)[head];
  }
#pragma unroll
  for (int k = 0; k < NE; ++k) wv[k] = att_weight<STABLE>(ss[k], q, at.slope);
  fma_vec<ELEM, NE>(acc, p, wv);
}
/* strided twin: element j at column col + j*G, head hd[j] with its own
 * (s_dst, M, S) in q[j], live while col + j*G < f */
template <int NSTR, int NE, bool STABLE, bool MIRROR, typename T>
__device__ __forceinline__ void att_edges_strided(
    float (&acc)[NSTR], const GatherSrc<T> &g, const AttSrc &at, uint32_t e,
    uint32_t col, uint32_t G, uint32_t K, const uint32_t (&hd)[NSTR],
    const AttDen (&q)[NSTR]) {
  const T *p[NE];
  const float *srow[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    const uint32_t src = g.nbr[e + k];
    p[k] = g.in + (uint64_t)(src - g.nbr_start) * g.ld + col;
    srow[k] = att_src_row<MIRROR>(at, src, K);
  }
#pragma unroll
  for (int k = 0; k < NE; ++k)
#pragma unroll
    for (int j = 0; j < NSTR; ++j)
      if (col + j * G < g.f)
        acc[j] = fmaf(att_weight<STABLE>(srow[k][hd[j]], q[j], at.slope),
                      to_f32(p[k][j * G]), acc[j]);
}

/* Pass 2: k_gather_spmm_heads<ELEM, T> with the weight computed, not loaded.
 * Same lane groups, tasks, 4-edge unroll, register accumulation and single
 * store; runs at K = 1 as well (C = f).  MIRROR: at.mirror_index is set. */
template <int ELEM, typename T, bool STABLE, bool MIRROR>
__global__ __launch_bounds__(NTS_BLOCK) void k_gather_att_heads(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    const uint32_t *__restrict__ nbr, const AttSrc at,
    const T *__restrict__ in, float *__restrict__ out, uint32_t nbr_start,
    uint32_t f, uint32_t G, uint32_t n_slabs, uint32_t K, uint32_t C) {
  constexpr int NSTR = (ELEM == 1) ? 4 : 1;
  const uint32_t n_items = *n_items_p;
  const uint32_t glane = threadIdx.x & (G - 1);
  const uint32_t tilef = G * ELEM * NSTR;
  const GatherSrc<T> g{nbr, nullptr, in, nbr_start, f, f};
  const GatherPlan pl{NTS_SCHED_ITEM, tilef, n_slabs, 1u};
  const XcdClass xc;
  const uint64_t total = (uint64_t)n_items * n_slabs;
  const uint64_t stride = (gridDim.x * NTS_BLOCK) / G;
  for (uint64_t t = (blockIdx.x * NTS_BLOCK + threadIdx.x) / G; t < total;
       t += stride) {
    const Task tk = decode_task<false>(pl, xc, t, n_items, f, tilef);
    const uint32_t col = tk.fbase + glane * ELEM;
    if (col >= f) continue;
    const Item im = load_item(items, tk.it);
    const uint32_t e_end = im.e0 + im.cnt;
    uint32_t e = im.e0;
    float acc[ELEM * NSTR] = {};
    float *o = out + (uint64_t)im.v * f + col;
    const uint64_t slot0 = (uint64_t)im.v * K;
    if constexpr (ELEM == 1) {
      uint32_t hd[NSTR];
      AttDen q[NSTR];
#pragma unroll
      for (int j = 0; j < NSTR; ++j) {
        hd[j] = (col + j * G < f) ? (col + j * G) / C : 0u;
        q[j] = att_den<STABLE>(at, slot0 + hd[j]);
      }
      for (; e + 4 <= e_end; e += 4)
        att_edges_strided<NSTR, 4, STABLE, MIRROR>(acc, g, at, e, col, G, K,
                                                   hd, q);
      for (; e < e_end; ++e)
        att_edges_strided<NSTR, 1, STABLE, MIRROR>(acc, g, at, e, col, G, K,
                                                   hd, q);
      store_strided(o, acc, G, col, f, im.shared);
    } else {
      const uint32_t head = col / C;
      const AttDen q = att_den<STABLE>(at, slot0 + head);
      for (; e + 4 <= e_end; e += 4)
        att_edges_vec<ELEM, 4, STABLE, MIRROR>(acc, g, at, e, col, K, head,
                                               q);
      for (; e < e_end; ++e)
        att_edges_vec<ELEM, 1, STABLE, MIRROR>(acc, g, at, e, col, K, head,
                                               q);
      store_acc<ELEM, common_ov(ELEM, (int)sizeof(T))>(o, acc, ELEM,
                                                       im.shared);
    }
  }
}

/* Normalize pass (pass 2 of the edge softmax):
 *   NORM_FWD     out = out / sum                 (out holds exp a)
 *   NORM_BWD     out = out - sum * cached        (out holds g * s)
 *   NORM_STABLE  out = exp(out - M) / S          (out holds a)
 * Optional extras (GAT fusions):
 *  - out2/pos2: ALSO write each value to out2[pos2[m]] — with pos2 = the
 *    CSC->CSR slot map this emits the result in CSR edge order in the same
 *    pass, replacing a separate nts_permute_f32 kernel (2x ~2 ms/step on
 *    the Reddit-scale GAT config).
 *  - lrelu_in/slope (NORM_BWD only): multiply by the leaky-relu derivative
 *    (lrelu_in[m] > 0 ? 1 : slope), fusing the attention activation's
 *    backward elementwise pass. */
enum NormMode { NORM_FWD, NORM_BWD, NORM_STABLE };
template <NormMode MODE>
using NormSlot =
    std::conditional_t<MODE == NORM_STABLE, unsigned long long, float>;

/* Attention dropout's emission rule for the forward modes: out keeps the
 * undropped softmax for the backward, and the dropped weight
 * w = keep ? v * scale : +0 goes to w_out[m] and, in place of v, to out2 —
 * one more [E, K] write in this pass instead of a mask tensor and an apply
 * pass.  The rule is an optional trailing argument (a pack that is empty or
 * one NormEmitDropped): without it the kernel has the arguments and the body
 * it had before the rule existed. */
struct NormEmitDropped {
  float *__restrict__ w_out;
  DropMask dm;
  __device__ float operator()(float v, uint64_t m) const {
    const float w = drop_keep(dm, m) ? v * dm.scale : 0.f;
    w_out[m] = w;
    return w;
  }
};

template <NormMode MODE, class... Emit>
__global__ void k_edge_softmax_norm(const uint4 *__restrict__ items,
                                    const uint32_t *__restrict__ n_items_p,
                                    float *__restrict__ out,
                                    const float *__restrict__ cached,
                                    const NormSlot<MODE> *__restrict__ slots,
                                    float *__restrict__ out2,
                                    const uint32_t *__restrict__ pos2,
                                    const float *__restrict__ lrelu_in,
                                    float slope,
                                    float *__restrict__ dst_accum,
                                    uint32_t f, const Emit... emit) {
  static_assert(sizeof...(Emit) <= 1, "at most one emission rule");
  const uint32_t n_items = *n_items_p;
  const WaveId w = wave_id();
  for (uint32_t it = w.wave; it < n_items; it += w.n_waves) {
    const Item im = load_item(items, it);
    const uint32_t d = im.v, e0 = im.e0;
    const uint64_t nel = (uint64_t)im.cnt * f;
    float gsum = 0.f; /* per-dst sum of the result (f==1 only) */
    for (uint64_t i = w.lane; i < nel; i += 64) {
      const uint32_t e = e0 + (uint32_t)(i / f);
      const uint32_t r = (uint32_t)(i % f);
      const uint64_t m = (uint64_t)e * f + r;
      const NormSlot<MODE> slot = slots[(uint64_t)d * f + r];
      float v;
      if constexpr (MODE == NORM_BWD) {
        v = out[m] - slot * cached[m];
        if (lrelu_in) v *= (lrelu_in[m] > 0.f) ? 1.f : slope;
      } else if constexpr (MODE == NORM_STABLE) {
        const MaxSum q = ms_unpack(slot);
        v = __expf(out[m] - q.m) / q.s;
      } else {
        v = out[m] / slot;
      }
      out[m] = v;
      float v2 = v;
      ((v2 = emit(v, m)), ...);
      if (out2) out2[(uint64_t)pos2[e] * f + r] = v2; /* pos2: per-edge map */
      if (dst_accum) gsum += v;
    }
    if (dst_accum) {
      /* the attention-scalar's per-destination reduction (gat.py g_dst),
       * emitted here instead of a separate f=1 gather pass; item-bounded,
       * so one fp32 atomic per (item, wave), hub-safe */
      gsum = wave_sum(gsum);
      if (w.lane == 0) atomicAdd(&dst_accum[d], gsum);
    }
  }
}

/* per-edge dot: out[e] = dot(dst_rows[d], src_rows[row_indices[e]-src_s]),
 * item-driven (bounded per-wave work even on power-law hubs); one wave per
 * edge, lanes stride the feature dim.  Measured against a lane-per-edge and
 * a sub-group (16/32 lanes per edge) form, both slower. */
__global__ void k_edge_dot(const uint4 *__restrict__ items,
                           const uint32_t *__restrict__ n_items_p,
                           float *__restrict__ out,
                           const float *__restrict__ dst_rows,
                           const float *__restrict__ src_rows,
                           const uint32_t *__restrict__ row_indices,
                           uint32_t src_start, uint32_t f) {
  const uint32_t n_items = *n_items_p;
  const WaveId w = wave_id();
  const uint32_t lane = w.lane;
  for (uint32_t it = w.wave; it < n_items; it += w.n_waves) {
    const Item im = load_item(items, it);
    const uint32_t e0 = im.e0, cnt = im.cnt;
    const float *a = dst_rows + (uint64_t)im.v * f;
    /* 4-edge unroll: four independent source-row loads in flight */
    uint32_t k = 0;
    for (; k + 4 <= cnt; k += 4) {
      const float *b[4];
#pragma unroll
      for (int q = 0; q < 4; ++q)
        b[q] = src_rows +
               (uint64_t)(row_indices[e0 + k + q] - src_start) * f;
      float sum[4] = {};
      for (uint32_t j = lane; j < f; j += 64) {
        const float av = a[j];
#pragma unroll
        for (int q = 0; q < 4; ++q) sum[q] = fmaf(av, b[q][j], sum[q]);
      }
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        sum[q] = wave_sum(sum[q]);
        if (lane == 0) out[e0 + k + q] = sum[q];
      }
    }
    for (; k < cnt; ++k) {
      const uint32_t e = e0 + k;
      const float *b = src_rows + (uint64_t)(row_indices[e] - src_start) * f;
      float sum = 0.f;
      for (uint32_t j = lane; j < f; j += 64) sum += a[j] * b[j];
      sum = wave_sum(sum);
      if (lane == 0) out[e] = sum;
    }
  }
}

/* ---- per-edge reductions over a row pair, K heads of C columns ---- */
/* out[e*K + k] = sum over head k's C columns j of term(own[d, j], nbr[src, j]).
 * The term is a rule struct: the per-head dot, or the GATv2 score, which
 * brings a third operand per column. */
template <int R, typename T>
__device__ __forceinline__ void load_cols(const T *p, float (&x)[R]) {
  if constexpr (R == 1) x[0] = to_f32(p[0]);
  else load_lane<R>(p, x);
}
/* a * b */
struct DotTerm {
  template <int R>
  __device__ void load(float (&x)[R], uint32_t) const {
#pragma unroll
    for (int j = 0; j < R; ++j) x[j] = 0.f; /* no third operand */
  }
  __device__ float operator()(float, float a, float b, float acc) const {
    return fmaf(a, b, acc);
  }
};
/* att[j] * lrelu(a + b): a + b is ONE fp32 add of the two loaded values */
struct Gatv2Term {
  const float *__restrict__ att;
  float slope;
  template <int R>
  __device__ void load(float (&x)[R], uint32_t col) const {
    load_cols<R>(att + col, x);
  }
  __device__ float operator()(float x, float a, float b, float acc) const {
    return fmaf(x, lrelu(a + b, slope), acc);
  }
};

/* The general form runs a wave per (edge, head): lanes stride the head's C
 * columns, wave_sum (64 - C lanes idle when C < 64).
 * k_edge_pair_seg, for C a power of two <= 64*R: a lane holds R consecutive
 * columns (one dwordxR load: 4, 2 or 1 by C and the pointers' alignment),
 * so a head is an aligned segment of L = C/R lanes and a row is G = f/R
 * lanes (at most 64 per step); 64/G edges share a wave.  The lane reduces
 * its R columns (the term's own operand is loaded once per (item, slab)
 * beside the own-row columns), a log2(L)-step butterfly sums each segment,
 * and the segment's first lane writes.  Lanes past the row's end and edge
 * slots past the item's end load a clamped (valid) address and are never
 * written: segments lie inside one head and one lane group, so what such
 * lanes hold never meets a live sum.
 * TD / TS = element types of dst_rows / src_rows (float, or uint16_t for
 * bfloat16 rows, widened exactly on load): a lane's R columns are then one
 * R*2-byte load (R = 1: a 2-byte load, any 2-byte alignment).  R follows C
 * and, per pointer, R * element size bytes of alignment; at the same R a
 * lane sums the same columns in the same order as the fp32 instantiation
 * and the butterfly is the same, so the result is bit-identical to the fp32
 * kernel's on the widened rows. */
__device__ __forceinline__ float seg_sum(float x, uint32_t L) {
  for (uint32_t w = L >> 1; w >= 1; w >>= 1) x += __shfl_xor(x, w, 64);
  return x;
}

template <int R, class Term, typename TD = float, typename TS = float>
__global__ void k_edge_pair_seg(const uint4 *__restrict__ items,
                                const uint32_t *__restrict__ n_items_p,
                                float *__restrict__ out,
                                const TD *__restrict__ dst_rows,
                                const TS *__restrict__ src_rows,
                                const uint32_t *__restrict__ row_indices,
                                uint32_t src_start, uint32_t f, uint32_t K,
                                uint32_t C, uint32_t G, const Term term) {
  const uint32_t n_items = *n_items_p;
  const WaveId w = wave_id();
  const uint32_t L = C / R;          /* lanes per head */
  const uint32_t gl = w.lane & (G - 1);
  const uint32_t gi = w.lane / G;    /* which of the wave's edge slots */
  const uint32_t ng = 64 / G;
  for (uint32_t it = w.wave; it < n_items; it += w.n_waves) {
    const Item im = load_item(items, it);
    const uint32_t e0 = im.e0, cnt = im.cnt;
    for (uint32_t base = 0; base < f; base += G * R) {
      const uint32_t col = base + gl * R;
      const bool live = col < f;     /* f % R == 0: a live lane is full */
      const uint32_t cc = live ? col : 0u;
      const bool writer = live && (gl & (L - 1)) == 0;
      const uint32_t head = cc / C;
      float av[R], xv[R];
      load_cols<R>(dst_rows + (uint64_t)im.v * f + cc, av);
      term.template load<R>(xv, cc);
      /* 4 edge slots per lane group in flight */
      for (uint32_t k0 = 0; k0 < cnt; k0 += 4 * ng) {
        float pr[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t k = min(k0 + q * ng + gi, cnt - 1);
          float bv[R];
          load_cols<R>(src_rows +
                           (uint64_t)(row_indices[e0 + k] - src_start) * f + cc,
                       bv);
          pr[q] = 0.f;
#pragma unroll
          for (int j = 0; j < R; ++j) pr[q] = term(xv[j], av[j], bv[j], pr[q]);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const uint32_t k = k0 + q * ng + gi;
          const float sum = seg_sum(pr[q], L);
          if (writer && k < cnt) out[(uint64_t)(e0 + k) * K + head] = sum;
        }
      }
    }
  }
}

/* general form, any K and C */
template <class Term, typename TD = float, typename TS = float>
__global__ void k_edge_pair(const uint4 *__restrict__ items,
                            const uint32_t *__restrict__ n_items_p,
                            float *__restrict__ out,
                            const TD *__restrict__ dst_rows,
                            const TS *__restrict__ src_rows,
                            const uint32_t *__restrict__ row_indices,
                            uint32_t src_start, uint32_t f, uint32_t K,
                            uint32_t C, const Term term) {
  const uint32_t n_items = *n_items_p;
  const WaveId w = wave_id();
  const uint32_t lane = w.lane;
  for (uint32_t it = w.wave; it < n_items; it += w.n_waves) {
    const Item im = load_item(items, it);
    const uint32_t e0 = im.e0, cnt = im.cnt;
    const TD *a = dst_rows + (uint64_t)im.v * f;
    for (uint32_t k = 0; k < cnt; ++k) {
      const uint32_t e = e0 + k;
      const TS *b = src_rows + (uint64_t)(row_indices[e] - src_start) * f;
      for (uint32_t h = 0; h < K; ++h) {
        float sum = 0.f;
        for (uint32_t j = h * C + lane; j < (h + 1) * C; j += 64) {
          float x[1];
          term.template load<1>(x, j);
          sum = term(x[0], to_f32(a[j]), to_f32(b[j]), sum);
        }
        sum = wave_sum(sum);
        if (lane == 0) out[(uint64_t)e * K + h] = sum;
      }
    }
  }
}

/* ---- GATv2 attention: the backward of the f-wide per-edge score ---- */

/* One walk over an offset array, the shape of k_gather_spmm_heads: a group of
 * G lanes per work item, a lane owning R consecutive columns of one head
 * (R = 1: any f, any K, the head is the column's own).  Per edge the lane
 * loads its R columns of the neighbour row and ONE grad_score[e, head]:
 *   dOwn[j] += gs * lrelu'(t)      -> grad_own[v, col+j] += att[col+j]*dOwn[j]
 *   dAtt[j] += gs * lrelu (t)      (WITH_ATT)
 * The column slab is the outer loop and the group's items the inner one, so
 * dAtt is R registers at any f; after the items the workgroup's 256/G groups
 * meet in LDS and ONE atomicAdd per (workgroup, column) reaches grad_att.
 * T = element type of own_rows and nbr_rows (float, or uint16_t for bfloat16
 * rows, widened exactly on load; R columns are one R*2-byte load, R = 1 a
 * 2-byte load); grad_score, att and both outputs are fp32.  At the same R a
 * lane runs the fp32 instantiation's chains on the widened values. */
template <int R, int NE, typename T>
__device__ __forceinline__ void gatv2_bwd_edges(
    float (&down)[R], float (&datt)[R], const float (&ov)[R],
    const T *__restrict__ nbr_rows, const uint32_t *__restrict__ nbr,
    const float *__restrict__ gscore, uint32_t nbr_start, uint32_t f,
    uint32_t K, uint32_t e, uint32_t col, uint32_t head, float slope,
    bool with_att) {
  float x[NE][R], gs[NE];
#pragma unroll
  for (int k = 0; k < NE; ++k) {
    load_cols<R>(nbr_rows + (uint64_t)(nbr[e + k] - nbr_start) * f + col,
                 x[k]);
    gs[k] = gscore[(uint64_t)(e + k) * K + head];
  }
#pragma unroll
  for (int k = 0; k < NE; ++k)
#pragma unroll
    for (int j = 0; j < R; ++j) {
      const float t = ov[j] + x[k][j];
      down[j] = fmaf(gs[k], t > 0.f ? 1.f : slope, down[j]);
      if (with_att) datt[j] = fmaf(gs[k], lrelu(t, slope), datt[j]);
    }
}

template <int R, bool WITH_ATT, typename T = float>
__global__ __launch_bounds__(NTS_BLOCK) void k_gatv2_backward(
    const uint4 *__restrict__ items, const uint32_t *__restrict__ n_items_p,
    float *__restrict__ grad_own, float *__restrict__ grad_att,
    const float *__restrict__ gscore, const T *__restrict__ own_rows,
    const T *__restrict__ nbr_rows, const float *__restrict__ att,
    float slope, const uint32_t *__restrict__ nbr, uint32_t nbr_start,
    uint32_t f, uint32_t K, uint32_t C, uint32_t G) {
  __shared__ float part[WITH_ATT ? NTS_BLOCK * R : 1];
  const uint32_t n_items = *n_items_p;
  const uint32_t glane = threadIdx.x & (G - 1);
  const uint32_t group = (blockIdx.x * NTS_BLOCK + threadIdx.x) / G;
  const uint32_t n_groups = (gridDim.x * NTS_BLOCK) / G;
  for (uint32_t base = 0; base < f; base += G * R) {
    const uint32_t col = base + glane * R;
    const bool live = col < f;       /* f % R == 0: a live lane is full */
    float datt[R] = {};
    if (live) {
      const uint32_t head = col / C;
      float at[R];
      if constexpr (R == 1) at[0] = att[col];
      else load_lane<R>(att + col, at);
      for (uint32_t it = group; it < n_items; it += n_groups) {
        const Item im = load_item(items, it);
        const uint32_t e_end = im.e0 + im.cnt;
        uint32_t e = im.e0;
        float ov[R], down[R] = {};
        load_cols<R>(own_rows + (uint64_t)im.v * f + col, ov);
        for (; e + 4 <= e_end; e += 4)
          gatv2_bwd_edges<R, 4>(down, datt, ov, nbr_rows, nbr, gscore,
                                nbr_start, f, K, e, col, head, slope, WITH_ATT);
        for (; e < e_end; ++e)
          gatv2_bwd_edges<R, 1>(down, datt, ov, nbr_rows, nbr, gscore,
                                nbr_start, f, K, e, col, head, slope, WITH_ATT);
#pragma unroll
        for (int j = 0; j < R; ++j) down[j] *= at[j];
        store_acc<R>(grad_own + (uint64_t)im.v * f + col, down, R, im.shared);
      }
    }
    if constexpr (WITH_ATT) {
      /* every thread of the workgroup arrives: the slab loop is uniform */
#pragma unroll
      for (int j = 0; j < R; ++j) part[threadIdx.x * R + j] = datt[j];
      __syncthreads();
      if (threadIdx.x < G && live) {
        float sum[R] = {};
        for (uint32_t g = 0; g < NTS_BLOCK / G; ++g)
#pragma unroll
          for (int j = 0; j < R; ++j)
            sum[j] += part[(g * G + threadIdx.x) * R + j];
#pragma unroll
        for (int j = 0; j < R; ++j) atomicAdd(&grad_att[col + j], sum[j]);
      }
      __syncthreads();
    }
  }
}

/* forward softmax also fills msg_cached */
__global__ void k_copy(float *__restrict__ dst, const float *__restrict__ src,
                       uint64_t n) {
  for (uint64_t i = blockIdx.x * (uint64_t)blockDim.x + threadIdx.x; i < n;
       i += (uint64_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}

/* NTS_DEBUG_SYNC=1: synchronize + error-check after every launch (debug). */
bool debug_sync_on() {
  static int v = -1;
  if (v < 0) {
    const char *e = getenv("NTS_DEBUG_SYNC");
    v = (e && *e && *e != '0') ? 1 : 0;
  }
  return v != 0;
}

void dbg_sync(nts_stream *s, const char *what) {
  if (!debug_sync_on()) return;
  hipError_t e = hipStreamSynchronize(s->stream);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) {
    fprintf(stderr, "nts_hip DEBUG after %s: %s\n", what, hipGetErrorString(e));
    abort();
  }
}

uint32_t grid_for(uint64_t threads, uint32_t cap) {
  uint64_t b = (threads + NTS_BLOCK - 1) / NTS_BLOCK;
  if (b < 1) b = 1;
  if (b > cap) b = cap;
  return (uint32_t)b;
}
uint32_t grid_for(uint64_t threads) { return grid_for(threads, NTS_MAX_BLOCKS); }

/* Build the bounded work items for (offset, batch) into the stream's
 * scratch buffer.  Rebuilt on EVERY call: caching by topology pointer is
 * unsound (the host may free a chunk and a later chunk's offsets can land
 * at the same address), and the build is two launches costing ~0.05% of a
 * gather.  All uses are ordered on the stream, so one scratch suffices. */
ItemsBuf &get_items(nts_stream *s, const uint32_t *offset, uint32_t batch,
                    uint32_t edges) {
  /* Opt-in reuse (nts_items_reuse): when the caller has pinned its
   * topology, a rebuilt-identical item set is skipped.  Default stays
   * rebuild-on-every-call — caching by pointer alone is unsound when
   * chunks are freed and reallocated at the same address. */
  if (s->items_reuse) {
    for (auto &slot : s->items_scratch) {
      if (slot.valid && slot.key_off == offset && slot.key_batch == batch &&
          slot.key_edges == edges) {
        return slot;
      }
    }
  }
  ItemsBuf &ib = s->items_scratch[s->items_rr];
  s->items_rr ^= 1;
  const uint64_t need = (uint64_t)batch + edges / NTS_SPLIT + 1;
  if (ib.cap < need) {
    NTS_CHECK(hipStreamSynchronize(s->stream));  /* old buffer may be in use */
    if (ib.items) NTS_CHECK(hipFree(ib.items));
    if (!ib.counter) NTS_CHECK(hipMalloc(&ib.counter, sizeof(uint32_t)));
    NTS_CHECK(hipMalloc(&ib.items, need * sizeof(uint4)));
    ib.cap = need;
  }
  NTS_CHECK(hipMemsetAsync(ib.counter, 0, sizeof(uint32_t), s->stream));
  {
    Tic t(s, NTS_KTAG_ITEMS);
    hipLaunchKernelGGL(k_build_items, dim3(grid_for(batch)), dim3(NTS_BLOCK), 0,
                       s->stream, offset, batch, NTS_SPLIT, ib.items,
                       ib.counter);
  }
  dbg_sync(s, "k_build_items");
  ib.key_off = offset;
  ib.key_batch = batch;
  ib.key_edges = edges;
  ib.valid = s->items_reuse;
  return ib;
}

/* grid of the wave-per-item kernels: one wave per (bounded) work item */
uint32_t items_grid(uint32_t batch, uint32_t edges) {
  return grid_for(((uint64_t)batch + edges / NTS_SPLIT) * 64);
}

/* When the automatic choice engages a blocked column schedule:
 *  - the gathered matrix (rows x f x element bytes) must exceed the 256 MiB Infinity
 *    Cache, far past the 8 x 4 MiB of L2: below that every row stays cached
 *    in any order, and what phase-major buys is a live set (rows x window)
 *    that fits the cache again;
 *  - each window re-reads the item's index and weight lists, up to 16 times
 *    at the narrowest split swept, so a gathered row must be re-read at least
 *    2 x 16 times (edges / rows) for row reuse to outweigh that.
 * One-window widths never engage (n_slabs == 1). */
constexpr uint64_t NTS_BLOCK_MIN_BYTES = 256ull << 20;
constexpr uint32_t NTS_BLOCK_MIN_REUSE = 32;
/* Automatic schedule and window (0 = that schedule's default width): the
 * winner of the sweep recorded in profiles/README.md (round3) — phase-major
 * over the native slab, 55.9 ms/step against 67.1 at the headline shape. */
constexpr int NTS_AUTO_SCHED = NTS_SCHED_PHASE;
constexpr uint32_t NTS_AUTO_WINDOW = 0;
/* The same for bfloat16 rows, from the sweep in profiles/bench_lines.md
 * (bf16 feature rows): XCD-affine over two windows of the headline width,
 * 35.1 ms/step against 37.4 for the native launch and 37.8 phase-major over
 * the native slab.  A width that 302-column windows do not cut into 2, 4 or
 * >= 8 runs the native launch, as for any XCD request. */
constexpr int NTS_AUTO_SCHED_BF16 = NTS_SCHED_XCD;
constexpr uint32_t NTS_AUTO_WINDOW_BF16 = 302;
/* The same for staged fp32 rows (dwordx4 lanes at a pitch of whole lines),
 * from the sweep in profiles/bench_lines.md (Row staging), ms/step at the
 * headline shape with the copy included, unstaged 57.0 in the same process:
 * phase-major over 128-float windows (32 lanes) 44.4; PHASE 256, the native
 * slab, 50.3; PHASE 304 52.5; ITEM 128 at the 2^20 grid 53.1; the native
 * launch 54.8; XCD 2x304 53.8; XCD 4x152 57.6.  A pitch of 640 floats (20
 * lines) instead of 608 (19): 44.7 / 50.1 / 54.0 / 59.0 for PHASE 128 /
 * PHASE 256 / XCD 304 / XCD 152 - no better, so the pitch unit stays one
 * line. */
constexpr int NTS_AUTO_SCHED_STAGED = NTS_SCHED_PHASE;
constexpr uint32_t NTS_AUTO_WINDOW_STAGED = 128;

/* What the environment adds to a gather launch decision, read once like
 * NTS_SPLIT.  Sweep overrides: NTS_GATHER_SCHED forces a schedule (0 = the
 * current order), NTS_GATHER_WINDOW its window width in floats (unset/0 =
 * the schedule's default); NTS_GATHER_STAGE is the row staging request of
 * streams that set none (1 force, -1 never, unset/0 automatic) and
 * NTS_GATHER_STAGE_PITCH the unit in floats the staged pitch is rounded up
 * to (a multiple of 4; unset/0 = NTS_STAGE_PITCH_UNIT); NTS_GATHER_STRIPE is
 * the stripe request of streams that set none (floats; -1 never, unset/0
 * automatic) and NTS_GATHER_STRIPE_RUN the tasks per wave of a striped launch
 * (unset/0 = the fewest that fit the grid cap). */
struct GatherEnv {
  bool forced = false;
  int sched = 0, window = 0;
  int stage = 0;                /* NTS_GATHER_STAGE: 0 auto, 1 force, -1 never */
  uint32_t stage_pitch = 0;     /* NTS_GATHER_STAGE_PITCH, 0 = the default */
  int stripe = 0;               /* NTS_GATHER_STRIPE: floats, -1 never, 0 auto */
  uint32_t stripe_run = 0;      /* NTS_GATHER_STRIPE_RUN, 0 = from the grid cap */
  uint32_t split, max_blocks, gather_blocks;
};
const GatherEnv &gather_env() {
  static const GatherEnv env = [] {
    GatherEnv v;
    const char *e = getenv("NTS_GATHER_SCHED");
    if (e && *e && atoi(e) >= 0) {
      v.forced = true;
      v.sched = atoi(e);
      const char *w = getenv("NTS_GATHER_WINDOW");
      if (w && *w) v.window = atoi(w);
    }
    const char *st = getenv("NTS_GATHER_STAGE");
    if (st && *st) v.stage = atoi(st) > 0 ? 1 : atoi(st) < 0 ? -1 : 0;
    v.stage_pitch = env_u32("NTS_GATHER_STAGE_PITCH", 0);
    const char *sp = getenv("NTS_GATHER_STRIPE");
    if (sp && *sp) v.stripe = atoi(sp) < 0 ? -1 : atoi(sp);
    v.stripe_run = env_u32("NTS_GATHER_STRIPE_RUN", 0);
    v.split = NTS_SPLIT;
    v.max_blocks = NTS_MAX_BLOCKS;
    v.gather_blocks = nts_gather_blocks();
    return v;
  }();
  return env;
}

/* Elements per lane from the width, the row element size and the pointers'
 * common alignment — the widest of 16, 8 or 4 bytes of a row in one load
 * (fp32: dwordx4 / dwordx2; bf16: 8 / 4 / 2 elements), else 4 strided
 * single elements — and the lane group: the smallest power of two in
 * [16,64] covering the slab work */
struct GatherGeom { int elem, nstr; uint32_t G; };
/* also_divides (0 = absent): a second width the lane's element count must
 * divide — the columns per head of a heads gather, so that no lane's vector
 * straddles two heads */
GatherGeom gather_geometry(uint32_t f, uintptr_t alignment,
                           uint32_t elem_bytes, uint32_t also_divides = 0) {
  GatherGeom g;
  g.elem = 1;
  for (uint32_t bytes = 16; bytes > elem_bytes; bytes /= 2) {
    const uint32_t n = bytes / elem_bytes;
    if (f % n == 0 && alignment % bytes == 0 &&
        (!also_divides || also_divides % n == 0)) {
      g.elem = (int)n;
      break;
    }
  }
  g.nstr = (g.elem == 1) ? 4 : 1;
  const uint32_t unit = g.elem * g.nstr; /* elements per lane */
  const uint32_t need = (f + unit - 1) / unit;
  g.G = 64;
  while (g.G / 2 >= need && g.G > 16) g.G /= 2;
  return g;
}

/* The whole launch decision of one gather; pl.sched and pl.wf are the
 * schedule and window that run. */
struct GatherLaunch {
  int elem;
  uint32_t G, grid;
  bool blocked;
  GatherPlan pl;
};

/* Pure: no HIP call, no stream.  rows == 0 (row count unknown to the caller)
 * never engages the automatic choice.  geo is the lane geometry the launch
 * runs with: gather_geometry's, or that of staged rows (staged = true: the
 * automatic choice is then NTS_AUTO_*_STAGED). */
GatherLaunch plan_gather(const GatherGeom &geo, uint32_t f,
                         uint32_t elem_bytes, uint32_t rows, uint32_t batch,
                         uint32_t edges, int sched_req, int window_req,
                         const GatherEnv &env, bool staged = false) {
  const uint32_t elem = geo.elem;
  const uint32_t unit = elem * geo.nstr; /* elements per lane */
  const uint32_t slabf = geo.G * unit;
  const uint32_t n_slabs = (f + slabf - 1) / slabf;
  const uint64_t bound_items = (uint64_t)batch + edges / env.split + 1;

  /* ---- column schedule: request (stream, then env) or automatic ---- */
  int sched = NTS_SCHED_ITEM;
  uint32_t wf = slabf;
  if (sched_req || window_req) {
    sched = sched_req;
    wf = window_req > 0 ? (uint32_t)window_req : 0;
  } else if (env.forced) {
    sched = env.sched;
    wf = env.window > 0 ? (uint32_t)env.window : 0;
  } else if (n_slabs > 1 &&
             (uint64_t)rows * f * elem_bytes > NTS_BLOCK_MIN_BYTES &&
             edges / NTS_BLOCK_MIN_REUSE >= rows) {
    sched = elem_bytes == 2 ? NTS_AUTO_SCHED_BF16
            : staged        ? NTS_AUTO_SCHED_STAGED
                            : NTS_AUTO_SCHED;
    wf = elem_bytes == 2 ? NTS_AUTO_WINDOW_BF16
         : staged        ? NTS_AUTO_WINDOW_STAGED
                         : NTS_AUTO_WINDOW;
  }
  if (sched < NTS_SCHED_ITEM || sched > NTS_SCHED_XCD) sched = NTS_SCHED_ITEM;
  if (wf == 0) {
    /* default width: the native slab; XCD: the widest full lane group
     * (64, 32 or 16 lanes) that still gives every class a window */
    wf = slabf;
    if (sched == NTS_SCHED_XCD)
      for (uint32_t g = 64; g >= 16; g /= 2) {
        wf = g * unit;
        if ((f + wf - 1) / wf >= 8) break;
      }
  }
  wf = (wf + elem - 1) / elem * elem;
  if (wf > f) wf = (f + elem - 1) / elem * elem;
  const uint32_t n_windows = (f + wf - 1) / wf;
  /* lane group of a window: the fewest lane slots (tiles x lanes), widest
   * group on a tie — masked lanes cost as much as live ones */
  uint32_t Gb = 64, tiles = (wf + 64 * unit - 1) / (64 * unit);
  for (uint32_t g = 32; g >= 16; g /= 2) {
    const uint32_t tl = (wf + g * unit - 1) / (g * unit);
    if (tl * g < tiles * Gb) { Gb = g; tiles = tl; }
  }
  uint32_t grid =
      grid_for(bound_items * n_windows * tiles * Gb, env.gather_blocks);
  if (sched == NTS_SCHED_XCD) {
    /* every class needs a workgroup and a window, its own or an even share
     * of one; otherwise the current order runs */
    const uint32_t cap8 = env.gather_blocks & ~7u;
    if ((n_windows < 8 && n_windows != 4 && n_windows != 2) || grid < 8 ||
        cap8 < 8) {
      sched = NTS_SCHED_ITEM;
      wf = slabf;
    } else {
      grid = min((grid + 7u) & ~7u, cap8);
    }
  }
  if (n_windows > 1 && !(sched == NTS_SCHED_ITEM && wf == slabf))
    return GatherLaunch{geo.elem, Gb, grid, true,
                        GatherPlan{(uint32_t)sched, wf, n_windows, tiles}};
  /* exactly the pre-window launch */
  return GatherLaunch{
      geo.elem, geo.G,
      grid_for(bound_items * n_slabs * geo.G, env.max_blocks), false,
      GatherPlan{NTS_SCHED_ITEM, slabf, n_slabs, 1u}};
}
/* the unstaged launch: lanes from the pointers' common alignment */
GatherLaunch plan_gather(uint32_t f, uintptr_t alignment, uint32_t elem_bytes,
                         uint32_t rows, uint32_t batch, uint32_t edges,
                         int sched_req, int window_req, const GatherEnv &env) {
  return plan_gather(gather_geometry(f, alignment, elem_bytes), f, elem_bytes,
                     rows, batch, edges, sched_req, window_req, env);
}

/* Row staging.  A gather's time follows lane slots and touched 128-byte
 * lines, not payload bytes: at f = 602 a row is 2408
 * bytes, 8-byte aligned and never a whole number of lines, so it runs
 * dwordx2 lanes over five windows, most of which straddle an extra line.
 * Staging copies the gathered matrix once per launch (k_repitch) into a
 * stream-owned buffer whose rows start on a line and are a whole number of
 * lines long; the gather then reads it with dwordx4 lanes, whatever the
 * caller's width and alignment (automatic choice: NTS_AUTO_*_STAGED).
 *
 * Automatic staging engages for fp32 rows when
 *  - rows is known and the staged pitch differs from f;
 *  - the blocked-schedule conditions hold (more than one native slab, matrix
 *    beyond NTS_BLOCK_MIN_BYTES): below them the rows stay cached and the
 *    straddled lines cost no HBM traffic;
 *  - edges / rows >= NTS_STAGE_MIN_REUSE.  The copy reads and writes each
 *    row once where the gather reads it edges / rows times: 2 / reuse of the
 *    gather's row bytes, 3% at 64, a quarter of the 12% that the padded
 *    width is worth at the headline shape (f = 608 against 602 in
 *    profiles/bench_lines.md), so the copy cannot eat the gain;
 *  - the staged matrix is at most NTS_STAGE_MAX_BYTES. */
constexpr uint32_t NTS_STAGE_MIN_REUSE = 64;
/* Staged pitch: f rounded up to this many floats (one 128-byte line), so
 * every row starts on a line and is a whole number of lines. */
constexpr uint32_t NTS_STAGE_PITCH_UNIT = 32;
/* Cap of the staging buffer, which lives as long as its stream: 4 GiB is
 * seven times the headline matrix (567 MB) and 1.4% of the 288 GB of HBM; a
 * matrix beyond it is one a caller partitions into chunks anyway.  It holds
 * for forced requests too. */
constexpr uint64_t NTS_STAGE_MAX_BYTES = 4ull << 30;

/* Floats per vector access of `out` in a staged launch: from the output's
 * alignment and f alone (the lanes are dwordx4 whatever the output is) */
int stage_store_width(uint32_t f, uintptr_t out_alignment) {
  if (f % 4 == 0 && out_alignment % 16 == 0) return 4;
  if (f % 2 == 0 && out_alignment % 8 == 0) return 2;
  return 1;
}

/* The whole decision of one gather: whether its rows are staged, at which
 * pitch, and the launch that runs.  Pure, like plan_gather.  stage_req is the
 * stream's nts_gather_staging request (0: the environment's, else automatic). */
struct StagePlan {
  bool staged;
  uint32_t ld;  /* row pitch of the gathered rows in elements: f if unstaged */
  int ov;       /* floats per vector access of `out` */
  GatherLaunch L;
};
StagePlan plan_stage(uint32_t f, uint32_t elem_bytes, uintptr_t in_alignment,
                     uintptr_t out_alignment, uint32_t rows, uint32_t batch,
                     uint32_t edges, int sched_req, int window_req,
                     int stage_req, const GatherEnv &env) {
  const int req = stage_req ? stage_req : env.stage;
  const uint32_t unit =
      env.stage_pitch ? (env.stage_pitch + 3u) / 4u * 4u : NTS_STAGE_PITCH_UNIT;
  const uint64_t ld = ((uint64_t)f + unit - 1) / unit * unit;
  bool staged = elem_bytes == sizeof(float) && rows && req >= 0 &&
                ld <= 0xffffffffu &&
                (uint64_t)rows * ld * sizeof(float) <= NTS_STAGE_MAX_BYTES;
  if (staged && req == 0) {
    const GatherGeom native =
        gather_geometry(f, in_alignment | out_alignment, elem_bytes);
    const uint32_t slabf = native.G * native.elem * native.nstr;
    staged = ld != f && f > slabf &&
             (uint64_t)rows * f * elem_bytes > NTS_BLOCK_MIN_BYTES &&
             edges / NTS_STAGE_MIN_REUSE >= rows;
  }
  if (!staged) {
    const GatherLaunch L =
        plan_gather(f, in_alignment | out_alignment, elem_bytes, rows, batch,
                    edges, sched_req, window_req, env);
    return StagePlan{false, f, common_ov(L.elem, (int)elem_bytes), L};
  }
  /* staged rows: dwordx4 lanes, the smallest lane group covering f */
  GatherGeom geo{4, 1, 64};
  while (geo.G / 2 >= (f + 3) / 4 && geo.G > 16) geo.G /= 2;
  return StagePlan{true, (uint32_t)ld, stage_store_width(f, out_alignment),
                   plan_gather(geo, f, elem_bytes, rows, batch, edges,
                               sched_req, window_req, env, true)};
}

/* Stripes (k_gather_spmm_stripe) are an attribute of a staged PHASE launch.
 * Automatic stripe width in floats (0 = none) and the least tasks per wave
 * of an automatic launch, from the sweep in profiles/bench_lines.md
 * (Stripes), kernel ms per forward + backward step at the headline shape,
 * the launch without stripes 44.7 to 45.1 in the same processes.  Window 128,
 * width / R: 128 (two sub-groups, no XCD split) 42.9 / 1, 40.0 / 4, 39.9 / 8,
 * 40.4 / 16; 64 (two stripes) 45.0 / 1, 37.4 / 4, 36.5 / 8, 36.0 / 16,
 * 36.3 / 32, 37.6 / 64; 32 (four) 53.6 / 1, 42.2 / 4, 38.8 / 8, 36.9 / 16,
 * 36.4 / 32, 38.6 / 64; 16 (eight) 74.1 / 4, 69.1 / 8.  Window 256: 64
 * (four stripes) 35.3 / 16, 35.5 / 32; 32 (eight) 42.2 / 4, 40.7 / 32; 128
 * (two) 39.8 / 8.  Window 256 / 64 is 0.7 ms below window 128 / 64 in both
 * sweeps that held the two; the window stays the 128 of the staged launch. */
constexpr uint32_t NTS_AUTO_STRIPE_STAGED = 64;
constexpr uint32_t NTS_AUTO_STRIPE_RUN = 16;

/* The stripe decision on top of a staged launch decision.  Pure, like
 * plan_stage.  stripe_req is the stream's nts_gather_stripes request (0: the
 * environment's, else automatic), run_req its tasks per wave (0: the
 * environment's, else NTS_AUTO_STRIPE_RUN for an automatic launch and the
 * fewest that fit the grid cap for a forced width; never fewer than fit).
 * Automatic: fp32 rows, staged by automatic choice, PHASE by automatic choice
 * (no schedule, window or staging request from the stream or the environment,
 * which implies the blocked-schedule conditions), and the automatic width
 * cuts the window into 1, 2, 4 or 8 stripes.  A request > 0 forces that width
 * on any staged launch that runs PHASE or was asked to (a width of one window
 * runs the native launch unstriped; striped it keeps the window asked for);
 * a width that does not cut the window into 1, 2, 4 or 8 stripes of 4 to 64
 * dwordx4 lanes runs without stripes. */
struct StripeLaunch {
  bool on;
  uint32_t Gs, P, grid; /* lanes per stripe, sub-groups per wave, workgroups */
  StripePlan sp;
};
StripeLaunch plan_stripe(const StagePlan &P, uint32_t f, uint32_t elem_bytes,
                         uint32_t batch, uint32_t edges, int sched_req,
                         int window_req, int stage_req, int stripe_req,
                         int run_req, const GatherEnv &env) {
  StripeLaunch off{};
  const int req = stripe_req ? stripe_req : env.stripe;
  if (req < 0 || !P.staged || elem_bytes != sizeof(float)) return off;
  /* the schedule request as plan_gather reads it */
  int rs = 0;
  uint32_t rw = 0;
  bool asked = false;
  if (sched_req || window_req) {
    asked = true;
    rs = sched_req;
    rw = window_req > 0 ? (uint32_t)window_req : 0;
  } else if (env.forced) {
    asked = true;
    rs = env.sched;
    rw = env.window > 0 ? (uint32_t)env.window : 0;
  }
  const bool phase = P.L.blocked && P.L.pl.sched == NTS_SCHED_PHASE;
  uint32_t sf, wf = P.L.pl.wf;
  if (req == 0) {
    if (asked || stage_req || env.stage || !phase) return off;
    sf = NTS_AUTO_STRIPE_STAGED;
  } else {
    if (!phase && !(asked && rs == NTS_SCHED_PHASE)) return off;
    if (!P.L.blocked && rw) wf = (rw + 3u) / 4u * 4u;
    sf = (uint32_t)req;
  }
  if (!sf || sf % 4u || wf % sf) return off;
  const uint32_t S = wf / sf, Gs = sf / 4u;
  if (S != 1 && S != 2 && S != 4 && S != 8) return off;
  if (Gs < 4 || Gs > 64 || (Gs & (Gs - 1))) return off;
  const uint32_t cap8 = env.gather_blocks & ~7u;
  if (cap8 < 8) return off;

  StripePlan sp{};
  sp.wf = wf;
  sp.sf = sf;
  sp.S = S;
  sp.n_windows = (f + wf - 1) / wf;
  const uint32_t last_w = f - (sp.n_windows - 1) * wf;
  const uint32_t last_live = (last_w + sf - 1) / sf;
  sp.n_full = last_live == S ? sp.n_windows : sp.n_windows - 1;
  sp.last_live = last_live == S ? 0u : last_live;
  /* the largest class: items dealt among the 8 / S classes of a stripe, the
   * short window's tasks among all eight */
  const uint64_t bound_items = (uint64_t)batch + edges / env.split + 1;
  const uint32_t cpw = 8u / S;
  const uint64_t tasks = (uint64_t)sp.n_full * ((bound_items + cpw - 1) / cpw) +
                         (bound_items * sp.last_live + 7u) / 8u;
  const uint64_t waves_cap = (uint64_t)(cap8 / 8u) * (NTS_BLOCK / 64);
  uint64_t R = (tasks + waves_cap - 1) / waves_cap;
  const uint32_t want = run_req > 0       ? (uint32_t)run_req
                        : env.stripe_run ? env.stripe_run
                        : req == 0       ? NTS_AUTO_STRIPE_RUN
                                         : 0u;
  if (R < want) R = want;
  if (R < 1) R = 1;
  if (R > 0xffffffffu) return off;
  sp.R = (uint32_t)R;
  const uint64_t waves = (tasks + R - 1) / R;
  uint64_t blocks = (waves + NTS_BLOCK / 64 - 1) / (NTS_BLOCK / 64);
  if (blocks < 1) blocks = 1;
  return StripeLaunch{true, Gs, 64u / Gs, (uint32_t)(blocks * 8u), sp};
}

/* The stream's staging buffer, grown on demand.  One per stream suffices:
 * the copy into it and the gather that reads it are ordered on the stream,
 * and so is the next call's copy behind that gather.  It is rebuilt on every
 * call: the rows are new data each time, and caching by pointer is unsound
 * for the reason get_items gives. */
float *get_stage(nts_stream *s, uint64_t n) {
  if (s->stage_cap < n) {
    NTS_CHECK(hipStreamSynchronize(s->stream)); /* old buffer may be in use */
    if (s->stage_ws) NTS_CHECK(hipFree(s->stage_ws));
    s->stage_ws = nullptr;
    s->stage_cap = 0;
    NTS_CHECK(hipMalloc(&s->stage_ws, n * sizeof(float)));
    /* rows start on a 128-byte line: a 32-float stripe of a row is then
     * exactly one line (k_gather_spmm_stripe) */
    if ((uintptr_t)s->stage_ws % 128 != 0) {
      fprintf(stderr, "nts_hip: staging buffer %p is not 128-byte aligned\n",
              (void *)s->stage_ws);
      abort();
    }
    s->stage_cap = n;
  }
  return s->stage_ws;
}

/* T = row element type of `in` (float, or uint16_t for bfloat16) */
template <typename T>
void launch_gather(nts_stream *s, const T *in, float *out, const float *ew,
                   const uint32_t *nbr, const uint32_t *offset,
                   uint32_t nbr_start, uint32_t batch, uint32_t edges,
                   uint32_t f, int with_weight, int tag, uint32_t rows) {
  if (!batch || !edges || !f) return;
  ItemsBuf &ib = get_items(s, offset, batch, edges);
  const StagePlan P = plan_stage(f, sizeof(T), (uintptr_t)in, (uintptr_t)out,
                                 rows, batch, edges, s->sched_req,
                                 s->window_req, s->stage_req, gather_env());
  const GatherLaunch &L = P.L;
  using Kernel = decltype(&k_gather_spmm<T, 1, false, false>);
#define NTS_K(E)                                                              \
  {{k_gather_spmm<T, E, false, false>, k_gather_spmm<T, E, false, true>},     \
   {k_gather_spmm<T, E, true, false>, k_gather_spmm<T, E, true, true>}}
  /* indexed by log2(elements per lane); the last entry is the widest lane:
   * 4 dwords, or 8 bf16 */
  constexpr int WIDEST = 16 / (int)sizeof(T);
  static const Kernel kernels[4][2][2] = {NTS_K(1), NTS_K(2), NTS_K(4),
                                          NTS_K(WIDEST)};
#undef NTS_K
  s->sched_last = (int)L.pl.sched;
  s->window_last = (int)L.pl.wf;
  s->staged_last = P.staged;
  s->stage_ld_last = P.staged ? P.ld : 0;
  s->stripe_last = s->stripe_run_last = 0;
  if constexpr (sizeof(T) == sizeof(float)) {
    if (P.staged) {
#define NTS_K(OV)                                                             \
  {{k_gather_spmm<float, 4, false, false, OV>,                                \
    k_gather_spmm<float, 4, false, true, OV>},                                \
   {k_gather_spmm<float, 4, true, false, OV>,                                 \
    k_gather_spmm<float, 4, true, true, OV>}}
      /* dwordx4 lanes; indexed by log2(floats per access of `out`) */
      static const Kernel staged_kernels[3][2][2] = {NTS_K(1), NTS_K(2),
                                                     NTS_K(4)};
#undef NTS_K
      float *stage = get_stage(s, (uint64_t)rows * P.ld);
      const int sv = stage_store_width(f, (uintptr_t)in); /* source side */
      /* one bracket: the copy's cost is part of the gather's tag */
      Tic t(s, tag);
      hipLaunchKernelGGL(sv == 4   ? k_repitch<4>
                         : sv == 2 ? k_repitch<2>
                                   : k_repitch<1>,
                         dim3(grid_for((uint64_t)rows * 64)), dim3(NTS_BLOCK),
                         0, s->stream, in, stage, rows, f, P.ld);
      const StripeLaunch SL = plan_stripe(
          P, f, sizeof(T), batch, edges, s->sched_req, s->window_req,
          s->stage_req, s->stripe_req, s->stripe_run_req, gather_env());
      if (SL.on) {
        using SKernel = decltype(&k_gather_spmm_stripe<4, false, 1, 4>);
#define NTS_K(OV, GS)                                                         \
  {k_gather_spmm_stripe<4, false, OV, GS>, k_gather_spmm_stripe<4, true, OV, GS>}
#define NTS_KG(OV)                                                            \
  {NTS_K(OV, 4), NTS_K(OV, 8), NTS_K(OV, 16), NTS_K(OV, 32), NTS_K(OV, 64)}
        /* indexed by log2(floats per access of `out`), log2(lanes / 4) */
        static const SKernel stripe_kernels[3][5][2] = {NTS_KG(1), NTS_KG(2),
                                                        NTS_KG(4)};
#undef NTS_KG
#undef NTS_K
        s->sched_last = NTS_SCHED_PHASE;
        s->window_last = (int)SL.sp.wf;
        s->stripe_last = SL.sp.sf;
        s->stripe_run_last = SL.sp.R;
        hipLaunchKernelGGL(stripe_kernels[__builtin_ctz((unsigned)P.ov)]
                                         [__builtin_ctz(SL.Gs) - 2]
                                         [with_weight != 0],
                           dim3(SL.grid), dim3(NTS_BLOCK), 0, s->stream,
                           ib.items, ib.counter, nbr, ew, (const float *)stage,
                           out, nbr_start, f, P.ld, SL.sp);
        dbg_sync(s, "k_gather_spmm_stripe");
        return;
      }
      hipLaunchKernelGGL(staged_kernels[__builtin_ctz((unsigned)P.ov)]
                                       [with_weight != 0][L.blocked],
                         dim3(L.grid), dim3(NTS_BLOCK), 0, s->stream, ib.items,
                         ib.counter, nbr, ew, (const float *)stage, out,
                         nbr_start, f, P.ld, L.G, L.pl);
      dbg_sync(s, "k_gather_spmm (staged)");
      return;
    }
  }
  Tic t(s, tag);
  hipLaunchKernelGGL(kernels[__builtin_ctz((unsigned)L.elem)]
                            [with_weight != 0][L.blocked],
                     dim3(L.grid), dim3(NTS_BLOCK), 0, s->stream, ib.items,
                     ib.counter, nbr, ew, in, out, nbr_start, f, f, L.G, L.pl);
  dbg_sync(s, "k_gather_spmm");
}

/* heads: 1 <= K <= f and K | f, else abort (error culture of the header) */
void check_heads(const char *entry, uint32_t f, uint32_t heads) {
  if (heads == 0 || heads > f || f % heads != 0) {
    fprintf(stderr, "%s: heads %u does not divide feature_size %u\n", entry,
            heads, f);
    abort();
  }
}

/* Launch decision of a heads gather: always the native launch (one tile per
 * slab, item-major), lanes narrowed until they divide the columns per head.
 * Pure, like plan_gather; at K = 1 it is plan_gather's native launch.
 * elem_bytes = 2 (bf16 rows): elements per lane are the widest of 8 / 4 / 2
 * that divides C as well as f and whose load (16 / 8 / 4 bytes) the common
 * alignment of `in` and `out` permits — `out` is then accessed in vectors of
 * half as many floats, the rule of the scalar bf16 gather — else 4 strided
 * single elements; the lane group is the smallest power of two in [16, 64]
 * covering f, the grid bound_items * slabs * lanes under the block cap. */
GatherLaunch plan_gather_heads(uint32_t f, uint32_t heads, uintptr_t alignment,
                               uint32_t batch, uint32_t edges,
                               const GatherEnv &env,
                               uint32_t elem_bytes = sizeof(float)) {
  const GatherGeom geo = gather_geometry(f, alignment, elem_bytes, f / heads);
  const uint32_t slabf = geo.G * geo.elem * geo.nstr;
  const uint32_t n_slabs = (f + slabf - 1) / slabf;
  const uint64_t bound_items = (uint64_t)batch + edges / env.split + 1;
  return GatherLaunch{
      geo.elem, geo.G,
      grid_for(bound_items * n_slabs * geo.G, env.max_blocks), false,
      GatherPlan{NTS_SCHED_ITEM, slabf, n_slabs, 1u}};
}

template <typename T>
void launch_gather_heads(nts_stream *s, const char *entry, const T *in,
                         float *out, const float *ew, const uint32_t *nbr,
                         const uint32_t *offset, uint32_t nbr_start,
                         uint32_t batch, uint32_t edges, uint32_t f,
                         uint32_t heads, int tag, uint32_t rows) {
  check_heads(entry, f, heads);
  if (heads == 1) { /* the scalar gather itself */
    launch_gather(s, in, out, ew, nbr, offset, nbr_start, batch, edges, f, 1,
                  tag, rows);
    return;
  }
  if (!batch || !edges) return;
  ItemsBuf &ib = get_items(s, offset, batch, edges);
  const GatherLaunch L = plan_gather_heads(
      f, heads, (uintptr_t)in | (uintptr_t)out, batch, edges, gather_env(),
      sizeof(T));
  s->sched_last = (int)L.pl.sched;
  s->window_last = (int)L.pl.wf;
  s->stripe_last = s->stripe_run_last = 0;
  /* indexed by log2(elements per lane); the last entry is the widest lane:
   * 4 dwords, or 8 bf16 */
  constexpr int WIDEST = 16 / (int)sizeof(T);
  static const decltype(&k_gather_spmm_heads<1, T>) kernels[4] = {
      k_gather_spmm_heads<1, T>, k_gather_spmm_heads<2, T>,
      k_gather_spmm_heads<4, T>, k_gather_spmm_heads<WIDEST, T>};
  Tic t(s, tag);
  hipLaunchKernelGGL(kernels[__builtin_ctz((unsigned)L.elem)],
                     dim3(L.grid), dim3(NTS_BLOCK), 0, s->stream, ib.items,
                     ib.counter, nbr, ew, in, out, nbr_start, f, L.G,
                     L.pl.n_windows, heads, f / heads);
  dbg_sync(s, "k_gather_spmm_heads");
}

/* ---- max / min gather ---- */
void check_reduce_op(const char *entry, int op) {
  if (op != NTS_REDUCE_MAX && op != NTS_REDUCE_MIN) {
    fprintf(stderr, "%s: op %d is neither NTS_REDUCE_MAX nor NTS_REDUCE_MIN\n",
            entry, op);
    abort();
  }
}

/* Launch decision of a max / min gather: the scalar gather's native launch
 * (request (0, -1)), plus the bytes of key scratch the hub merge needs —
 * none while no vertex can be split.  Pure, like plan_gather. */
struct ReduceLaunch {
  GatherLaunch L;
  uint64_t key_elems; /* u64 keys: batch * f, or 0 */
};
ReduceLaunch plan_reduce(uint32_t f, uintptr_t alignment, uint32_t batch,
                         uint32_t edges, const GatherEnv &env) {
  ReduceLaunch r{};
  if (!batch || !edges || !f) return r; /* no gather is launched */
  r.L = plan_gather(f, alignment, sizeof(float), batch, batch, edges,
                    NTS_SCHED_ITEM, -1, env);
  r.key_elems = edges > env.split ? (uint64_t)batch * f : 0;
  return r;
}

/* stream-owned key scratch, grown on demand (not cleared: the row pre-pass
 * zeroes what the launch uses) */
unsigned long long *get_keys(nts_stream *s, uint64_t n) {
  if (s->keys_cap < n) {
    NTS_CHECK(hipStreamSynchronize(s->stream)); /* old buffer may be in use */
    if (s->keys_ws) NTS_CHECK(hipFree(s->keys_ws));
    NTS_CHECK(hipMalloc(&s->keys_ws, n * sizeof(unsigned long long)));
    s->keys_cap = n;
  }
  return s->keys_ws;
}

void launch_reduce(nts_stream *s, int op, const float *in, float *out,
                   uint32_t *arg, const uint32_t *nbr, const uint32_t *offset,
                   uint32_t nbr_start, uint32_t batch, uint32_t edges,
                   uint32_t f) {
  check_reduce_op("nts_reduce_by_dst_from_src", op);
  if (!batch || !f) return;
  const ReduceLaunch R = plan_reduce(
      f, (uintptr_t)in | (uintptr_t)out | (uintptr_t)arg, batch, edges,
      gather_env());
  ItemsBuf *ib = edges ? &get_items(s, offset, batch, edges) : nullptr;
  unsigned long long *keys = R.key_elems ? get_keys(s, R.key_elems) : nullptr;
  const uint32_t row_grid = grid_for((uint64_t)batch * 64);
  s->sched_last = NTS_SCHED_ITEM;
  s->window_last = (int)R.L.pl.wf;
  s->stripe_last = s->stripe_run_last = 0;
  Tic t(s, NTS_KTAG_FWD);
  hipLaunchKernelGGL((k_reduce_rows<false, false>), dim3(row_grid),
                     dim3(NTS_BLOCK), 0, s->stream, offset, batch, NTS_SPLIT,
                     out, arg, keys, f);
  if (ib) {
    using Kernel = decltype(&k_gather_reduce<1, false, false>);
#define NTS_K(E)                                                              \
  {{k_gather_reduce<E, false, false>, k_gather_reduce<E, false, true>},       \
   {k_gather_reduce<E, true, false>, k_gather_reduce<E, true, true>}}
    /* [log2(dwords per lane)][min][message form] */
    static const Kernel kernels[3][2][2] = {NTS_K(1), NTS_K(2), NTS_K(4)};
#undef NTS_K
    hipLaunchKernelGGL(
        kernels[__builtin_ctz((unsigned)R.L.elem)][op == NTS_REDUCE_MIN]
               [nbr == nullptr],
        dim3(R.L.grid), dim3(NTS_BLOCK), 0, s->stream, ib->items, ib->counter,
        nbr, in, out, arg, keys, nbr_start, f, R.L.G, R.L.pl.n_windows);
  }
  if (keys)
    hipLaunchKernelGGL((op == NTS_REDUCE_MIN ? k_reduce_rows<true, true>
                                             : k_reduce_rows<true, false>),
                       dim3(row_grid), dim3(NTS_BLOCK), 0, s->stream, offset,
                       batch, NTS_SPLIT, out, arg, keys, f);
  dbg_sync(s, "k_gather_reduce");
}
}  // namespace

/* ================= C-ABI ================= */
extern "C" {

nts_stream *nts_stream_create(void) {
  nts_stream *s = new nts_stream();
  NTS_CHECK(hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking));
  s->owned = true;
  return s;
}

nts_stream *nts_stream_wrap(void *hip_stream) {
  nts_stream *s = new nts_stream();
  s->stream = (hipStream_t)hip_stream;
  s->owned = false;
  return s;
}

void nts_stream_destroy(nts_stream *s) {
  if (!s) return;
  drain_timing(s);
  for (auto &p : s->freeev) {
    hipEventDestroy(p.first);
    hipEventDestroy(p.second);
  }
  for (auto &slot : s->items_scratch) {
    if (slot.items) hipFree(slot.items);
    if (slot.counter) hipFree(slot.counter);
  }
  if (s->sums_ws) hipFree(s->sums_ws);
  if (s->pairs_ws) hipFree(s->pairs_ws);
  if (s->keys_ws) hipFree(s->keys_ws);
  if (s->stage_ws) hipFree(s->stage_ws);
  if (s->owned) hipStreamDestroy(s->stream);
  delete s;
}

void nts_stream_sync(nts_stream *s) { NTS_CHECK(hipStreamSynchronize(s->stream)); }
void *nts_stream_handle(nts_stream *s) { return (void *)s->stream; }

void nts_stream_wait_stream(nts_stream *waiter, nts_stream *waitee) {
  /* hipEventDestroy is stream-safe after the wait is enqueued (the wait
   * captured the record at call time); creation cost is ~µs, called P-1
   * times per layer */
  hipEvent_t ev;
  NTS_CHECK(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  NTS_CHECK(hipEventRecord(ev, waitee->stream));
  NTS_CHECK(hipStreamWaitEvent(waiter->stream, ev, 0));
  NTS_CHECK(hipEventDestroy(ev));
}

void nts_stream_timing(nts_stream *s, int enable) { s->timing = enable != 0; }

void nts_stream_timing_reset(nts_stream *s) {
  drain_timing(s);
  memset(s->acc_ns, 0, sizeof(s->acc_ns));
  memset(s->acc_n, 0, sizeof(s->acc_n));
}

double nts_stream_kernel_ns(nts_stream *s, int tag) {
  drain_timing(s);
  return (tag >= 0 && tag < NTS_KTAG_COUNT) ? s->acc_ns[tag] : 0.0;
}

long long nts_stream_kernel_launches(nts_stream *s, int tag) {
  drain_timing(s);
  return (tag >= 0 && tag < NTS_KTAG_COUNT) ? s->acc_n[tag] : 0;
}

void *nts_malloc_gpu(long bytes) {
  void *p = nullptr;
  NTS_CHECK(hipMalloc(&p, (size_t)bytes));
  return p;
}

void *nts_malloc_pinned(long bytes) {
  void *p = nullptr;
  NTS_CHECK(hipHostMalloc(&p, (size_t)bytes, hipHostMallocMapped));
  return p;
}

void *nts_get_device_pointer(void *pinned) {
  void *d = nullptr;
  NTS_CHECK(hipHostGetDevicePointer(&d, pinned, 0));
  return d;
}

void nts_free_gpu(void *p) { NTS_CHECK(hipFree(p)); }
void nts_free_host(void *p) { NTS_CHECK(hipHostFree(p)); }

void nts_zero_buffer(nts_stream *s, float *d, long n) {
  NTS_CHECK(hipMemsetAsync(d, 0, (size_t)n * sizeof(float), s->stream));
}

void nts_memcpy_h2d(nts_stream *s, void *d, const void *h, long bytes, int sync) {
  NTS_CHECK(hipMemcpyAsync(d, h, (size_t)bytes, hipMemcpyHostToDevice, s->stream));
  if (sync) NTS_CHECK(hipStreamSynchronize(s->stream));
}

void nts_memcpy_d2h(nts_stream *s, void *h, const void *d, long bytes, int sync) {
  NTS_CHECK(hipMemcpyAsync(h, d, (size_t)bytes, hipMemcpyDeviceToHost, s->stream));
  if (sync) NTS_CHECK(hipStreamSynchronize(s->stream));
}

void nts_gather_by_dst_from_src(nts_stream *s, const float *input,
                                float *output, const float *weight_forward,
                                const nts_vid *row_indices,
                                const nts_vid *column_offset, nts_vid src_start,
                                nts_vid src_end, nts_vid dst_start,
                                nts_vid dst_end, nts_vid edges,
                                nts_vid batch_size, nts_vid feature_size,
                                int with_weight) {
  (void)dst_start; (void)dst_end;
  launch_gather(s, input, output, weight_forward, row_indices, column_offset,
                src_start, batch_size, edges, feature_size, with_weight,
                NTS_KTAG_FWD, src_end > src_start ? src_end - src_start : 0);
}

void nts_gather_by_src_from_dst(nts_stream *s, const float *input,
                                float *output, const float *weight_backward,
                                const nts_vid *row_offset,
                                const nts_vid *column_indices,
                                nts_vid src_start, nts_vid src_end,
                                nts_vid dst_start, nts_vid dst_end,
                                nts_vid edges, nts_vid batch_size,
                                nts_vid feature_size, int with_weight) {
  (void)src_start; (void)src_end;
  launch_gather(s, input, output, weight_backward, column_indices, row_offset,
                dst_start, batch_size, edges, feature_size, with_weight,
                NTS_KTAG_BWD, dst_end > dst_start ? dst_end - dst_start : 0);
}

void nts_gather_by_dst_from_src_bf16(
    nts_stream *s, const uint16_t *input, float *output,
    const float *weight_forward, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, int with_weight) {
  (void)dst_start; (void)dst_end;
  launch_gather(s, input, output, weight_forward, row_indices, column_offset,
                src_start, batch_size, edges, feature_size, with_weight,
                NTS_KTAG_FWD, src_end > src_start ? src_end - src_start : 0);
}

void nts_gather_by_src_from_dst_bf16(
    nts_stream *s, const uint16_t *input, float *output,
    const float *weight_backward, const nts_vid *row_offset,
    const nts_vid *column_indices, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, int with_weight) {
  (void)src_start; (void)src_end;
  launch_gather(s, input, output, weight_backward, column_indices, row_offset,
                dst_start, batch_size, edges, feature_size, with_weight,
                NTS_KTAG_BWD, dst_end > dst_start ? dst_end - dst_start : 0);
}

void nts_gather_by_dst_from_src_heads(
    nts_stream *s, const float *input, float *output,
    const float *weight_forward, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, nts_vid heads) {
  (void)dst_start; (void)dst_end;
  launch_gather_heads(s, "nts_gather_by_dst_from_src_heads", input, output,
                      weight_forward, row_indices, column_offset, src_start,
                      batch_size, edges, feature_size, heads, NTS_KTAG_FWD,
                      src_end > src_start ? src_end - src_start : 0);
}

void nts_gather_by_src_from_dst_heads(
    nts_stream *s, const float *input, float *output,
    const float *weight_backward, const nts_vid *row_offset,
    const nts_vid *column_indices, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, nts_vid heads) {
  (void)src_start; (void)src_end;
  launch_gather_heads(s, "nts_gather_by_src_from_dst_heads", input, output,
                      weight_backward, column_indices, row_offset, dst_start,
                      batch_size, edges, feature_size, heads, NTS_KTAG_BWD,
                      dst_end > dst_start ? dst_end - dst_start : 0);
}

void nts_gather_by_dst_from_src_heads_bf16(
    nts_stream *s, const uint16_t *input, float *output,
    const float *weight_forward, const nts_vid *row_indices,
    const nts_vid *column_offset, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, nts_vid heads) {
  (void)dst_start; (void)dst_end;
  launch_gather_heads(s, "nts_gather_by_dst_from_src_heads_bf16", input,
                      output, weight_forward, row_indices, column_offset,
                      src_start, batch_size, edges, feature_size, heads,
                      NTS_KTAG_FWD,
                      src_end > src_start ? src_end - src_start : 0);
}

void nts_gather_by_src_from_dst_heads_bf16(
    nts_stream *s, const uint16_t *input, float *output,
    const float *weight_backward, const nts_vid *row_offset,
    const nts_vid *column_indices, nts_vid src_start, nts_vid src_end,
    nts_vid dst_start, nts_vid dst_end, nts_vid edges, nts_vid batch_size,
    nts_vid feature_size, nts_vid heads) {
  (void)src_start; (void)src_end;
  launch_gather_heads(s, "nts_gather_by_src_from_dst_heads_bf16", input,
                      output, weight_backward, column_indices, row_offset,
                      dst_start, batch_size, edges, feature_size, heads,
                      NTS_KTAG_BWD,
                      dst_end > dst_start ? dst_end - dst_start : 0);
}

static void report_plan_heads(const char *entry, uint32_t elem_bytes,
                              nts_vid feature_size, nts_vid heads,
                              unsigned alignment_bytes, nts_vid batch_size,
                              nts_vid edges, int *lane_group,
                              int *vector_width, int *grid) {
  check_heads(entry, feature_size, heads);
  GatherLaunch L{};
  if (batch_size && edges) /* else nothing is launched */
    L = plan_gather_heads(feature_size, heads, alignment_bytes, batch_size,
                          edges, gather_env(), elem_bytes);
  if (lane_group) *lane_group = (int)L.G;
  if (vector_width) *vector_width = L.elem;
  if (grid) *grid = (int)L.grid;
}

void nts_gather_plan_heads(nts_vid feature_size, nts_vid heads,
                           unsigned alignment_bytes, nts_vid batch_size,
                           nts_vid edges, int *lane_group, int *vector_width,
                           int *grid) {
  report_plan_heads("nts_gather_plan_heads", sizeof(float), feature_size,
                    heads, alignment_bytes, batch_size, edges, lane_group,
                    vector_width, grid);
}

void nts_gather_plan_heads_bf16(nts_vid feature_size, nts_vid heads,
                                unsigned alignment_bytes, nts_vid batch_size,
                                nts_vid edges, int *lane_group,
                                int *vector_width, int *grid) {
  report_plan_heads("nts_gather_plan_heads_bf16", sizeof(uint16_t),
                    feature_size, heads, alignment_bytes, batch_size, edges,
                    lane_group, vector_width, grid);
}

void nts_reduce_by_dst_from_src(nts_stream *s, int op, const float *input,
                                float *output, nts_vid *arg,
                                const nts_vid *row_indices,
                                const nts_vid *column_offset, nts_vid src_start,
                                nts_vid src_end, nts_vid dst_start,
                                nts_vid dst_end, nts_vid edges,
                                nts_vid batch_size, nts_vid feature_size) {
  (void)src_end; (void)dst_start; (void)dst_end;
  launch_reduce(s, op, input, output, arg, row_indices, column_offset,
                src_start, batch_size, edges, feature_size);
}

void nts_reduce_backward(nts_stream *s, const float *grad_output,
                         const nts_vid *arg, const nts_vid *row_indices,
                         nts_vid src_start, float *grad_input,
                         nts_vid batch_size, nts_vid feature_size) {
  const uint64_t n = (uint64_t)batch_size * feature_size;
  if (!n) return;
  Tic t(s, NTS_KTAG_BWD);
  hipLaunchKernelGGL(k_reduce_backward, dim3(grid_for(n)), dim3(NTS_BLOCK), 0,
                     s->stream, grad_output, arg, row_indices, src_start,
                     grad_input, n, feature_size);
  dbg_sync(s, "k_reduce_backward");
}

void nts_reduce_plan(nts_vid feature_size, unsigned alignment_bytes,
                     nts_vid batch_size, nts_vid edges, int *lane_group,
                     int *vector_width, int *grid,
                     unsigned long long *scratch_bytes) {
  const ReduceLaunch R = plan_reduce(feature_size, alignment_bytes, batch_size,
                                     edges, gather_env());
  if (lane_group) *lane_group = (int)R.L.G;
  if (vector_width) *vector_width = R.L.elem;
  if (grid) *grid = (int)R.L.grid;
  if (scratch_bytes) *scratch_bytes = R.key_elems * sizeof(unsigned long long);
}

void nts_gather_schedule(nts_stream *s, int schedule, int window_floats) {
  s->sched_req = schedule;
  s->window_req = window_floats;
}

void nts_gather_schedule_last(nts_stream *s, int *schedule,
                              int *window_floats) {
  if (schedule) *schedule = s->sched_last;
  if (window_floats) *window_floats = s->window_last;
}

static void report_plan(uint32_t elem_bytes, nts_vid feature_size,
                        unsigned alignment_bytes, nts_vid rows,
                        nts_vid batch_size, nts_vid edges, int schedule_req,
                        int window_req, int *schedule, int *window_floats,
                        int *lane_group, int *vector_width, int *grid,
                        int *blocked) {
  GatherLaunch L{};
  if (batch_size && edges && feature_size) /* else nothing is launched */
    L = plan_gather(feature_size, alignment_bytes, elem_bytes, rows,
                    batch_size, edges, schedule_req, window_req, gather_env());
  if (schedule) *schedule = (int)L.pl.sched;
  if (window_floats) *window_floats = (int)L.pl.wf;
  if (lane_group) *lane_group = (int)L.G;
  if (vector_width) *vector_width = L.elem;
  if (grid) *grid = (int)L.grid;
  if (blocked) *blocked = L.blocked ? 1 : 0;
}

void nts_gather_plan(nts_vid feature_size, unsigned alignment_bytes,
                     nts_vid rows, nts_vid batch_size, nts_vid edges,
                     int schedule_req, int window_req, int *schedule,
                     int *window_floats, int *lane_group, int *vector_width,
                     int *grid, int *blocked) {
  report_plan(sizeof(float), feature_size, alignment_bytes, rows, batch_size,
              edges, schedule_req, window_req, schedule, window_floats,
              lane_group, vector_width, grid, blocked);
}

void nts_gather_plan_bf16(nts_vid feature_size, unsigned alignment_bytes,
                          nts_vid rows, nts_vid batch_size, nts_vid edges,
                          int schedule_req, int window_req, int *schedule,
                          int *window_floats, int *lane_group,
                          int *vector_width, int *grid, int *blocked) {
  report_plan(sizeof(uint16_t), feature_size, alignment_bytes, rows,
              batch_size, edges, schedule_req, window_req, schedule,
              window_floats, lane_group, vector_width, grid, blocked);
}

void nts_gather_staging(nts_stream *s, int mode) {
  s->stage_req = mode > 0 ? 1 : mode < 0 ? -1 : 0;
}

void nts_gather_staging_last(nts_stream *s, int *staged, int *pitch_floats) {
  if (staged) *staged = s->staged_last ? 1 : 0;
  if (pitch_floats) *pitch_floats = (int)s->stage_ld_last;
}

void nts_gather_stage_plan(nts_vid feature_size, unsigned elem_bytes,
                           unsigned in_alignment_bytes,
                           unsigned out_alignment_bytes, nts_vid rows,
                           nts_vid batch_size, nts_vid edges, int schedule_req,
                           int window_req, int stage_req, int *staged,
                           int *pitch_floats, int *schedule,
                           int *window_floats, int *lane_group,
                           int *vector_width, int *store_width, int *grid,
                           int *blocked) {
  StagePlan P{};
  if (batch_size && edges && feature_size) /* else nothing is launched */
    P = plan_stage(feature_size, elem_bytes, in_alignment_bytes,
                   out_alignment_bytes, rows, batch_size, edges, schedule_req,
                   window_req, stage_req, gather_env());
  if (staged) *staged = P.staged ? 1 : 0;
  if (pitch_floats) *pitch_floats = (int)P.ld;
  if (schedule) *schedule = (int)P.L.pl.sched;
  if (window_floats) *window_floats = (int)P.L.pl.wf;
  if (lane_group) *lane_group = (int)P.L.G;
  if (vector_width) *vector_width = P.L.elem;
  if (store_width) *store_width = P.ov;
  if (grid) *grid = (int)P.L.grid;
  if (blocked) *blocked = P.L.blocked ? 1 : 0;
}

void nts_gather_stripes(nts_stream *s, int stripe_floats) {
  s->stripe_req = stripe_floats < 0 ? -1 : stripe_floats;
}

void nts_gather_stripes_run(nts_stream *s, int tasks_per_wave) {
  s->stripe_run_req = tasks_per_wave > 0 ? tasks_per_wave : 0;
}

void nts_gather_stripes_last(nts_stream *s, int *stripe_floats,
                             int *tasks_per_wave) {
  if (stripe_floats) *stripe_floats = (int)s->stripe_last;
  if (tasks_per_wave) *tasks_per_wave = (int)s->stripe_run_last;
}

/* the stage plan plus the stripe decision of the same arguments */
static StripeLaunch stripe_plan_of(nts_vid feature_size, unsigned elem_bytes,
                                   unsigned in_alignment_bytes,
                                   unsigned out_alignment_bytes, nts_vid rows,
                                   nts_vid batch_size, nts_vid edges,
                                   int schedule_req, int window_req,
                                   int stage_req, int stripe_req, int run_req,
                                   StagePlan &P) {
  P = StagePlan{};
  if (!batch_size || !edges || !feature_size) /* nothing is launched */
    return StripeLaunch{};
  P = plan_stage(feature_size, elem_bytes, in_alignment_bytes,
                 out_alignment_bytes, rows, batch_size, edges, schedule_req,
                 window_req, stage_req, gather_env());
  return plan_stripe(P, feature_size, elem_bytes, batch_size, edges,
                     schedule_req, window_req, stage_req, stripe_req, run_req,
                     gather_env());
}

void nts_gather_stripe_plan(nts_vid feature_size, unsigned elem_bytes,
                            unsigned in_alignment_bytes,
                            unsigned out_alignment_bytes, nts_vid rows,
                            nts_vid batch_size, nts_vid edges, int schedule_req,
                            int window_req, int stage_req, int stripe_req,
                            int run_req, int *staged, int *pitch_floats,
                            int *schedule, int *window_floats, int *lane_group,
                            int *vector_width, int *store_width, int *grid,
                            int *blocked, int *stripe_floats,
                            int *stripe_lanes, int *subgroups, int *stripes,
                            int *tasks_per_wave) {
  StagePlan P;
  const StripeLaunch SL = stripe_plan_of(
      feature_size, elem_bytes, in_alignment_bytes, out_alignment_bytes, rows,
      batch_size, edges, schedule_req, window_req, stage_req, stripe_req,
      run_req, P);
  if (staged) *staged = P.staged ? 1 : 0;
  if (pitch_floats) *pitch_floats = (int)P.ld;
  if (schedule) *schedule = SL.on ? (int)NTS_SCHED_PHASE : (int)P.L.pl.sched;
  if (window_floats) *window_floats = (int)(SL.on ? SL.sp.wf : P.L.pl.wf);
  if (lane_group) *lane_group = (int)(SL.on ? SL.Gs : P.L.G);
  if (vector_width) *vector_width = P.L.elem;
  if (store_width) *store_width = P.ov;
  if (grid) *grid = (int)(SL.on ? SL.grid : P.L.grid);
  if (blocked) *blocked = (SL.on || P.L.blocked) ? 1 : 0;
  if (stripe_floats) *stripe_floats = (int)SL.sp.sf;
  if (stripe_lanes) *stripe_lanes = (int)SL.Gs;
  if (subgroups) *subgroups = (int)SL.P;
  if (stripes) *stripes = (int)SL.sp.S;
  if (tasks_per_wave) *tasks_per_wave = (int)SL.sp.R;
}

long long nts_gather_stripe_task(
    nts_vid feature_size, unsigned elem_bytes, unsigned in_alignment_bytes,
    unsigned out_alignment_bytes, nts_vid rows, nts_vid batch_size,
    nts_vid edges, int schedule_req, int window_req, int stage_req,
    int stripe_req, int run_req, nts_vid n_items, unsigned long long first_slot,
    unsigned long long count, nts_vid *item, nts_vid *first_column,
    nts_vid *column_bound) {
  StagePlan P;
  const StripeLaunch SL = stripe_plan_of(
      feature_size, elem_bytes, in_alignment_bytes, out_alignment_bytes, rows,
      batch_size, edges, schedule_req, window_req, stage_req, stripe_req,
      run_req, P);
  long long live = 0;
  constexpr uint32_t WAVES = NTS_BLOCK / 64;
  for (unsigned long long k = 0; k < count; ++k) {
    Task tk{0u, 0u, 0u};
    if (SL.on) {
      const unsigned long long slot = first_slot + k;
      const unsigned long long w = slot / SL.sp.R;
      if (w / WAVES < SL.grid)
        tk = stripe_task(SL.grid, n_items, feature_size, SL.sp,
                         (uint32_t)(w / WAVES), (uint32_t)(w % WAVES),
                         (uint32_t)(slot % SL.sp.R));
    }
    if (item) item[k] = tk.it;
    if (first_column) first_column[k] = tk.fbase;
    if (column_bound) column_bound[k] = tk.fend;
    live += tk.fbase < tk.fend;
  }
  return live;
}

void nts_items_cache_clear(nts_stream *s) {
  NTS_CHECK(hipStreamSynchronize(s->stream));
  for (auto &slot : s->items_scratch) slot.valid = false;
}

void nts_items_reuse(nts_stream *s, int enable) {
  if (!enable) nts_items_cache_clear(s);
  s->items_reuse = enable != 0;
}

void nts_deserialize_to_gpu(nts_stream *s, float *gpu_buffer, const float *msg,
                            nts_vid count, nts_vid feature_size,
                            nts_vid partition_start, nts_vid partition_end,
                            int sync) {
  (void)partition_end;
  if (count) {
    Tic t(s, NTS_KTAG_DESER);
    hipLaunchKernelGGL(k_deserialize,
                       dim3(grid_for((uint64_t)count * feature_size)),
                       dim3(NTS_BLOCK), 0, s->stream, msg, count,
                       partition_start, gpu_buffer, feature_size);
  }
  if (sync) NTS_CHECK(hipStreamSynchronize(s->stream));
}

void nts_aggregate_comm_result(nts_stream *s, float *master, const float *msg,
                               nts_vid count, nts_vid feature_size,
                               nts_vid partition_start, nts_vid partition_end,
                               int sync) {
  (void)partition_end;
  if (count) {
    Tic t(s, NTS_KTAG_AGGMSG);
    hipLaunchKernelGGL(k_agg_msg,
                       dim3(grid_for((uint64_t)count * feature_size)),
                       dim3(NTS_BLOCK), 0, s->stream, master, msg, count,
                       partition_start, feature_size);
  }
  if (sync) NTS_CHECK(hipStreamSynchronize(s->stream));
}

void nts_gather_rows(nts_stream *s, const float *dense, float *packed,
                     const nts_vid *index, nts_vid count, nts_vid row_start,
                     nts_vid feature_size) {
  if (!count) return;
  hipLaunchKernelGGL((k_rows<ROW_GATHER>),
                     dim3(grid_for((uint64_t)count * feature_size)),
                     dim3(NTS_BLOCK), 0, s->stream, const_cast<float *>(dense),
                     packed, index, count, row_start, feature_size);
}

void nts_scatter_rows(nts_stream *s, float *dense, const float *packed,
                      const nts_vid *index, nts_vid count, nts_vid row_start,
                      nts_vid feature_size) {
  if (!count) return;
  hipLaunchKernelGGL((k_rows<ROW_SCATTER>),
                     dim3(grid_for((uint64_t)count * feature_size)),
                     dim3(NTS_BLOCK), 0, s->stream, dense,
                     const_cast<float *>(packed), index, count, row_start,
                     feature_size);
}

void nts_scatter_add_rows(nts_stream *s, float *dense, const float *packed,
                          const nts_vid *index, nts_vid count,
                          nts_vid row_start, nts_vid feature_size) {
  if (!count) return;
  hipLaunchKernelGGL((k_rows<ROW_SCATTER_ADD>),
                     dim3(grid_for((uint64_t)count * feature_size)),
                     dim3(NTS_BLOCK), 0, s->stream, dense,
                     const_cast<float *>(packed), index, count, row_start,
                     feature_size);
}

static uint32_t read_edge_count(nts_stream *s, const nts_vid *column_offset,
                                nts_vid batch) {
  uint32_t last = 0;
  NTS_CHECK(hipMemcpyAsync(&last, column_offset + batch, sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s->stream));
  NTS_CHECK(hipStreamSynchronize(s->stream));
  return last;
}

/* Prologue of the item-driven edge entry points: the edge count (one host
 * sync), the work items and the grid.  ib == nullptr: nothing to do. */
struct EdgeItems {
  ItemsBuf *ib = nullptr;
  uint32_t edges = 0, grid = 0;
};
static EdgeItems edge_items(nts_stream *s, const nts_vid *offset,
                            nts_vid batch) {
  EdgeItems p;
  if (!batch) return p;
  p.edges = read_edge_count(s, offset, batch);
  if (!p.edges) return p;
  p.ib = &get_items(s, offset, batch, p.edges);
  p.grid = items_grid(batch, p.edges);
  return p;
}

static float *get_sums(nts_stream *s, uint64_t n) {
  if (s->sums_cap < n) {
    NTS_CHECK(hipStreamSynchronize(s->stream));
    if (s->sums_ws) NTS_CHECK(hipFree(s->sums_ws));
    NTS_CHECK(hipMalloc(&s->sums_ws, n * sizeof(float)));
    s->sums_cap = n;
  }
  NTS_CHECK(hipMemsetAsync(s->sums_ws, 0, n * sizeof(float), s->stream));
  return s->sums_ws;
}

/* the stable softmax's (max, sum) pairs; all-zero = empty */
static unsigned long long *get_pairs(nts_stream *s, uint64_t n) {
  if (s->pairs_cap < n) {
    NTS_CHECK(hipStreamSynchronize(s->stream));
    if (s->pairs_ws) NTS_CHECK(hipFree(s->pairs_ws));
    NTS_CHECK(hipMalloc(&s->pairs_ws, n * sizeof(unsigned long long)));
    s->pairs_cap = n;
  }
  NTS_CHECK(hipMemsetAsync(s->pairs_ws, 0, n * sizeof(unsigned long long),
                           s->stream));
  return s->pairs_ws;
}

void nts_edge_softmax_stable(nts_stream *s, int enable) {
  s->softmax_stable = enable != 0;
}

void nts_edge_softmax_stable_last(nts_stream *s, int *stable) {
  if (stable) *stable = s->softmax_stable_last ? 1 : 0;
}

/* the FLAT layout takes K a power of two <= 64 */
static bool heads_flat(const nts_stream *s, uint32_t K) {
  return !s->heads_general && K <= 64 && (K & (K - 1)) == 0;
}

extern "C++" { /* a template cannot have the C linkage of this block */
/* one k_edge_reduce pass in a given lane layout ... */
template <bool FLAT, int KC, class Value, class Reduce>
static void launch_reduce_as(nts_stream *s, const EdgeItems &p, uint32_t K,
                             const Value &val, const Reduce &red) {
  hipLaunchKernelGGL((k_edge_reduce<FLAT, KC, Value, Reduce>), dim3(p.grid),
                     dim3(NTS_BLOCK), 0, s->stream, p.ib->items,
                     p.ib->counter, val, red, K);
}
/* ... and in the layout heads_flat() picks; one column has one layout */
template <class Value, class Reduce>
static void launch_reduce(nts_stream *s, const EdgeItems &p, uint32_t K,
                          const Value &val, const Reduce &red) {
  if (K == 1) launch_reduce_as<false, 1>(s, p, K, val, red);
  else if (heads_flat(s, K)) launch_reduce_as<true, 0>(s, p, K, val, red);
  else launch_reduce_as<false, 0>(s, p, K, val, red);
}
}  // extern "C++"

/* the per-destination scratch of a softmax forward: sums (default) or pairs
 * (stable), the other null */
struct SoftmaxScratch {
  float *sums = nullptr;
  unsigned long long *pairs = nullptr;
};
static SoftmaxScratch softmax_scratch(nts_stream *s, uint64_t n) {
  SoftmaxScratch ws;
  if (s->softmax_stable) ws.pairs = get_pairs(s, n);
  else ws.sums = get_sums(s, n);
  return ws;
}

extern "C++" {
template <NormMode MODE>
static void launch_norm(nts_stream *s, const EdgeItems &p, float *out,
                        const float *cached, const NormSlot<MODE> *slots,
                        float *out2, const nts_vid *pos2, nts_vid f,
                        const float *lrelu_in = nullptr, float slope = 0.f,
                        float *dst_accum = nullptr) {
  hipLaunchKernelGGL(k_edge_softmax_norm<MODE>, dim3(p.grid), dim3(NTS_BLOCK),
                     0, s->stream, p.ib->items, p.ib->counter, out, cached,
                     slots, out2, pos2, lrelu_in, slope, dst_accum, f);
}
/* the forward modes under attention dropout: out = the softmax, emit.w_out
 * and out2 = the dropped weights */
template <NormMode MODE>
static void launch_norm_drop(nts_stream *s, const EdgeItems &p, float *out,
                             const NormSlot<MODE> *slots, float *out2,
                             const nts_vid *pos2, nts_vid f,
                             const NormEmitDropped &emit) {
  hipLaunchKernelGGL((k_edge_softmax_norm<MODE, NormEmitDropped>),
                     dim3(p.grid), dim3(NTS_BLOCK), 0, s->stream, p.ib->items,
                     p.ib->counter, out, (const float *)nullptr, slots, out2,
                     pos2, (const float *)nullptr, 0.f, (float *)nullptr, f,
                     emit);
}
}  // extern "C++"

/* what follows pass 1 of a softmax or attention forward: the split items'
 * sum pass (stable only), then the normalize pass.  drop: out keeps the
 * softmax, drop->w_out and out2 get the dropped weights. */
static void launch_softmax_tail(nts_stream *s, const EdgeItems &p, float *out,
                                const SoftmaxScratch &ws, float *out2,
                                const nts_vid *pos2, nts_vid f,
                                const NormEmitDropped *drop = nullptr) {
  if (ws.pairs) {
    launch_reduce(s, p, f, EdgeStashExp{out, ws.pairs, 0.f},
                  SplitSumToPairs{ws.pairs});
    if (drop)
      launch_norm_drop<NORM_STABLE>(s, p, out, ws.pairs, out2, pos2, f, *drop);
    else
      launch_norm<NORM_STABLE>(s, p, out, nullptr, ws.pairs, out2, pos2, f);
  } else if (drop) {
    launch_norm_drop<NORM_FWD>(s, p, out, ws.sums, out2, pos2, f, *drop);
  } else {
    launch_norm<NORM_FWD>(s, p, out, nullptr, ws.sums, out2, pos2, f);
  }
}

static void launch_edge_op(nts_stream *s, EdgeOp op, float *message,
                           float *vfeat, const nts_vid *row_indices,
                           const nts_vid *column_offset,
                           const nts_vid *mirror_index, nts_vid batch,
                           nts_vid f) {
  if (!f) return;
  const EdgeItems p = edge_items(s, column_offset, batch);
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  static constexpr decltype(&k_edge_items<E_SCATTER_SRC>) kernels[] = {
      k_edge_items<E_SCATTER_SRC>, k_edge_items<E_GATHER_SRC>,
      k_edge_items<E_SCATTER_DST>, k_edge_items<E_GATHER_DST>,
      k_edge_items<E_SCATTER_GRAD>}; /* in EdgeOp order */
  hipLaunchKernelGGL(kernels[op], dim3(p.grid), dim3(NTS_BLOCK), 0, s->stream,
                     p.ib->items, p.ib->counter, message, vfeat, row_indices,
                     mirror_index, f);
  dbg_sync(s, "k_edge_items");
}

/* Edge softmax, two item-parallel passes over the items of p (p.ib set):
 * pass 1 stashes exp(in) (forward) or g*s (backward) in out and reduces
 * per-destination sums, pass 2 normalizes.  Strided walk at every f. */
static void softmax_forward_passes(nts_stream *s, const EdgeItems &p,
                                   float *out, const float *in, nts_vid batch,
                                   nts_vid f, float *out2, const nts_vid *pos2,
                                   const NormEmitDropped *drop = nullptr) {
  const SoftmaxScratch ws = softmax_scratch(s, (uint64_t)batch * f);
  Tic t(s, NTS_KTAG_EDGE);
  if (ws.pairs)
    launch_reduce_as<false, 0>(s, p, f, EdgeIn{in},
                               MaxSumToPairs{out, ws.pairs});
  else
    launch_reduce_as<false, 0>(s, p, f, EdgeIn{in},
                               SumToSums<true>{out, ws.sums});
  launch_softmax_tail(s, p, out, ws, out2, pos2, f, drop);
  dbg_sync(s, "k_edge_softmax");
}

/* drop: in is the gradient of the dropped weights (EdgeInCachedDrop) */
static void softmax_backward_passes(nts_stream *s, const EdgeItems &p,
                                    float *out, const float *in,
                                    const float *cached, nts_vid batch,
                                    nts_vid f, float *out2,
                                    const nts_vid *pos2, const float *lrelu_in,
                                    float slope, float *dst_accum,
                                    const DropMask *drop = nullptr) {
  float *sums = get_sums(s, (uint64_t)batch * f);
  Tic t(s, NTS_KTAG_EDGE);
  if (drop)
    launch_reduce_as<false, 0>(s, p, f, EdgeInCachedDrop{in, cached, *drop},
                               SumToSums<false>{out, sums});
  else
    launch_reduce_as<false, 0>(s, p, f, EdgeInCached{in, cached},
                               SumToSums<false>{out, sums});
  launch_norm<NORM_BWD>(s, p, out, cached, sums, out2, pos2, f, lrelu_in,
                        slope, dst_accum);
  dbg_sync(s, "k_edge_softmax_backward");
}

/* The entries that read the edge count from the device.  Returns that count
 * (0: nothing ran). */
static uint32_t launch_edge_softmax(nts_stream *s, bool backward, float *out,
                                    const float *in, const float *cached,
                                    const nts_vid *column_offset,
                                    nts_vid batch, nts_vid f,
                                    float *out2 = nullptr,
                                    const nts_vid *pos2 = nullptr,
                                    const float *lrelu_in = nullptr,
                                    float slope = 0.f,
                                    float *dst_accum = nullptr) {
  if (dst_accum && f != 1) abort(); /* per-dst sum emission is f==1 only */
  if (!backward) s->softmax_stable_last = s->softmax_stable;
  if (!f) return 0;
  const EdgeItems p = edge_items(s, column_offset, batch);
  if (!p.ib) return 0;
  if (backward)
    softmax_backward_passes(s, p, out, in, cached, batch, f, out2, pos2,
                            lrelu_in, slope, dst_accum);
  else
    softmax_forward_passes(s, p, out, in, batch, f, out2, pos2);
  return p.edges;
}

void nts_scatter_src_mirror_to_msg(nts_stream *s, float *message,
                                   const float *src_mirror_feature,
                                   const nts_vid *row_indices,
                                   const nts_vid *column_offset,
                                   const nts_vid *mirror_index,
                                   nts_vid batch_size, nts_vid feature_size) {
  launch_edge_op(s, E_SCATTER_SRC, message,
                 const_cast<float *>(src_mirror_feature), row_indices,
                 column_offset, mirror_index, batch_size, feature_size);
}

void nts_gather_msg_to_src_mirror(nts_stream *s, float *src_mirror_feature,
                                  const float *message,
                                  const nts_vid *row_indices,
                                  const nts_vid *column_offset,
                                  const nts_vid *mirror_index,
                                  nts_vid batch_size, nts_vid feature_size) {
  launch_edge_op(s, E_GATHER_SRC, const_cast<float *>(message),
                 src_mirror_feature, row_indices, column_offset, mirror_index,
                 batch_size, feature_size);
}

void nts_scatter_dst_to_msg(nts_stream *s, float *message,
                            const float *dst_feature,
                            const nts_vid *row_indices,
                            const nts_vid *column_offset, nts_vid batch_size,
                            nts_vid feature_size) {
  launch_edge_op(s, E_SCATTER_DST, message, const_cast<float *>(dst_feature),
                 row_indices, column_offset, nullptr, batch_size, feature_size);
}

void nts_gather_msg_to_dst(nts_stream *s, float *dst_feature,
                           const float *message, const nts_vid *row_indices,
                           const nts_vid *column_offset, nts_vid batch_size,
                           nts_vid feature_size) {
  launch_edge_op(s, E_GATHER_DST, const_cast<float *>(message), dst_feature,
                 row_indices, column_offset, nullptr, batch_size, feature_size);
}

void nts_edge_dot(nts_stream *s, float *out, const float *dst_rows,
                  const float *src_rows, const nts_vid *row_indices,
                  const nts_vid *column_offset, nts_vid src_start,
                  nts_vid batch_size, nts_vid feature_size) {
  if (!feature_size) return;
  const EdgeItems p = edge_items(s, column_offset, batch_size);
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  hipLaunchKernelGGL(k_edge_dot, dim3(p.grid), dim3(NTS_BLOCK), 0, s->stream,
                     p.ib->items, p.ib->counter, out, dst_rows, src_rows,
                     row_indices, src_start, feature_size);
  dbg_sync(s, "k_edge_dot");
}

void nts_scatter_grad_back_to_message(nts_stream *s, const float *input_grad,
                                      float *message_grad,
                                      const nts_vid *row_indices,
                                      const nts_vid *column_offset,
                                      nts_vid batch_size,
                                      nts_vid feature_size) {
  launch_edge_op(s, E_SCATTER_GRAD, message_grad,
                 const_cast<float *>(input_grad), row_indices, column_offset,
                 nullptr, batch_size, feature_size);
}

void nts_edge_softmax_forward(nts_stream *s, float *msg_output,
                              const float *msg_input, float *msg_cached,
                              const nts_vid *row_indices,
                              const nts_vid *column_offset, nts_vid batch_size,
                              nts_vid feature_size) {
  (void)row_indices;
  nts_edge_softmax_forward_dual(s, msg_output, nullptr, nullptr, msg_input,
                                msg_cached, column_offset, batch_size,
                                feature_size);
}

void nts_edge_softmax_backward(nts_stream *s, float *msg_input_grad,
                               const float *msg_output_grad,
                               const float *msg_cached,
                               const nts_vid *row_indices,
                               const nts_vid *column_offset,
                               nts_vid batch_size, nts_vid feature_size) {
  (void)row_indices;
  launch_edge_softmax(s, true, msg_input_grad, msg_output_grad, msg_cached,
                      column_offset, batch_size, feature_size);
}

/* ---- GAT fusion entry points (additive; see include/nts_hip.h) ---- */

void nts_edge_softmax_forward_dual(nts_stream *s, float *msg_output,
                                   float *msg_output_perm,
                                   const nts_vid *perm_pos,
                                   const float *msg_input, float *msg_cached,
                                   const nts_vid *column_offset,
                                   nts_vid batch_size, nts_vid feature_size) {
  const uint32_t edges =
      launch_edge_softmax(s, false, msg_output, msg_input, nullptr,
                          column_offset, batch_size, feature_size,
                          msg_output_perm, perm_pos);
  /* cache = output for backward (reference caches at
   * ntsCUDADistKernel.cuh:210) */
  const uint64_t n = (uint64_t)edges * feature_size;
  if (n && msg_cached && msg_cached != msg_output)
    hipLaunchKernelGGL(k_copy, dim3(grid_for(n)), dim3(NTS_BLOCK), 0,
                       s->stream, msg_cached, msg_output, n);
}

void nts_edge_softmax_backward_fused(nts_stream *s, float *msg_input_grad,
                                     float *msg_input_grad_perm,
                                     const nts_vid *perm_pos,
                                     const float *msg_output_grad,
                                     const float *msg_cached,
                                     const float *lrelu_input, float slope,
                                     float *dst_sum,
                                     const nts_vid *column_offset,
                                     nts_vid batch_size, nts_vid feature_size) {
  launch_edge_softmax(s, true, msg_input_grad, msg_output_grad, msg_cached,
                      column_offset, batch_size, feature_size,
                      msg_input_grad_perm, perm_pos, lrelu_input, slope,
                      dst_sum);
}

/* ---- attention and multi-head entries (additive; see include/nts_hip.h) ----
 * A one-column entry is its heads entry at K = 1 behind the other prologue. */

/* Prologue of the heads edge entries: as edge_items, with the edge count
 * from the caller — no device-to-host copy, no stream synchronize. */
static EdgeItems edge_items_known(nts_stream *s, const nts_vid *offset,
                                  nts_vid batch, nts_vid edges) {
  EdgeItems p;
  if (!batch || !edges) return p;
  p.edges = edges;
  p.ib = &get_items(s, offset, batch, edges);
  p.grid = items_grid(batch, edges);
  return p;
}

void nts_heads_dbg_general(nts_stream *s, int enable) {
  s->heads_general = enable != 0;
}

/* Pass 1 fuses the score, the activation, the exp and the per-destination
 * sums; pass 2 is the softmax's normalize (dual-order emission). */
static void attention_forward(nts_stream *s, const EdgeItems &p, nts_vid K,
                              nts_vid batch, float *softmax_out,
                              float *softmax_out_perm, const nts_vid *perm_pos,
                              const EdgeScore &score,
                              const NormEmitDropped *drop = nullptr) {
  s->softmax_stable_last = s->softmax_stable;
  if (!p.ib) return;
  const SoftmaxScratch ws = softmax_scratch(s, (uint64_t)batch * K);
  Tic t(s, NTS_KTAG_EDGE);
  if (ws.pairs)
    launch_reduce(s, p, K, score, MaxSumToPairs{softmax_out, ws.pairs});
  else
    launch_reduce(s, p, K, score, SumToSums<true>{softmax_out, ws.sums});
  launch_softmax_tail(s, p, softmax_out, ws, softmax_out_perm, perm_pos, K,
                      drop);
  dbg_sync(s, "k_edge_att");
}

void nts_edge_attention_forward(nts_stream *s, float *softmax_out,
                                float *softmax_out_perm,
                                const nts_vid *perm_pos, float *m_sum_out,
                                const float *s_src_mirror, const float *s_dst,
                                const nts_vid *row_indices,
                                const nts_vid *mirror_index, float slope,
                                const nts_vid *column_offset,
                                nts_vid batch_size) {
  attention_forward(s, edge_items(s, column_offset, batch_size), 1, batch_size,
                    softmax_out, softmax_out_perm, perm_pos,
                    EdgeScore{m_sum_out, s_src_mirror, s_dst, row_indices,
                              mirror_index, slope, 0.f});
}

void nts_edge_attention_forward_heads(
    nts_stream *s, float *softmax_out, float *softmax_out_perm,
    const nts_vid *perm_pos, float *m_sum_out, const float *s_src_mirror,
    const float *s_dst, const nts_vid *row_indices,
    const nts_vid *mirror_index, float slope, const nts_vid *column_offset,
    nts_vid batch_size, nts_vid edges, nts_vid heads) {
  check_heads("nts_edge_attention_forward_heads", heads, heads);
  attention_forward(s, edge_items_known(s, column_offset, batch_size, edges),
                    heads, batch_size, softmax_out, softmax_out_perm, perm_pos,
                    EdgeScore{m_sum_out, s_src_mirror, s_dst, row_indices,
                              mirror_index, slope, 0.f});
}

/* ---- fused inference forward (additive; see include/nts_hip.h) ---- */
extern "C++" {
template <typename T, bool STABLE, bool MIRROR>
static void launch_gather_att(nts_stream *s, const EdgeItems &p,
                              const GatherLaunch &L, const AttSrc &at,
                              const T *in, float *out, const nts_vid *nbr,
                              nts_vid nbr_start, nts_vid f, nts_vid K) {
  /* indexed by log2(elements per lane); the last entry is the widest lane:
   * 4 dwords, or 8 bf16 */
  constexpr int WIDEST = 16 / (int)sizeof(T);
  static const decltype(&k_gather_att_heads<1, T, STABLE, MIRROR>) kernels[4] =
      {k_gather_att_heads<1, T, STABLE, MIRROR>,
       k_gather_att_heads<2, T, STABLE, MIRROR>,
       k_gather_att_heads<4, T, STABLE, MIRROR>,
       k_gather_att_heads<WIDEST, T, STABLE, MIRROR>};
  hipLaunchKernelGGL(kernels[__builtin_ctz((unsigned)L.elem)], dim3(L.grid),
                     dim3(NTS_BLOCK), 0, s->stream, p.ib->items, p.ib->counter,
                     nbr, at, in, out, nbr_start, f, L.G, L.pl.n_windows, K,
                     f / K);
}

/* Pass 1 under NTS_KTAG_EDGE: the denominators, nothing per edge; pass 2
 * under NTS_KTAG_FWD: the heads gather's launch with the weights computed in
 * registers.  Both walk the one item decomposition of column_offset. */
template <typename T>
static void gat_forward_fused(nts_stream *s, const char *entry, const T *in,
                              float *out, const EdgeScoreOnly &score,
                              const nts_vid *offset, nts_vid nbr_start,
                              nts_vid batch, nts_vid edges, nts_vid f,
                              nts_vid K) {
  check_heads(entry, f, K);
  s->softmax_stable_last = s->softmax_stable;
  const EdgeItems p = edge_items_known(s, offset, batch, edges);
  if (!p.ib) return;
  const SoftmaxScratch ws = softmax_scratch(s, (uint64_t)batch * K);
  {
    Tic t(s, NTS_KTAG_EDGE);
    if (ws.pairs) {
      launch_reduce(s, p, K, score, MaxSumOnlyToPairs{ws.pairs});
      launch_reduce(s, p, K, EdgeScoreExp{score, ws.pairs, 0.f},
                    SplitSumToPairs{ws.pairs});
    } else {
      launch_reduce(s, p, K, score, ExpSumToSums{ws.sums});
    }
    dbg_sync(s, "k_edge_reduce (fused forward)");
  }
  const GatherLaunch L = plan_gather_heads(
      f, K, (uintptr_t)in | (uintptr_t)out, batch, edges, gather_env(),
      sizeof(T));
  s->sched_last = (int)L.pl.sched;
  s->window_last = (int)L.pl.wf;
  s->stripe_last = s->stripe_run_last = 0;
  const AttSrc at{score.s_src, score.s_dst, score.mirror_index,
                  ws.pairs ? (const void *)ws.pairs : (const void *)ws.sums,
                  score.slope};
  Tic t(s, NTS_KTAG_FWD);
  static constexpr decltype(&launch_gather_att<T, false, false>) launch[2][2] =
      {{launch_gather_att<T, false, false>, launch_gather_att<T, false, true>},
       {launch_gather_att<T, true, false>, launch_gather_att<T, true, true>}};
  launch[ws.pairs != nullptr][at.mirror_index != nullptr](
      s, p, L, at, in, out, score.row_indices, nbr_start, f, K);
  dbg_sync(s, "k_gather_att_heads");
}
}  // extern "C++"

void nts_gat_forward_fused(nts_stream *s, const float *input, float *output,
                           const float *s_src_mirror, const float *s_dst,
                           const nts_vid *row_indices,
                           const nts_vid *mirror_index, float slope,
                           const nts_vid *column_offset, nts_vid src_start,
                           nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
                           nts_vid edges, nts_vid batch_size,
                           nts_vid feature_size, nts_vid heads) {
  (void)src_end; (void)dst_start; (void)dst_end;
  gat_forward_fused(s, "nts_gat_forward_fused", input, output,
                    EdgeScoreOnly{s_src_mirror, s_dst, row_indices,
                                  mirror_index, slope, 0.f},
                    column_offset, src_start, batch_size, edges, feature_size,
                    heads);
}

void nts_gat_forward_fused_bf16(
    nts_stream *s, const uint16_t *input, float *output,
    const float *s_src_mirror, const float *s_dst, const nts_vid *row_indices,
    const nts_vid *mirror_index, float slope, const nts_vid *column_offset,
    nts_vid src_start, nts_vid src_end, nts_vid dst_start, nts_vid dst_end,
    nts_vid edges, nts_vid batch_size, nts_vid feature_size, nts_vid heads) {
  (void)src_end; (void)dst_start; (void)dst_end;
  gat_forward_fused(s, "nts_gat_forward_fused_bf16", input, output,
                    EdgeScoreOnly{s_src_mirror, s_dst, row_indices,
                                  mirror_index, slope, 0.f},
                    column_offset, src_start, batch_size, edges, feature_size,
                    heads);
}

/* ---- attention dropout entries (additive; see include/nts_hip.h) ---- */

/* the mask constants of (p, seed); p outside [0, 1) aborts (error culture of
 * the header: the bindings check first) */
static DropMask drop_mask(const char *entry, float p,
                          unsigned long long seed) {
  if (!(p >= 0.f && p < 1.f)) {
    fprintf(stderr, "%s: dropout probability %g is not in [0, 1)\n", entry,
            (double)p);
    abort();
  }
  return DropMask{drop_fmix64(seed), (uint32_t)lrintf(p * 16777216.0f),
                  1.0f / (1.0f - p)};
}

void nts_edge_dropout_keep(unsigned long long seed, float p,
                           unsigned long long first, unsigned long long count,
                           uint8_t *keep) {
  const DropMask dm = drop_mask("nts_edge_dropout_keep", p, seed);
  for (unsigned long long j = 0; j < count; ++j)
    keep[j] = drop_keep(dm, first + j) ? 1 : 0;
}

void nts_edge_attention_forward_drop(
    nts_stream *s, float *softmax_out, float *softmax_out_perm,
    const nts_vid *perm_pos, float *m_sum_out, const float *s_src_mirror,
    const float *s_dst, const nts_vid *row_indices,
    const nts_vid *mirror_index, float slope, const nts_vid *column_offset,
    nts_vid batch_size, nts_vid edges, nts_vid heads, float *alpha_out,
    float p, unsigned long long seed) {
  check_heads("nts_edge_attention_forward_drop", heads, heads);
  const NormEmitDropped drop{
      softmax_out, drop_mask("nts_edge_attention_forward_drop", p, seed)};
  /* pass 1 stashes into alpha_out, which the normalize pass turns into the
   * softmax while it writes the dropped weights to the two weight outputs */
  attention_forward(s, edge_items_known(s, column_offset, batch_size, edges),
                    heads, batch_size, alpha_out, softmax_out_perm, perm_pos,
                    EdgeScore{m_sum_out, s_src_mirror, s_dst, row_indices,
                              mirror_index, slope, 0.f},
                    &drop);
}

void nts_edge_softmax_forward_drop(nts_stream *s, float *msg_output,
                                   float *msg_output_perm,
                                   const nts_vid *perm_pos,
                                   const float *msg_input, float *msg_cached,
                                   const nts_vid *column_offset,
                                   nts_vid batch_size, nts_vid edges,
                                   nts_vid feature_size, float p,
                                   unsigned long long seed) {
  const NormEmitDropped drop{
      msg_output, drop_mask("nts_edge_softmax_forward_drop", p, seed)};
  s->softmax_stable_last = s->softmax_stable;
  if (!feature_size) return;
  const EdgeItems it = edge_items_known(s, column_offset, batch_size, edges);
  if (!it.ib) return;
  softmax_forward_passes(s, it, msg_cached, msg_input, batch_size,
                         feature_size, msg_output_perm, perm_pos, &drop);
}

void nts_edge_softmax_backward_drop(
    nts_stream *s, float *msg_input_grad, float *msg_input_grad_perm,
    const nts_vid *perm_pos, const float *msg_output_grad,
    const float *msg_cached, const float *lrelu_input, float slope,
    float *dst_sum, const nts_vid *column_offset, nts_vid batch_size,
    nts_vid edges, nts_vid feature_size, float p, unsigned long long seed) {
  const DropMask dm = drop_mask("nts_edge_softmax_backward_drop", p, seed);
  if (dst_sum && feature_size != 1) abort(); /* as for the fused entry */
  if (!feature_size) return;
  const EdgeItems it = edge_items_known(s, column_offset, batch_size, edges);
  if (!it.ib) return;
  softmax_backward_passes(s, it, msg_input_grad, msg_output_grad, msg_cached,
                          batch_size, feature_size, msg_input_grad_perm,
                          perm_pos, lrelu_input, slope, dst_sum, &dm);
}

static void weight_sum(nts_stream *s, const EdgeItems &p, nts_vid K,
                       float *out, const float *weights) {
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  launch_reduce(s, p, K, EdgeIn{weights}, SumToOut{out});
  dbg_sync(s, "k_weight_sum");
}

void nts_weight_sum(nts_stream *s, float *out, const float *weights,
                    const nts_vid *offset, nts_vid batch_size) {
  weight_sum(s, edge_items(s, offset, batch_size), 1, out, weights);
}

void nts_weight_sum_heads(nts_stream *s, float *out, const float *weights,
                          const nts_vid *offset, nts_vid batch_size,
                          nts_vid edges, nts_vid heads) {
  check_heads("nts_weight_sum_heads", heads, heads);
  weight_sum(s, edge_items_known(s, offset, batch_size, edges), heads, out,
             weights);
}

/* The row-pair passes' lane geometry.  R, columns per lane: the widest of
 * 4 / 2 / 1 that divides C and that every pointer permits, each by its own
 * element size: R * 4 bytes of alignment for an fp32 operand, R * 2 for a
 * bf16 one (R = 1 runs at any element alignment).  L = C / R lanes per head.
 * seg: L a power of two <= 64.  G, the lane group of one row: f / R lanes
 * rounded up to a power of two, <= 64. */
extern "C++" {
/* fp32_alignment / bf16_alignment: the OR of the pointers of each kind */
static uint32_t pair_cols(uint32_t C, uintptr_t fp32_alignment,
                          uintptr_t bf16_alignment) {
  for (uint32_t R = 4; R > 1; R /= 2)
    if (C % R == 0 && fp32_alignment % (R * sizeof(float)) == 0 &&
        bf16_alignment % (R * sizeof(uint16_t)) == 0)
      return R;
  return 1;
}
template <typename T>
static uintptr_t align_as(const T *p, size_t elem_bytes) {
  return sizeof(T) == elem_bytes ? (uintptr_t)p : 0;
}
/* fp32_extra: the term's own fp32 operand (att), 0 if none */
template <class Term, typename TD, typename TS>
static void launch_edge_pair(nts_stream *s, const EdgeItems &p, float *out,
                             const TD *dst_rows, const TS *src_rows,
                             const nts_vid *row_indices, nts_vid src_start,
                             nts_vid f, nts_vid K, uintptr_t fp32_extra,
                             const Term &term) {
  const uint32_t C = f / K;
  const uint32_t R = pair_cols(
      C, fp32_extra | align_as(dst_rows, 4) | align_as(src_rows, 4),
      align_as(dst_rows, 2) | align_as(src_rows, 2));
  const uint32_t L = C / R;
  if (!s->heads_general && (L & (L - 1)) == 0 && L <= 64) {
    uint32_t G = 64;
    while (G / 2 >= f / R) G /= 2;
    hipLaunchKernelGGL((R == 4   ? k_edge_pair_seg<4, Term, TD, TS>
                        : R == 2 ? k_edge_pair_seg<2, Term, TD, TS>
                                 : k_edge_pair_seg<1, Term, TD, TS>),
                       dim3(p.grid), dim3(NTS_BLOCK), 0, s->stream,
                       p.ib->items, p.ib->counter, out, dst_rows, src_rows,
                       row_indices, src_start, f, K, C, G, term);
  } else {
    hipLaunchKernelGGL((k_edge_pair<Term, TD, TS>), dim3(p.grid), dim3(NTS_BLOCK), 0,
                       s->stream, p.ib->items, p.ib->counter, out, dst_rows,
                       src_rows, row_indices, src_start, f, K, C, term);
  }
}
}  // extern "C++"

void nts_edge_dot_heads(nts_stream *s, float *out, const float *dst_rows,
                        const float *src_rows, const nts_vid *row_indices,
                        const nts_vid *column_offset, nts_vid src_start,
                        nts_vid batch_size, nts_vid edges,
                        nts_vid feature_size, nts_vid heads) {
  check_heads("nts_edge_dot_heads", feature_size, heads);
  const EdgeItems p = edge_items_known(s, column_offset, batch_size, edges);
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  if (heads == 1) /* k_edge_dot: another shape, measured */
    hipLaunchKernelGGL(k_edge_dot, dim3(p.grid), dim3(NTS_BLOCK), 0, s->stream,
                       p.ib->items, p.ib->counter, out, dst_rows, src_rows,
                       row_indices, src_start, feature_size);
  else
    launch_edge_pair(s, p, out, dst_rows, src_rows, row_indices, src_start,
                     feature_size, heads, 0, DotTerm{});
  dbg_sync(s, "k_edge_dot_heads");
}

void nts_edge_dot_heads_bf16(nts_stream *s, float *out, const float *dst_rows,
                             const uint16_t *src_rows,
                             const nts_vid *row_indices,
                             const nts_vid *column_offset, nts_vid src_start,
                             nts_vid batch_size, nts_vid edges,
                             nts_vid feature_size, nts_vid heads) {
  check_heads("nts_edge_dot_heads_bf16", feature_size, heads);
  const EdgeItems p = edge_items_known(s, column_offset, batch_size, edges);
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  /* heads == 1 too: the row-pair forms at K = 1 (k_edge_dot is fp32 only) */
  launch_edge_pair(s, p, out, dst_rows, src_rows, row_indices, src_start,
                   feature_size, heads, 0, DotTerm{});
  dbg_sync(s, "k_edge_dot_heads_bf16");
}

void nts_edge_gatv2_score(nts_stream *s, float *score, const float *dst_rows,
                          const float *src_rows, const float *att, float slope,
                          const nts_vid *row_indices,
                          const nts_vid *column_offset, nts_vid src_start,
                          nts_vid batch_size, nts_vid edges,
                          nts_vid feature_size, nts_vid heads) {
  check_heads("nts_edge_gatv2_score", feature_size, heads);
  const EdgeItems p = edge_items_known(s, column_offset, batch_size, edges);
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  launch_edge_pair(s, p, score, dst_rows, src_rows, row_indices, src_start,
                   feature_size, heads, (uintptr_t)att, Gatv2Term{att, slope});
  dbg_sync(s, "k_gatv2_score");
}

void nts_edge_gatv2_score_bf16(nts_stream *s, float *score,
                               const uint16_t *dst_rows,
                               const uint16_t *src_rows, const float *att,
                               float slope, const nts_vid *row_indices,
                               const nts_vid *column_offset, nts_vid src_start,
                               nts_vid batch_size, nts_vid edges,
                               nts_vid feature_size, nts_vid heads) {
  check_heads("nts_edge_gatv2_score_bf16", feature_size, heads);
  const EdgeItems p = edge_items_known(s, column_offset, batch_size, edges);
  if (!p.ib) return;
  Tic t(s, NTS_KTAG_EDGE);
  launch_edge_pair(s, p, score, dst_rows, src_rows, row_indices, src_start,
                   feature_size, heads, (uintptr_t)att, Gatv2Term{att, slope});
  dbg_sync(s, "k_gatv2_score_bf16");
}

extern "C++" {
template <typename T>
static void launch_gatv2_backward(nts_stream *s, const char *entry,
                                  float *grad_own, float *grad_att,
                                  const float *grad_score, const T *own_rows,
                                  const T *nbr_rows, const float *att,
                                  float slope, const nts_vid *offset,
                                  const nts_vid *nbr_indices,
                                  nts_vid nbr_start, nts_vid batch_size,
                                  nts_vid edges, nts_vid feature_size,
                                  nts_vid heads) {
  check_heads(entry, feature_size, heads);
  const EdgeItems p = edge_items_known(s, offset, batch_size, edges);
  if (!p.ib) return;
  const uint32_t f = feature_size, C = f / heads;
  /* columns per lane: 4 / 2 dividing C (a lane stays inside one head) where
   * every row pointer, att and grad_own permit the vector access (each by
   * its own element size, as pair_cols has it), else 1, which is also the
   * general form nts_heads_dbg_general asks for */
  uint32_t R = 1;
  if (!s->heads_general)
    R = pair_cols(C,
                  (uintptr_t)grad_own | (uintptr_t)att |
                      align_as(own_rows, 4) | align_as(nbr_rows, 4),
                  align_as(own_rows, 2) | align_as(nbr_rows, 2));
  uint32_t G = 64;
  while (G / 2 >= f / R && G > 16) G /= 2;
  const uint64_t bound_items = (uint64_t)batch_size + edges / NTS_SPLIT + 1;
  const uint32_t grid = grid_for(bound_items * G);
  Tic t(s, NTS_KTAG_EDGE);
#define NTS_K(RR)                                                             \
  (grad_att ? k_gatv2_backward<RR, true, T> : k_gatv2_backward<RR, false, T>)
  hipLaunchKernelGGL(R == 4 ? NTS_K(4) : R == 2 ? NTS_K(2) : NTS_K(1),
                     dim3(grid), dim3(NTS_BLOCK), 0, s->stream, p.ib->items,
                     p.ib->counter, grad_own, grad_att, grad_score, own_rows,
                     nbr_rows, att, slope, nbr_indices, nbr_start, f, heads, C,
                     G);
#undef NTS_K
  dbg_sync(s, "k_gatv2_backward");
}
}  // extern "C++"

void nts_edge_gatv2_backward(nts_stream *s, float *grad_own, float *grad_att,
                             const float *grad_score, const float *own_rows,
                             const float *nbr_rows, const float *att,
                             float slope, const nts_vid *offset,
                             const nts_vid *nbr_indices, nts_vid nbr_start,
                             nts_vid batch_size, nts_vid edges,
                             nts_vid feature_size, nts_vid heads) {
  launch_gatv2_backward(s, "nts_edge_gatv2_backward", grad_own, grad_att,
                        grad_score, own_rows, nbr_rows, att, slope, offset,
                        nbr_indices, nbr_start, batch_size, edges,
                        feature_size, heads);
}

void nts_edge_gatv2_backward_bf16(
    nts_stream *s, float *grad_own, float *grad_att, const float *grad_score,
    const uint16_t *own_rows, const uint16_t *nbr_rows, const float *att,
    float slope, const nts_vid *offset, const nts_vid *nbr_indices,
    nts_vid nbr_start, nts_vid batch_size, nts_vid edges, nts_vid feature_size,
    nts_vid heads) {
  launch_gatv2_backward(s, "nts_edge_gatv2_backward_bf16", grad_own, grad_att,
                        grad_score, own_rows, nbr_rows, att, slope, offset,
                        nbr_indices, nbr_start, batch_size, edges,
                        feature_size, heads);
}

int nts_gather_by_src_from_dst_dot(nts_stream *s, const float *input,
                                   float *output, const float *weight_backward,
                                   const nts_vid *row_offset,
                                   const nts_vid *column_indices,
                                   nts_vid dst_start, nts_vid batch_size,
                                   nts_vid edges, nts_vid feature_size,
                                   const float *dot_vec, float *dot_out,
                                   const nts_vid *dot_pos) {
  const uint32_t f = feature_size;
  if (!batch_size || !edges || !f) return 1;
  const GatherGeom geo = gather_geometry(
      f, (uintptr_t)input | (uintptr_t)output | (uintptr_t)dot_vec,
      sizeof(float));
  const int elem = geo.elem;
  const uint32_t G = geo.G;
  if (elem == 1 || f > G * (uint32_t)elem) {
    /* ragged or multi-slab width: unfused fallback — plain CSR gather; the
     * caller must compute the dot with nts_edge_dot */
    launch_gather(s, input, output, weight_backward, column_indices,
                  row_offset, dst_start, batch_size, edges, f, 1,
                  NTS_KTAG_BWD, /*rows unknown*/ 0);
    return 0;
  }
  ItemsBuf &ib = get_items(s, row_offset, batch_size, edges);
  const uint64_t bound_groups = (uint64_t)batch_size + edges / NTS_SPLIT + 1;
  const uint32_t grid = grid_for(bound_groups * G);
  Tic t(s, NTS_KTAG_BWD);
  hipLaunchKernelGGL(
      elem == 4 ? k_gather_spmm_dot_lds<4> : k_gather_spmm_dot_lds<2>,
      dim3(grid), dim3(NTS_BLOCK), 0, s->stream, ib.items, ib.counter,
      column_indices, weight_backward, input, output, dst_start, dot_vec,
      dot_out, dot_pos, f, G);
  dbg_sync(s, "k_gather_spmm_dot_lds");
  return 1;
}

static void launch_sampler(nts_stream *s,
                           decltype(&k_sample_reservoir<false>) kernel,
                           const nts_vid *column_offset,
                           const nts_vid *row_indices, const nts_vid *dst_list,
                           nts_vid n_dst, nts_vid fanout,
                           unsigned long long seed, nts_vid *out_src,
                           nts_vid *out_cnt) {
  if (!n_dst || !fanout) return;
  if (fanout > NTS_MAX_FANOUT) {
    fprintf(stderr, "nts_sample_reservoir: fanout %u > %u\n", fanout,
            NTS_MAX_FANOUT);
    abort();
  }
  Tic t(s, NTS_KTAG_ITEMS);
  hipLaunchKernelGGL(kernel, dim3(grid_for((uint64_t)n_dst * 64)),
                     dim3(NTS_BLOCK), 0, s->stream, column_offset, row_indices,
                     dst_list, n_dst, fanout, seed, out_src, out_cnt);
  dbg_sync(s, "k_sample_reservoir");
}

void nts_sample_reservoir(nts_stream *s, const nts_vid *column_offset,
                          const nts_vid *row_indices, const nts_vid *dst_list,
                          nts_vid n_dst, nts_vid fanout,
                          unsigned long long seed, nts_vid *out_src,
                          nts_vid *out_cnt) {
  launch_sampler(s, k_sample_reservoir<false>, column_offset, row_indices,
                 dst_list, n_dst, fanout, seed, out_src, out_cnt);
}

/* TEST-ONLY: same sampler with the 32-bit threshold search skipped, so the
 * deterministic 64-bit (key,slot) fallback — the path real inputs almost
 * never reach — is exercised on hardware.  Results must equal the normal
 * entry point's exactly (both select the fanout smallest (key,slot)). */
void nts_sample_reservoir_dbg_fallback(
    nts_stream *s, const nts_vid *column_offset, const nts_vid *row_indices,
    const nts_vid *dst_list, nts_vid n_dst, nts_vid fanout,
    unsigned long long seed, nts_vid *out_src, nts_vid *out_cnt) {
  launch_sampler(s, k_sample_reservoir<true>, column_offset, row_indices,
                 dst_list, n_dst, fanout, seed, out_src, out_cnt);
}

void nts_permute_f32(nts_stream *s, float *out, const float *in,
                     const nts_vid *index, long n) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_permute_f32, dim3(grid_for((uint64_t)n)),
                     dim3(NTS_BLOCK), 0, s->stream, out, in, index,
                     (uint64_t)n);
}

int nts_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

void nts_set_device(int dev) { NTS_CHECK(hipSetDevice(dev)); }

const char *nts_build_arch(void) { return "gfx950"; }

}  /* extern "C" */
