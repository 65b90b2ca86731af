"""Case driver of tests/test_gpu_grid_cap.py.  A helper module: no tests here.

    python -m tests.grid_cases --out FILE [--only NAME,...]

runs a table of named cases, one per entry point and kernel form, on the
current device and writes every output into one .npz, together with a JSON
block ("__meta__") that holds the NTS_* environment the process saw and, per
case, batch, edges, the work-item count computed on the host and the grid the
matching *_plan function reports in this process.

NTS_SPLIT, NTS_MAX_BLOCKS and NTS_GATHER_BLOCKS are read once into statics of
the library, so a configuration needs a process of its own; the test starts
one child per configuration and compares their files.  Inputs come from fixed
seeds: two children compute on the same inputs.

A case is (run, expect): run(env) launches on the device and returns the
outputs as numpy arrays; expect() needs no device and returns, per output, the
float64 reference, the bound of the existing GPU test of that entry (None:
exact), the number of edges behind every output row (for the bit-identity
checks) and the prefill.  The graphs, inputs and references are those of the
existing tests, imported from them.
"""
import argparse
import functools
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (_HERE, os.path.dirname(_HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import edge_ref as R  # noqa: E402
import heads_ref as H  # noqa: E402
import reduce_ref as RR  # noqa: E402
import sampler_ref as SR  # noqa: E402
import softmax_stable_ref as S  # noqa: E402
import dropout_ref as D  # noqa: E402
import test_gpu_edge_kernels as TE  # noqa: E402
import test_gpu_gat_backward_fused as TB  # noqa: E402
import test_gpu_gat_bf16 as T16  # noqa: E402
import test_gpu_gat_dropout as TD  # noqa: E402
import test_gpu_gat_infer as TI  # noqa: E402
import test_gpu_gather_dot as TGD  # noqa: E402
import test_gpu_gatv2_fused as TF  # noqa: E402
import test_gpu_gat_heads as TH  # noqa: E402
import test_gpu_gatv2 as TV  # noqa: E402
import test_gpu_parity as TP  # noqa: E402
import test_gpu_reduce as TR  # noqa: E402

SLOPE = TE.SLOPE
DEFAULT_SPLIT = R.SPLIT
DEFAULT_CAP = 8192
BLOCK = 256                # threads of a workgroup, 4 waves
SENT = 0x5A5A5A5A          # of tests/test_gpu_sampler_paths.py
ENV_NAMES = ("NTS_SPLIT", "NTS_MAX_BLOCKS", "NTS_GATHER_BLOCKS")

# the shape of the latch check: 2^20 rows of 64 floats are 2^16 workgroups
# uncapped, above every NTS_MAX_BLOCKS of the configurations
LATCH_SHAPE = dict(f=64, alignment=256, rows=1 << 20, batch=1 << 20,
                   edges=1 << 20, schedule=0, window=-1)


def env_seen():
    return {n: os.environ[n] for n in sorted(os.environ) if n.startswith("NTS_")}


def env_u32(name, default):
    """The library's rule for its three tunables (env_u32 in nts_hip.hip)."""
    try:
        v = int(os.environ.get(name, "") or 0)
    except ValueError:
        v = 0
    return v if v > 0 else default


# --------------------------------------------------------------------------
# topology: the edge-case graph walked by destination (csc); walked by source
# (csr) it has no vertex above 15 edges, so that direction runs on
# edge_ref.grid_case_graph, which has the same size and id range
# --------------------------------------------------------------------------
def graph():
    return R.edge_case_graph()


@functools.lru_cache(maxsize=None)
def csr_topology():
    """(row_offset, column_indices holding global destination ids) of
    grid_case_graph; destination d is global vertex src_start + d."""
    g = R.grid_case_graph()
    perm, _ = R.csc_to_csr(g.row_indices)
    roff = R.csr_offsets(g.row_indices, g.src_start, g.v_src)
    cidx = (g.src_start + g.dst_of_edge[perm]).astype(np.uint32)
    return roff, cidx


def topology(direction):
    """(offset, nbr, nbr_start, gathered rows, output rows), the tuple of
    test_gpu_gat_heads._topology."""
    if direction == "fwd":
        return TH._topology("fwd")
    g = R.grid_case_graph()
    roff, cidx = csr_topology()
    return roff, cidx, g.src_start, g.batch, g.v_src


@functools.lru_cache(maxsize=None)
def offsets(direction):
    if direction == "csc":
        return graph().column_offset
    return csr_topology()[0]


def degrees(direction):
    return np.diff(offsets(direction).astype(np.int64))


def item_count(direction, split):
    """Work items of a walk: every non-empty vertex is ceil(deg / split)."""
    deg = degrees(direction)
    return int((-(-deg // split)).sum())


def edge_degrees():
    """Per CSC edge: the in-degree of its destination."""
    g = graph()
    return g.deg[g.dst_of_edge]


class Expect(SimpleNamespace):
    """ref      float64 reference (or the exact array);
    bound    array / scalar, or None: exact;
    exact    "bits" (a copy) or "value" (IEEE ==, so -0 equals +0);
    deg      per leading row: how many terms are merged into it (None: the
             output takes no part in the bit-identity checks);
    atomic   the terms of a row arrive by atomics of several work items, so
             a row is order-free only with at most one term;
    prefill  what a row without terms must still hold, or None."""

    def __init__(self, ref, bound=None, exact="bits", deg=None, atomic=False,
                 prefill=None):
        super().__init__(ref=ref, bound=bound, exact=exact, deg=deg,
                         atomic=atomic, prefill=prefill)


class Case(SimpleNamespace):
    """entry    the shim entry point the case runs;
    run      run(env) -> {key: array};
    expect   expect() -> {key: Expect};
    work     work(split) -> number of work items (or elements, unit "thread")
             the launch strides over;
    unit     "wave", "thread", or "group" (lane groups of `plan`);
    plan     plan(shim) -> dict with grid (and lane_group), or None;
    blocked  the launch is capped by NTS_GATHER_BLOCKS, not NTS_MAX_BLOCKS."""


CASES = {}


def add(name, entry, run, expect, work, unit="wave", plan=None, blocked=False,
        size=None):
    """size: (batch, edges) where the case runs on a graph of its own."""
    assert name not in CASES, name
    CASES[name] = Case(name=name, entry=entry, run=run, expect=expect,
                       work=work, unit=unit, plan=plan, blocked=blocked,
                       size=size)


# --------------------------------------------------------------------------
# device helpers
# --------------------------------------------------------------------------
def make_env():
    import torch
    from neutronstarlite_amd import shim
    assert torch.cuda.is_available(), "the case driver needs a GPU"
    dev = torch.device("cuda:0")
    g = graph()
    roff, cidx = csr_topology()
    pos = R.csc_to_csr(g.row_indices)[1]
    up32 = lambda a: TH._up32(dev, a)
    env = SimpleNamespace(
        torch=torch, shim=shim, dev=dev, up32=up32,
        st=shim.Stream.wrap_torch_current(),
        general=shim.Stream.wrap_torch_current(),
        coff=up32(g.column_offset), rows=up32(g.row_indices),
        mi=up32(g.mirror_index), pos=up32(pos), roff=up32(roff),
        cidx=up32(cidx))
    env.general.heads_dbg_general(1)
    # the by-source walk of the edge-case graph itself (the GATv2 cases)
    env.roff_edge, env.cidx_edge = (up32(a) for a in TH._csr_topology()[:2])
    env.up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    env.buf = lambda shape, fill=None: TH.Buf(dev, shape, fill)
    env.streams = {}
    # the `gpu` dictionary the run helpers of the existing test modules take
    env.gpu = {"dev": dev, "shim": shim, "s": env.st, "general": env.general,
               "coff": env.coff, "rows": env.rows, "mi": env.mi,
               "roff": env.roff_edge, "cidx": env.cidx_edge}
    return env


def stream_of(env, general=False, stable=False):
    """A stream of its own per (general forms, stable softmax)."""
    key = (bool(general), bool(stable))
    if key not in env.streams:
        st = env.shim.Stream.wrap_torch_current()
        st.heads_dbg_general(int(key[0]))
        st.edge_softmax_stable(int(key[1]))
        env.streams[key] = st
    return env.streams[key]


def items_of(offset, split):
    deg = np.diff(np.asarray(offset).astype(np.int64))
    return int((-(-deg // split)).sum())


def _stream(env, form):
    return env.general if form == "general" else env.st


class _stable:
    """The stream's softmax mode for the calls inside the block."""

    def __init__(self, st, mode):
        self.st, self.on = st, mode == "stable"

    def __enter__(self):
        self.st.edge_softmax_stable(1 if self.on else 0)

    def __exit__(self, *exc):
        assert self.st.edge_softmax_stable_last() == (1 if self.on else 0)
        self.st.edge_softmax_stable(0)


MODES = ("default", "stable")


# --------------------------------------------------------------------------
# scalar gathers (bound of test_gather_heads, whose K = 1 is this entry)
# --------------------------------------------------------------------------
def _direction(direction):
    return "csc" if direction == "fwd" else "csr"


@functools.lru_cache(maxsize=None)
def _scalar_gather_case(f, direction, weighted):
    g = graph()
    off, nbr, start, n_in, n_out = topology(direction)
    rng = np.random.default_rng([11000, f, int(direction == "bwd"),
                                 int(weighted)])
    x = rng.uniform(-1, 1, (n_in, f)).astype(np.float32)
    w = rng.uniform(-1, 1, g.edges).astype(np.float32)
    pre = (rng.normal(size=(n_out, f)) + 3).astype(np.float32)
    ref, mag = H.gather(off, nbr, start, x,
                        w if weighted else np.ones_like(w), 1, pre)
    return x, w, pre, ref, mag


def _gather_args(env, direction, x_ptr, out_ptr, w_ptr, f):
    g = graph()
    _, _, start, n_in, n_out = topology(direction)
    if direction == "fwd":
        return (x_ptr, out_ptr, w_ptr, env.rows.data_ptr(),
                env.coff.data_ptr(), start, start + n_in, start,
                start + n_out, g.edges, n_out, f)
    return (x_ptr, out_ptr, w_ptr, env.roff.data_ptr(), env.cidx.data_ptr(),
            start, start + n_out, start, start + n_in, g.edges, n_out, f)


def _gather_expect(pre, ref, mag, direction):
    return {"out": Expect(ref, 1e-4 * np.abs(ref) + 1e-4 * mag,
                          deg=degrees(_direction(direction)), prefill=pre)}


# requests of the column-blocked and striped launches at f = 72, as
# (schedule, window, staging, stripe): three 32-float windows, the last of 8;
# NTS_SCHED_XCD needs 2, 4 or >= 8 windows, so it gets four of 20, the last
# of 12
PHASE, XCD = 1, 2
FORCED = {"phase": (PHASE, 32, 0, 0), "xcd": (XCD, 20, 0, 0),
          "stripe": (PHASE, 32, 1, 16)}


def _scalar_gather(f, direction, weighted, forced=None):
    sched, window, stage, stripe = FORCED[forced] if forced else (0, 0, 0, 0)

    def run(env):
        x, w, pre, _, _ = _scalar_gather_case(f, direction, weighted)
        st = env.st
        d_x, d_w = env.up(x), env.up(w)
        out = env.buf(pre.shape, pre)
        entry = (st.gather_by_dst_from_src if direction == "fwd"
                 else st.gather_by_src_from_dst)
        st.gather_schedule(sched, window)
        st.gather_staging(stage)
        st.gather_stripes(stripe)
        try:
            entry(*_gather_args(env, direction, d_x.data_ptr(), out.ptr,
                                d_w.data_ptr(), f), weighted)
            ran = (st.gather_schedule_last() + st.gather_staging_last()
                   + st.gather_stripes_last())
        finally:
            st.gather_schedule(0, 0)
            st.gather_staging(0)
            st.gather_stripes(0)
        return {"out": out.read("gather"),
                "ran": np.array([int(v) for v in ran], dtype=np.int64)}

    def expect():
        _, _, pre, ref, mag = _scalar_gather_case(f, direction, weighted)
        return _gather_expect(pre, ref, mag, direction)

    def plan(shim):
        _, _, _, n_in, n_out = topology(direction)
        return shim.gather_stripe_plan(f, 256, 256, n_in, n_out, graph().edges,
                                       sched, window, stage, stripe)

    name = (f"gather_{direction}_f{f}_{'w' if weighted else 'now'}"
            + (f"_{forced}" if forced else ""))
    add(name, "gather_by_dst_from_src" if direction == "fwd"
        else "gather_by_src_from_dst", run, expect,
        lambda split: item_count(_direction(direction), split), "group", plan,
        blocked=forced is not None)
    return name


SCALAR_GATHERS = [_scalar_gather(f, d, w) for f in (33, 64)
                  for d in ("fwd", "bwd") for w in (True, False)]
FORCED_GATHERS = [_scalar_gather(72, "fwd", True, k) for k in FORCED]


# --------------------------------------------------------------------------
# heads gathers
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _heads_gather_case(heads, c_per, direction):
    """test_gpu_gat_heads._gather_case; by source, the same draw on
    grid_case_graph."""
    if direction == "fwd":
        return TH._gather_case(heads, c_per, direction)
    off, nbr, start, n_in, n_out = topology(direction)
    f = heads * c_per
    rng = np.random.default_rng([7000, heads, c_per, 1, 0])
    x = rng.uniform(-1, 1, (n_in, f)).astype(np.float32)
    w = rng.uniform(-1, 1, (graph().edges, heads)).astype(np.float32)
    pre = (rng.normal(size=(n_out, f)) + 3).astype(np.float32)
    return (x, w, pre) + H.gather(off, nbr, start, x, w, heads, pre)


def _heads_gather(heads, c_per, direction):
    f = heads * c_per

    def run(env):
        x, w, pre, _, _ = _heads_gather_case(heads, c_per, direction)
        d_x, d_w = env.up(x), env.up(w)
        out = env.buf(pre.shape, pre)
        entry = (env.st.gather_by_dst_from_src_heads if direction == "fwd"
                 else env.st.gather_by_src_from_dst_heads)
        entry(*_gather_args(env, direction, d_x.data_ptr(), out.ptr,
                            d_w.data_ptr(), f), heads)
        return {"out": out.read("heads gather")}

    def expect():
        _, _, pre, ref, mag = _heads_gather_case(heads, c_per, direction)
        return _gather_expect(pre, ref, mag, direction)

    def plan(shim):
        off = offsets(_direction(direction))
        return shim.gather_plan_heads(f, heads, 256, len(off) - 1,
                                      graph().edges)

    add(f"gather_heads_{direction}_K{heads}_C{c_per}",
        "gather_by_dst_from_src_heads" if direction == "fwd"
        else "gather_by_src_from_dst_heads", run, expect,
        lambda split: item_count(_direction(direction), split), "group", plan)


for _k, _c in ((8, 8), (3, 7)):
    for _d in ("fwd", "bwd"):
        _heads_gather(_k, _c, _d)


# --------------------------------------------------------------------------
# the five k_edge_items ops (inputs, references and bounds of test_edge_op)
# --------------------------------------------------------------------------
EDGE_OPS = R.OVERWRITE[:2] + R.ACCUMULATE
EDGE_ENTRY = {"scatter_src_to_msg": "scatter_src_mirror_to_msg",
              "scatter_dst_to_msg": "scatter_dst_to_msg",
              "gather_msg_to_src": "gather_msg_to_src_mirror",
              "gather_msg_to_dst": "gather_msg_to_dst",
              "scatter_grad_back_to_msg": "scatter_grad_back_to_message"}


def _mirror_terms():
    """Per mirror row (the extra ones included): how many edges add to it."""
    g = graph()
    rows = g.mirror_index[g.row_indices].astype(np.int64)
    return np.bincount(rows, minlength=g.m + TE.EXTRA_ROWS)


def _edge_op(op, f):
    def run(env):
        g, x = graph(), TE._edge_inputs(f)
        st = env.st
        topo = (env.rows.data_ptr(), env.coff.data_ptr())
        if op == "scatter_src_to_msg":
            src = env.up(x["mirror"])
            out = env.buf((g.edges, f))
            st.scatter_src_mirror_to_msg(out.ptr, src.data_ptr(), *topo,
                                         env.mi.data_ptr(), g.batch, f)
        elif op == "scatter_dst_to_msg":
            src = env.up(x["dstf"])
            out = env.buf((g.edges, f))
            st.scatter_dst_to_msg(out.ptr, src.data_ptr(), *topo, g.batch, f)
        elif op == "gather_msg_to_src":
            src = env.up(x["msg"])
            out = env.buf((g.m + TE.EXTRA_ROWS, f), x["pre_src"])
            st.gather_msg_to_src_mirror(out.ptr, src.data_ptr(), *topo,
                                        env.mi.data_ptr(), g.batch, f)
        elif op == "gather_msg_to_dst":
            src = env.up(x["msg"])
            out = env.buf((g.batch, f), x["pre_dst"])
            st.gather_msg_to_dst(out.ptr, src.data_ptr(), *topo, g.batch, f)
        else:
            src = env.up(x["dstf"])
            out = env.buf((g.edges, f), x["pre_msg"])
            st.scatter_grad_back_to_message(src.data_ptr(), out.ptr, *topo,
                                            g.batch, f)
        return {"out": out.read(op)}

    def expect():
        g, x = graph(), TE._edge_inputs(f)
        ref, mag = TE._edge_ref(op, f)
        if op in R.OVERWRITE:
            return {"out": Expect(ref.astype(np.float32), deg=edge_degrees())}
        bound = 1e-4 * np.abs(ref) + 1e-4 * mag
        if op == "gather_msg_to_src":
            return {"out": Expect(ref, bound, deg=_mirror_terms(),
                                  atomic=True, prefill=x["pre_src"])}
        if op == "gather_msg_to_dst":
            return {"out": Expect(ref, bound, deg=g.deg,
                                  prefill=x["pre_dst"])}
        return {"out": Expect(ref, bound, deg=edge_degrees())}

    add(f"{op}_f{f}", EDGE_ENTRY[op], run, expect,
        lambda split: item_count("csc", split))


for _op in EDGE_OPS:
    for _f in (1, 5):
        _edge_op(_op, _f)


# --------------------------------------------------------------------------
# edge softmax (inputs of test_softmax_forward / test_softmax_backward, the
# "normal" regime; the bound is the relative 1e-4 of _assert_rel there and of
# _assert_softmax in test_gpu_softmax_stable.py, every reference value being
# far above its 1e-30 floor)
# --------------------------------------------------------------------------
SOFTMAX_F = 3


def _softmax_ref(mode):
    x, ref = TE._softmax_case("normal", SOFTMAX_F)
    if mode == "stable":
        ref = S.softmax_forward(graph().column_offset, x)
    return x, ref


def _softmax_forward(mode, dual):
    f = SOFTMAX_F

    def run(env):
        g = graph()
        x, _ = _softmax_ref(mode)
        d_x = env.up(x)
        out, cached = env.buf((g.edges, f)), env.buf((g.edges, f))
        with _stable(env.st, mode):
            if dual:
                out2 = env.buf((g.edges, f))
                env.st.edge_softmax_forward_dual(
                    out.ptr, out2.ptr, env.pos.data_ptr(), d_x.data_ptr(),
                    cached.ptr, env.coff.data_ptr(), g.batch, f)
            else:
                env.st.edge_softmax_forward(
                    out.ptr, d_x.data_ptr(), cached.ptr, env.rows.data_ptr(),
                    env.coff.data_ptr(), g.batch, f)
        res = {"out": out.read("softmax"), "cached": cached.read("cached")}
        if dual:
            res["perm"] = out2.read("perm")
        return res

    def expect():
        _, ref = _softmax_ref(mode)
        e = {k: Expect(ref, 1e-4 * np.abs(ref), deg=edge_degrees())
             for k in ("out", "cached")}
        if dual:
            perm = R.csc_to_csr(graph().row_indices)[0]
            e["perm"] = Expect(ref[perm], 1e-4 * np.abs(ref[perm]),
                               deg=edge_degrees()[perm])
        return e

    add(f"softmax_forward{'_dual' if dual else ''}_{mode}",
        "edge_softmax_forward_dual" if dual else "edge_softmax_forward",
        run, expect, lambda split: item_count("csc", split))


for _mode in MODES:
    _softmax_forward(_mode, False)
    _softmax_forward(_mode, True)


def _softmax_backward(fused, mode):
    """Under both softmax modes of the stream, which the backward entries
    must not be moved by; fused runs at f = 1 with the mask, the CSR-order
    copy and dst_sum."""
    f = 1 if fused else SOFTMAX_F

    def run(env):
        env.st.edge_softmax_stable(int(mode == "stable"))
        try:
            return launch(env)
        finally:
            env.st.edge_softmax_stable(0)

    def launch(env):
        g = graph()
        grad, cached, lin, pre, _, _ = TE._backward_case(f)
        d_g, d_c, d_l = env.up(grad), env.up(cached), env.up(lin)
        out = env.buf((g.edges, f))
        if not fused:
            env.st.edge_softmax_backward(
                out.ptr, d_g.data_ptr(), d_c.data_ptr(), env.rows.data_ptr(),
                env.coff.data_ptr(), g.batch, f)
            return {"out": out.read("softmax bwd")}
        out2, dsum = env.buf((g.edges, f)), env.buf((g.batch,), pre)
        env.st.edge_softmax_backward_fused(
            out.ptr, out2.ptr, env.pos.data_ptr(), d_g.data_ptr(),
            d_c.data_ptr(), d_l.data_ptr(), SLOPE, env.coff.data_ptr(),
            g.batch, f, dst_sum=dsum.ptr)
        return {"out": out.read("bwd fused"), "perm": out2.read("perm"),
                "dst_sum": dsum.read("dst_sum")}

    def expect():
        g = graph()
        _, _, _, pre, plain, masked = TE._backward_case(f)
        if not fused:
            return {"out": Expect(plain[0], 1e-4 * plain[1],
                                  deg=edge_degrees())}
        perm = R.csc_to_csr(g.row_indices)[0]
        return {"out": Expect(masked[0], 1e-4 * masked[1],
                              deg=edge_degrees()),
                "perm": Expect(masked[0][perm], 1e-4 * masked[1][perm],
                               deg=edge_degrees()[perm]),
                "dst_sum": Expect(masked[2], 1e-4 * masked[3], deg=g.deg,
                                  prefill=pre)}

    add(f"softmax_backward{'_fused' if fused else ''}_{mode}",
        "edge_softmax_backward_fused" if fused else "edge_softmax_backward",
        run, expect, lambda split: item_count("csc", split))


for _mode in MODES:
    _softmax_backward(False, _mode)
    _softmax_backward(True, _mode)


# --------------------------------------------------------------------------
# attention forward: the single entry and the heads entry, fast and general
# --------------------------------------------------------------------------
ATT_HEADS = 3


def _attention(entry, form, mode):
    heads = 1 if entry == "single" else ATT_HEADS

    def run(env):
        g = graph()
        s_src, s_dst, _, _ = TH._attention_case(heads, True)
        st = _stream(env, form)
        d_src, d_dst = env.up(s_src), env.up(s_dst)
        shape = (g.edges, heads)
        out, out2, msum = (env.buf(shape) for _ in range(3))
        args = (out.ptr, out2.ptr, env.pos.data_ptr(), msum.ptr,
                d_src.data_ptr(), d_dst.data_ptr(), env.rows.data_ptr(),
                env.mi.data_ptr(), SLOPE, env.coff.data_ptr(), g.batch)
        with _stable(st, mode):
            if entry == "single":
                st.edge_attention_forward(*args)
            else:
                st.edge_attention_forward_heads(*args, g.edges, heads)
        return {"out": out.read("attention"), "perm": out2.read("perm"),
                "m_sum": msum.read("m_sum")}

    def expect():
        _, _, m_ref, s_ref = TH._attention_case(heads, True)
        perm = R.csc_to_csr(graph().row_indices)[0]
        ed = edge_degrees()
        return {"out": Expect(s_ref, 1e-4 * np.abs(s_ref), deg=ed),
                "perm": Expect(s_ref[perm], 1e-4 * np.abs(s_ref[perm]),
                               deg=ed[perm]),
                "m_sum": Expect(m_ref, deg=ed)}

    add(f"attention_{entry}_{form}_{mode}",
        "edge_attention_forward" if entry == "single"
        else "edge_attention_forward_heads", run, expect,
        lambda split: item_count("csc", split))


for _mode in MODES:
    _attention("single", "auto", _mode)
    _attention("heads", "auto", _mode)
    _attention("heads", "general", _mode)


# --------------------------------------------------------------------------
# edge dot, weight sum, permute
# --------------------------------------------------------------------------
def _edge_dot(f):
    def run(env):
        g = graph()
        a, b, _, _ = TE._dot_case(f)
        d_a, d_b = env.up(a), env.up(b)
        out = env.buf((g.edges,))
        env.st.edge_dot(out.ptr, d_a.data_ptr(), d_b.data_ptr(),
                        env.rows.data_ptr(), env.coff.data_ptr(), g.src_start,
                        g.batch, f)
        return {"out": out.read("edge_dot")}

    def expect():
        _, _, ref, mag = TE._dot_case(f)
        return {"out": Expect(ref, 1e-5 + 1e-4 * mag, deg=edge_degrees())}

    add(f"edge_dot_f{f}", "edge_dot", run, expect,
        lambda split: item_count("csc", split))


_edge_dot(33)


def _edge_dot_heads(heads, c_per, form):
    def run(env):
        g = graph()
        a, b, _, _ = TH._dot_case(heads, c_per)
        d_a, d_b = env.up(a), env.up(b)
        out = env.buf((g.edges, heads))
        _stream(env, form).edge_dot_heads(
            out.ptr, d_a.data_ptr(), d_b.data_ptr(), env.rows.data_ptr(),
            env.coff.data_ptr(), g.src_start, g.batch, g.edges,
            heads * c_per, heads)
        return {"out": out.read("edge_dot_heads")}

    def expect():
        _, _, ref, mag = TH._dot_case(heads, c_per)
        return {"out": Expect(ref, 1e-5 + 1e-4 * mag, deg=edge_degrees())}

    add(f"edge_dot_heads_K{heads}_C{c_per}_{form}", "edge_dot_heads", run,
        expect, lambda split: item_count("csc", split))


_edge_dot_heads(8, 16, "auto")
_edge_dot_heads(8, 16, "general")
_edge_dot_heads(3, 7, "auto")


@functools.lru_cache(maxsize=None)
def _weight_sum_case(heads, order):
    """Signed weights onto a non-zero prefill, as test_weight_sum[_heads]."""
    g = graph()
    off = offsets(order)
    n = len(off) - 1
    rng = np.random.default_rng([12000, heads, int(order == "csr")])
    w = rng.normal(size=(g.edges, heads)).astype(np.float32)
    pre = (rng.normal(size=(n, heads)) + 2).astype(np.float32)
    ref, mag = H.weight_sum(off, w, pre)
    return w, pre, ref, mag


def _weight_sum(heads, form, order):
    """heads = 0: the scalar entry (bound of test_weight_sum, 1e-4 * mag);
    else the heads entry (bound of test_weight_sum_heads)."""
    k = max(heads, 1)

    def run(env):
        g = graph()
        w, pre, _, _ = _weight_sum_case(k, order)
        d_w = env.up(w)
        d_off = env.coff if order == "csc" else env.roff
        out = env.buf(pre.shape, pre)
        if heads:
            _stream(env, form).weight_sum_heads(
                out.ptr, d_w.data_ptr(), d_off.data_ptr(), pre.shape[0],
                g.edges, heads)
        else:
            env.st.weight_sum(out.ptr, d_w.data_ptr(), d_off.data_ptr(),
                              pre.shape[0])
        return {"out": out.read("weight_sum")}

    def expect():
        _, pre, ref, mag = _weight_sum_case(k, order)
        bound = 1e-4 * np.abs(ref) + 1e-4 * mag if heads else 1e-4 * mag
        return {"out": Expect(ref, bound, deg=degrees(order), prefill=pre)}

    name = (f"weight_sum_heads_K{heads}_{form}_{order}" if heads
            else f"weight_sum_{order}")
    add(name, "weight_sum_heads" if heads else "weight_sum", run, expect,
        lambda split: item_count(order, split))


for _order in ("csc", "csr"):
    _weight_sum(0, "auto", _order)
    _weight_sum(3, "auto", _order)
    _weight_sum(3, "general", _order)


PERMUTE_N = 70001


@functools.lru_cache(maxsize=None)
def _permute_case():
    """Random bit patterns, NaN payloads among them, under an index with
    repeats (test_permute)."""
    rng = np.random.default_rng(13000)
    n_in = PERMUTE_N // 2 + 1
    bits = rng.integers(-2**31, 2**31, n_in, dtype=np.int64).astype(np.int32)
    bits[::5] = np.int32(0x7fc00000) | rng.integers(
        1, 1 << 22, len(bits[::5])).astype(np.int32)
    index = rng.integers(0, n_in, PERMUTE_N).astype(np.uint32)
    return bits, index


def _permute():
    def run(env):
        bits, index = _permute_case()
        d_in, d_idx = env.up(bits), env.up32(index)
        out = env.buf((PERMUTE_N,))
        env.st.permute_f32(out.ptr, d_in.data_ptr(), d_idx.data_ptr(),
                           PERMUTE_N)
        return {"out": out.read("permute")}

    def expect():
        bits, index = _permute_case()
        return {"out": Expect(bits[index].view(np.float32),
                              deg=np.ones(PERMUTE_N, dtype=np.int64))}

    add("permute_f32", "permute_f32", run, expect, lambda split: PERMUTE_N,
        "thread")


_permute()


# --------------------------------------------------------------------------
# GATv2: score, and the backward with grad_att (inputs, references and
# bounds of test_score / test_backward in test_gpu_gatv2.py; both walks are
# those of the edge-case graph, as there)
# --------------------------------------------------------------------------
V2_SHAPE = (8, 16)      # the fast form holds datt[4] per lane at C = 16


def _gatv2_score(form):
    heads, c_per = V2_SHAPE

    def run(env):
        g = graph()
        x_l, x_r, att = TV._inputs(heads, c_per)
        d_r, d_l, d_a = env.up(x_r), env.up(x_l), env.up(att)
        out = env.buf((g.edges, heads))
        _stream(env, form).edge_gatv2_score(
            out.ptr, d_r.data_ptr(), d_l.data_ptr(), d_a.data_ptr(), SLOPE,
            env.rows.data_ptr(), env.coff.data_ptr(), g.src_start, g.batch,
            g.edges, heads * c_per, heads)
        return {"out": out.read("gatv2 score")}

    def expect():
        ref, mag = TV._score_ref(heads, c_per)
        return {"out": Expect(ref, 1e-5 + 1e-4 * mag, deg=edge_degrees())}

    add(f"gatv2_score_{form}", "edge_gatv2_score", run, expect,
        lambda split: item_count("csc", split))


def _edge_csr_items(split):
    deg = np.diff(TH._csr_topology()[0].astype(np.int64))
    return int((-(-deg // split)).sum())


def _gatv2_backward(form, d):
    """grad_att is asked for in both walks: its order of addition is not
    fixed (the header), so it is held to the bound only."""
    heads, c_per = V2_SHAPE

    def case():
        x_l, x_r, att = TV._inputs(heads, c_per)
        own, nbr_rows = TV._own_nbr(d, x_l, x_r)
        off, nbr, start, _, _ = TV._direction(d)
        rng = np.random.default_rng([16000, int(d == "csr")])
        g = graph()
        gs = rng.normal(size=(g.edges, heads)).astype(np.float32)
        pre = (rng.normal(size=own.shape) + 3).astype(np.float32)
        pre_att = (rng.normal(size=heads * c_per) + 3).astype(np.float32)
        res = TV.V.backward(off, nbr, start, gs, own, nbr_rows, att, SLOPE,
                            heads, pre, pre_att)
        return (own, nbr_rows, att, gs, pre, pre_att, off) + tuple(res)

    case = functools.lru_cache(maxsize=None)(case)

    def run(env):
        g = graph()
        own, nbr_rows, att, gs, pre, pre_att = case()[:6]
        d_own, d_nbr, d_att, d_gs = (env.up(a) for a in
                                     (own, nbr_rows, att, gs))
        out = env.buf(own.shape, pre)
        out_att = env.buf((att.size,), pre_att)
        off, nbr = ((env.coff, env.rows) if d == "csc"
                    else (env.roff_edge, env.cidx_edge))
        _stream(env, form).edge_gatv2_backward(
            out.ptr, out_att.ptr, d_gs.data_ptr(), d_own.data_ptr(),
            d_nbr.data_ptr(), d_att.data_ptr(), SLOPE, off.data_ptr(),
            nbr.data_ptr(), g.src_start, own.shape[0], g.edges, own.shape[1],
            heads)
        return {"grad_own": out.read("gatv2 backward"),
                "grad_att": out_att.read("grad_att")}

    def expect():
        g = graph()
        _, _, _, _, pre, _, off, ref, mag, ref_att, mag_att = case()
        return {"grad_own": Expect(ref, 1e-4 * np.abs(ref) + 1e-4 * mag,
                                   deg=np.diff(off.astype(np.int64)),
                                   prefill=pre),
                "grad_att": Expect(ref_att,
                                   (g.edges + 2) * 2.0 ** -24 * mag_att)}

    add(f"gatv2_backward_{form}_{d}", "edge_gatv2_backward", run, expect,
        (lambda split: item_count("csc", split)) if d == "csc"
        else _edge_csr_items)


for _form in ("auto", "general"):
    _gatv2_score(_form)
    for _d in ("csc", "csr"):
        _gatv2_backward(_form, _d)


# --------------------------------------------------------------------------
# bf16 rows: the scalar and heads gathers, the per-head dot, GATv2 score and
# backward.  Rows and run helpers of test_gpu_gat_bf16.py; the references are
# evaluated on the widened rows and the bounds are the fp32 entries'.
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _gather16_case(heads, c_per, direction, weighted):
    """heads = 0: the scalar entry, one weight per edge."""
    k = max(heads, 1)
    off, nbr, start, n_in, n_out = topology(direction)
    f = k * c_per
    rng = np.random.default_rng([17000, heads, c_per,
                                 int(direction == "bwd"), int(weighted)])
    bits, x = T16.make_rows((n_in, f), rng)
    w = rng.uniform(-1, 1, (graph().edges, k)).astype(np.float32)
    pre = (rng.normal(size=(n_out, f)) + 3).astype(np.float32)
    ref, mag = H.gather(off, nbr, start, x,
                        w if weighted else np.ones_like(w), k, pre)
    return bits, w, pre, ref, mag


def _gather16(heads, c_per, direction, weighted=True):
    f = max(heads, 1) * c_per

    def run(env):
        bits, w, pre, _, _ = _gather16_case(heads, c_per, direction, weighted)
        d_x, d_w = T16.Inp16(env.dev, bits), env.up(w)
        out = env.buf(pre.shape, pre)
        name = ("gather_by_dst_from_src" if direction == "fwd"
                else "gather_by_src_from_dst") + ("_heads" if heads else "")
        getattr(env.st, name + "_bf16")(
            *_gather_args(env, direction, d_x.ptr, out.ptr, d_w.data_ptr(),
                          f), heads if heads else weighted)
        return {"out": out.read("bf16 gather")}

    def expect():
        _, _, pre, ref, mag = _gather16_case(heads, c_per, direction,
                                             weighted)
        return _gather_expect(pre, ref, mag, direction)

    def plan(shim):
        off, _, _, n_in, n_out = topology(direction)
        if heads:
            return shim.gather_plan_heads_bf16(f, heads, 256, n_out,
                                               graph().edges)
        return shim.gather_plan_bf16(f, 256, n_in, n_out, graph().edges)

    entry = ("gather_by_dst_from_src" if direction == "fwd"
             else "gather_by_src_from_dst")
    if heads:
        add(f"gather_heads_bf16_{direction}_K{heads}_C{c_per}",
            entry + "_heads_bf16", run, expect,
            lambda split: item_count(_direction(direction), split), "group",
            plan)
    else:
        add(f"gather_bf16_{direction}_f{f}_{'w' if weighted else 'now'}",
            entry + "_bf16", run, expect,
            lambda split: item_count(_direction(direction), split), "group",
            plan)


for _d in ("fwd", "bwd"):
    for _f in (33, 64):
        for _w in (True, False):
            _gather16(0, _f, _d, _w)
    for _k, _c in ((8, 8), (3, 7)):
        _gather16(_k, _c, _d)


def _edge_dot_heads_bf16(heads, c_per, form):
    def run(env):
        a, bits, _, _, _ = T16._dot_case(heads, c_per)
        out = T16._run_dot(env.gpu, form, heads, c_per, TH.Inp(env.dev, a),
                           T16.Inp16(env.dev, bits), True)
        return {"out": out.read("edge_dot_heads_bf16")}

    def expect():
        _, _, _, ref, mag = T16._dot_case(heads, c_per)
        return {"out": Expect(ref, 1e-5 + 1e-4 * mag, deg=edge_degrees())}

    add(f"edge_dot_heads_bf16_K{heads}_C{c_per}_{form}",
        "edge_dot_heads_bf16", run, expect,
        lambda split: item_count("csc", split))


_edge_dot_heads_bf16(8, 16, "auto")
_edge_dot_heads_bf16(3, 7, "auto")


def _gatv2_score_bf16(form):
    heads, c_per = V2_SHAPE

    def run(env):
        (l_bits, _), (r_bits, _), att = T16._v2_inputs(heads, c_per)
        out = T16._run_score(env.gpu, form, heads, c_per,
                             T16.Inp16(env.dev, r_bits),
                             T16.Inp16(env.dev, l_bits),
                             TH.Inp(env.dev, att), True)
        return {"out": out.read("gatv2 score bf16")}

    def expect():
        ref, mag = T16._score_ref(heads, c_per)
        return {"out": Expect(ref, 1e-5 + 1e-4 * mag, deg=edge_degrees())}

    add(f"gatv2_score_bf16_{form}", "edge_gatv2_score_bf16", run, expect,
        lambda split: item_count("csc", split))


def _gatv2_backward_bf16(form, d):
    """As _gatv2_backward: grad_att asked for in both walks."""
    heads, c_per = V2_SHAPE

    @functools.lru_cache(maxsize=None)
    def case():
        (l_bits, x_l), (r_bits, x_r), att = T16._v2_inputs(heads, c_per)
        own, nbr_rows = TV._own_nbr(d, x_l, x_r)
        own_bits, nbr_bits = TV._own_nbr(d, l_bits, r_bits)
        off, nbr, start, _, _ = TV._direction(d)
        rng = np.random.default_rng([18000, int(d == "csr")])
        gs = rng.normal(size=(graph().edges, heads)).astype(np.float32)
        pre = (rng.normal(size=own.shape) + 3).astype(np.float32)
        pre_att = (rng.normal(size=heads * c_per) + 3).astype(np.float32)
        res = TV.V.backward(off, nbr, start, gs, own, nbr_rows, att, SLOPE,
                            heads, pre, pre_att)
        return (own_bits, nbr_bits, att, gs, pre, pre_att, off) + tuple(res)

    def run(env):
        own_bits, nbr_bits, att, gs, pre, pre_att = case()[:6]
        got, got_att = T16._run_backward(
            env.gpu, d, form, heads, T16.Inp16(env.dev, own_bits),
            T16.Inp16(env.dev, nbr_bits), pre.shape, att, gs, pre, pre_att,
            SLOPE, True, True, "gatv2 backward bf16")
        return {"grad_own": got, "grad_att": got_att}

    def expect():
        g = graph()
        _, _, _, _, pre, _, off, ref, mag, ref_att, mag_att = case()
        return {"grad_own": Expect(ref, 1e-4 * np.abs(ref) + 1e-4 * mag,
                                   deg=np.diff(off.astype(np.int64)),
                                   prefill=pre),
                "grad_att": Expect(ref_att,
                                   (g.edges + 2) * 2.0 ** -24 * mag_att)}

    add(f"gatv2_backward_bf16_{form}_{d}", "edge_gatv2_backward_bf16", run,
        expect, (lambda split: item_count("csc", split)) if d == "csc"
        else _edge_csr_items)


for _form in ("auto", "general"):
    _gatv2_score_bf16(_form)
    for _d in ("csc", "csr"):
        _gatv2_backward_bf16(_form, _d)


# --------------------------------------------------------------------------
# the fused GAT forward (cases, bound and run helper of test_gpu_gat_infer.py)
# --------------------------------------------------------------------------
FUSED_SHAPE = (8, 16)


def _gat_forward_fused(bf16, mode):
    heads, c_per = FUSED_SHAPE

    def case():
        if bf16:
            return TI._bf16_case(heads, c_per)
        return (None,) + TI._case(heads, c_per)

    def run(env):
        bits, x, pre, _, _ = case()
        _, mirror, s_dst, _ = TI._scalars(heads)
        st = stream_of(env, False, mode == "stable")
        got = TI._run_fused(env.gpu, st, x, pre, mirror, s_dst, True, heads,
                            bits=bits)
        assert st.edge_softmax_stable_last() == int(mode == "stable")
        return {"out": got}

    def expect():
        _, _, pre, ref, mag = case()
        return {"out": Expect(ref, TI._bound(ref, mag), deg=graph().deg,
                              prefill=pre)}

    def plan(shim):
        g = graph()
        fn = shim.gather_plan_heads_bf16 if bf16 else shim.gather_plan_heads
        return fn(heads * c_per, heads, 256, g.batch, g.edges)

    add(f"gat_forward_fused{'_bf16' if bf16 else ''}_{mode}",
        "gat_forward_fused" + ("_bf16" if bf16 else ""), run, expect,
        lambda split: item_count("csc", split), "group", plan)


# --------------------------------------------------------------------------
# the fused GATv2 forward, which carries (m, S, acc) from item to item (cases,
# bound and run helper of test_gpu_gatv2_fused.py)
# --------------------------------------------------------------------------
def _gatv2_forward_fused(bf16, form, mode):
    heads, c_per = FUSED_SHAPE
    stable = int(mode == "stable")

    def run(env):
        x_l, x_r, att, pre, _, _, _ = TF._case(heads, c_per, 1.0, bf16)
        if bf16:
            d_l, d_r = (T16.Inp16(env.dev, T16.round_bf16(a))
                        for a in (x_l, x_r))
        else:
            d_l, d_r = TH.Inp(env.dev, x_l), TH.Inp(env.dev, x_r)
        st = stream_of(env, form == "general", stable)
        out, ran = TF._run(env.gpu, st, heads, c_per, d_l, d_r, att, pre,
                           bf16=bf16)
        assert ran == 1 and st.edge_softmax_stable_last() == stable
        return {"out": out.read("gatv2 fused")}

    def expect():
        _, _, _, pre, ref, bound, _ = TF._case(heads, c_per, 1.0, bf16)
        return {"out": Expect(ref, bound, deg=graph().deg, prefill=pre)}

    def plan(shim):
        g = graph()
        return shim.gatv2_forward_fused_plan(
            heads * c_per, heads, 2 if bf16 else 4, 256, 256, g.batch,
            g.edges, form == "general")

    add(f"gatv2_forward_fused{'_bf16' if bf16 else ''}_{form}_{mode}",
        "gatv2_forward_fused" + ("_bf16" if bf16 else ""), run, expect,
        lambda split: item_count("csc", split), "group", plan)


# --------------------------------------------------------------------------
# the fused GAT backward, which re-seeds own, the record and acc_s per item
# (graph, cases, tolerance and run helper of test_gpu_gat_backward_fused.py)
# --------------------------------------------------------------------------
def _gat_backward_fused(bf16, general, mode):
    heads, c_per = FUSED_SHAPE
    stable = mode == "stable"

    def run(env):
        g = TB._graph()
        if "topo" not in env.gpu:
            env.gpu["topo"] = [env.up32(a) for a in (
                g.row_indices, g.column_offset, g.row_offset,
                g.column_indices)]
        st = stream_of(env, general, stable)
        got = TB._run(env.gpu, st, heads, c_per, bf16)
        assert st.edge_softmax_stable_last() == int(stable)
        return dict(zip(("grad_h", "g_src", "g_dst"), got))

    def expect():
        g = TB._graph()
        _, _, _, _, _, pre, ref = TB._case(heads, c_per, bf16)
        # a source's gradients read the records of its destinations: they are
        # order-free where the source and all of them are one item each
        worst_in = np.zeros(g.v_src, dtype=np.int64)
        np.maximum.at(worst_in, g.row_indices.astype(np.int64) - g.src_start,
                      g.deg[g.dst_of_edge])
        degs = (np.maximum(g.out_deg, worst_in),
                np.maximum(g.out_deg, worst_in), g.deg)
        return {k: Expect(r, TH.RTOL * np.abs(r) + TH.ATOL, deg=d, prefill=p)
                for k, r, p, d in zip(("grad_h", "g_src", "g_dst"), ref, pre,
                                      degs)}

    def plan(shim):
        g = TB._graph()
        p = shim.gat_backward_fused_plan(
            heads * c_per, heads, 2 if bf16 else 4, 256, 256, g.v_src,
            g.batch, g.edges, general)
        p["grid"] = max(p["grid_csr"], p["grid_csc"])
        return p

    g0 = TB._graph()
    add(f"gat_backward_fused{'_bf16' if bf16 else ''}_"
        f"{'general' if general else 'auto'}_{mode}",
        "gat_backward_fused" + ("_bf16" if bf16 else ""), run, expect,
        lambda split: min(items_of(TB._graph().row_offset, split),
                          items_of(TB._graph().column_offset, split)),
        "group", plan, size=(g0.batch, g0.edges))


for _bf in (False, True):
    for _mode in MODES:
        _gat_forward_fused(_bf, _mode)
        for _form in ("auto", "general"):
            _gatv2_forward_fused(_bf, _form, _mode)
            _gat_backward_fused(_bf, _form == "general", _mode)


# --------------------------------------------------------------------------
# attention dropout at p = 0.3 (graph A, inputs, tolerance and run helpers of
# test_gpu_gat_dropout.py).  "dropped" is where the dropped weight is +0.0f:
# it must be the complement of shim.edge_dropout_keep in every configuration,
# the mask being a function of (seed, edge position, head) alone.
# --------------------------------------------------------------------------
DROP_P, DROP_SEED = 0.3, TD.SEED
DROP_HEADS, DROP_F = 3, 4


def _drop_gpu(env):
    if "A" not in env.gpu:
        g = TD._graph("A")
        env.gpu["A"] = {k: env.up32(g[k]) for k in ("coff", "rows", "pos")}
    return env.gpu


def _keep(width):
    from neutronstarlite_amd import shim
    g = TD._graph("A")
    return shim.edge_dropout_keep(DROP_SEED, DROP_P, 0,
                                  g["edges"] * width).reshape(g["edges"],
                                                              width)


def _dropped(w):
    return (np.ascontiguousarray(w).view(np.int32) == 0).astype(np.uint8)


def _drop_tol(ref):
    return TD.RTOL * np.abs(ref) + TD.ATOL


def _drop_forward(entry, mode):
    width = DROP_HEADS if entry == "attention" else DROP_F

    def run(env):
        st = stream_of(env, False, mode == "stable")
        if entry == "attention":
            w, w_perm, msum, alpha = TD._run_attention(
                _drop_gpu(env), "A", st, width, DROP_P, DROP_SEED)
        else:
            w, w_perm, alpha = TD._run_softmax(_drop_gpu(env), "A", st,
                                               width, DROP_P, DROP_SEED)
        assert st.edge_softmax_stable_last() == int(mode == "stable")
        res = {"w": w, "w_perm": w_perm, "alpha": alpha,
               "dropped": _dropped(w)}
        if entry == "attention":
            res["m_sum"] = msum
        return res

    def expect():
        g = TD._graph("A")
        keep = _keep(width)
        assert (keep == D.keep_edges(DROP_SEED, DROP_P, g["edges"],
                                     width)).all()
        if entry == "attention":
            _, _, m_ref, alpha = TD._attention_case("A", width)
        else:
            alpha = R.softmax_forward(g["coff"], TD._scores("A", width))
        w = alpha * D.factor(keep, DROP_P)
        perm = R.csc_to_csr(g["rows"])[0]
        ed = g["deg"][g["doe"]]
        e = {"w": Expect(w, _drop_tol(w), deg=ed),
             "w_perm": Expect(w[perm], _drop_tol(w[perm]), deg=ed[perm]),
             "alpha": Expect(alpha, _drop_tol(alpha), deg=ed),
             "dropped": Expect((~keep).astype(np.uint8), deg=ed)}
        if entry == "attention":
            e["m_sum"] = Expect(m_ref, deg=ed)
        return e

    g0 = TD._graph("A")
    add(f"{entry}_forward_drop_{mode}",
        "edge_attention_forward_drop" if entry == "attention"
        else "edge_softmax_forward_drop", run, expect,
        lambda split: items_of(TD._graph("A")["coff"], split),
        size=(g0["batch"], g0["edges"]))


def _drop_backward():
    f = 1

    def run(env):
        got, got_perm, dsum, _ = TD._run_backward(
            _drop_gpu(env), "A", env.st, f, True, DROP_P, DROP_SEED)
        return {"out": got, "perm": got_perm, "dst_sum": dsum}

    def expect():
        g = TD._graph("A")
        gw, alpha, lin = TD._backward_case("A", f)
        pre = np.zeros(g["batch"], dtype=np.float32)
        ref = D.softmax_backward(g["coff"], gw, alpha, _keep(f), DROP_P, lin,
                                 SLOPE, pre)
        perm = R.csc_to_csr(g["rows"])[0]
        ed = g["deg"][g["doe"]]
        return {"out": Expect(ref[0], _drop_tol(ref[0]), deg=ed),
                "perm": Expect(ref[0][perm], _drop_tol(ref[0][perm]),
                               deg=ed[perm]),
                "dst_sum": Expect(ref[2], _drop_tol(ref[2]), deg=g["deg"])}

    g0 = TD._graph("A")
    add("softmax_backward_drop", "edge_softmax_backward_drop", run, expect,
        lambda split: items_of(TD._graph("A")["coff"], split),
        size=(g0["batch"], g0["edges"]))


for _mode in MODES:
    _drop_forward("attention", _mode)
    _drop_forward("softmax", _mode)
_drop_backward()


# --------------------------------------------------------------------------
# the gather fused with the per-edge dot, f = 32 (graph, case, tolerances and
# run helper of test_gpu_gather_dot.py)
# --------------------------------------------------------------------------
DOT_F = 32


def _gather_dot():
    def run(env):
        ch = TGD._graph()
        if not hasattr(env, "dot_gpu"):
            perm = np.random.default_rng(5).permutation(
                ch.edge_size).astype(np.uint32)
            env.dot_gpu = {
                "dev": env.dev, "s": env.st, "roff": env.up32(ch.row_offset),
                "cols": env.up32(ch.column_indices),
                "w": env.up(ch.edge_weight_backward), "perm": perm,
                "d_perm": env.up32(perm)}
        rc, out, dot = TGD._run(env.dot_gpu, DOT_F, False)
        assert rc == 1, "the fused kernel must run at this width"
        return {"out": out, "dot": dot}

    def expect():
        ch = TGD._graph()
        _, _, out_ref, dot_ref, dot_mag = TGD._case(DOT_F)
        deg = np.diff(ch.row_offset.astype(np.int64))
        return {"out": Expect(out_ref, TGD.RTOL * np.abs(out_ref) + TGD.ATOL,
                              deg=deg),
                "dot": Expect(dot_ref, 1e-5 + 1e-4 * dot_mag,
                              deg=np.repeat(deg, deg))}

    ch0 = TGD._graph()
    add(f"gather_dot_f{DOT_F}", "gather_by_src_from_dst_dot", run, expect,
        lambda split: items_of(TGD._graph().row_offset, split),
        size=(int(ch0.src_n), int(ch0.edge_size)))


_gather_dot()


# --------------------------------------------------------------------------
# max / min aggregation on tied values, and its backward
# --------------------------------------------------------------------------
REDUCE_F = 5
NO_EDGE = RR.NO_EDGE


@functools.lru_cache(maxsize=None)
def reduce_case(form, op):
    """(x, y_ref, arg_ref): tie_input of test_gpu_reduce.py, six values only,
    so nearly every (destination, column) has its extremum more than once."""
    g = graph()
    if form == "csc":
        x = TR.tie_input(g.v_src, REDUCE_F, 14000)
        y, arg = RR.reduce_forward(g.column_offset, g.row_indices, x, op,
                                   g.src_start)
    else:
        x = TR.tie_input(g.edges, REDUCE_F, 14001)
        y, arg = RR.reduce_forward(g.column_offset, None, x, op)
    return x, y, arg


def reduce_tied_pairs(form, op):
    """(destination, column) pairs whose extremum sits on two edges or more."""
    g = graph()
    x, y, _ = reduce_case(form, op)
    seg = (x if form == "msg"
           else x[g.row_indices.astype(np.int64) - g.src_start])
    hits = R.segment_sum(seg == y[g.dst_of_edge], g.column_offset)
    return int((hits >= 2).sum())


def _reduce(form, op):
    def run(env):
        g = graph()
        x, _, _ = reduce_case(form, op)
        torch = env.torch
        d_x = env.up(x)
        y = torch.full((g.batch, REDUCE_F), 123.25, device=env.dev)
        arg = torch.full((g.batch, REDUCE_F), 7, dtype=torch.int32,
                         device=env.dev)
        env.st.reduce_by_dst_from_src(
            op, d_x.data_ptr(), y.data_ptr(), arg.data_ptr(),
            env.rows.data_ptr() if form == "csc" else None,
            env.coff.data_ptr(), g.src_start, g.src_start + g.v_src,
            g.src_start, g.src_start + g.batch, g.edges, g.batch, REDUCE_F)
        torch.cuda.synchronize()
        return {"y": y.cpu().numpy(), "arg": arg.cpu().numpy().view(np.uint32)}

    def expect():
        g = graph()
        _, y, arg = reduce_case(form, op)
        return {"y": Expect(y, exact="value", deg=g.deg),
                "arg": Expect(arg, deg=g.deg)}

    def plan(shim):
        g = graph()
        return shim.reduce_plan(REDUCE_F, 16, g.batch, g.edges, op)

    add(f"reduce_{form}_{op}", "reduce_by_dst_from_src", run, expect,
        lambda split: item_count("csc", split), "group", plan)


for _form in ("csc", "msg"):
    for _op in ("max", "min"):
        _reduce(_form, _op)


def _reduce_backward(form):
    """Integer gradients: every partial sum is exact, whatever the order of
    the atomics (test_backward_integer_gradients_bit_for_bit)."""
    def inputs():
        g = graph()
        _, _, arg = reduce_case(form, "max")
        grad = np.random.default_rng(14002).integers(
            -8, 9, (g.batch, REDUCE_F)).astype(np.float32)
        rows = g.v_src if form == "csc" else g.edges
        ref = RR.reduce_backward(arg, grad, g.row_indices
                                 if form == "csc" else None, rows,
                                 g.src_start if form == "csc" else 0)
        return arg, grad, rows, ref

    def run(env):
        g = graph()
        arg, grad, rows, _ = inputs()
        d_arg, d_g = env.up32(arg), env.up(grad)
        gx = env.buf((rows, REDUCE_F), np.zeros((rows, REDUCE_F)))
        env.st.reduce_backward(
            "max", d_g.data_ptr(), d_arg.data_ptr(),
            env.rows.data_ptr() if form == "csc" else None, g.src_start,
            gx.ptr, g.batch, REDUCE_F)
        return {"grad_input": gx.read("reduce_backward")}

    def expect():
        _, _, _, ref = inputs()
        assert np.abs(ref).max() < 2 ** 24
        # the indexed form's order is not fixed (the header): no bit-identity
        # claim; the message form writes every target once
        deg = None if form == "csc" else np.ones(len(ref), dtype=np.int64)
        return {"grad_input": Expect(ref, exact="value", deg=deg)}

    add(f"reduce_backward_{form}", "reduce_backward", run, expect,
        lambda split: graph().batch * REDUCE_F, "thread")


_reduce_backward("csc")
_reduce_backward("msg")


# --------------------------------------------------------------------------
# sampler: every destination of the graph, exact against sampler_ref
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def sampler_expected(fanout, forced):
    g = graph()
    table = np.full((g.batch, fanout), SENT, dtype=np.uint32)
    cnt = np.zeros(g.batch, dtype=np.uint32)
    for d in range(g.batch):
        src, k = SR.expected_sample(g.column_offset, g.row_indices, d, fanout,
                                    SR.SEED, forced=forced)
        table[d, :k] = src
        cnt[d] = k
    return table, cnt


def _sampler(fanout, forced):
    def run(env):
        g = graph()
        torch = env.torch
        dst = torch.arange(g.batch, dtype=torch.int32, device=env.dev)
        out_src = torch.full((g.batch * fanout + 256,), SENT,
                             dtype=torch.int32, device=env.dev)
        out_cnt = torch.full((g.batch + 256,), SENT, dtype=torch.int32,
                             device=env.dev)
        entry = (env.st.sample_reservoir_dbg_fallback if forced
                 else env.st.sample_reservoir)
        entry(env.coff.data_ptr(), env.rows.data_ptr(), dst.data_ptr(),
              g.batch, fanout, SR.SEED, out_src.data_ptr(), out_cnt.data_ptr())
        torch.cuda.synchronize()
        src = out_src.cpu().numpy().view(np.uint32)
        cnt = out_cnt.cpu().numpy().view(np.uint32)
        n = g.batch * fanout
        return {"out_src": src[:n].reshape(g.batch, fanout),
                "out_cnt": cnt[:g.batch],
                "guards": np.concatenate([src[n:], cnt[g.batch:]])}

    def expect():
        table, cnt = sampler_expected(fanout, forced)
        one = np.ones(graph().batch, dtype=np.int64)
        return {"out_src": Expect(table, deg=one),
                "out_cnt": Expect(cnt, deg=one),
                "guards": Expect(np.full(512, SENT, dtype=np.uint32))}

    add(f"sample_reservoir{'_dbg_fallback' if forced else ''}_fanout{fanout}",
        "sample_reservoir_dbg_fallback" if forced else "sample_reservoir",
        run, expect, lambda split: graph().batch)


for _fan in (4, 10):
    _sampler(_fan, False)
    _sampler(_fan, True)


# --------------------------------------------------------------------------
# message transfer and row pack: grid-strided over count * f elements
# --------------------------------------------------------------------------
T_COUNT, T_START, T_ROWS = 300, 100, 400


@functools.lru_cache(maxsize=None)
def transfer_case(f, repeat):
    """count records / indices with global ids from T_START on, a dense block
    of T_ROWS rows.  repeat: ids drawn with replacement from 120 rows, so
    most of them occur twice or more (the atomic entries must add them up);
    else they are distinct."""
    rng = np.random.default_rng([15000, f, int(repeat)])
    if repeat:
        ids = rng.integers(0, 120, T_COUNT)
    else:
        ids = rng.permutation(T_ROWS)[:T_COUNT]
    ids = (ids + T_START).astype(np.uint32)
    payload = rng.uniform(-1, 1, (T_COUNT, f)).astype(np.float32)
    msg = np.empty((T_COUNT, f + 1), dtype=np.float32)
    msg[:, 0] = ids.view(np.float32)
    msg[:, 1:] = payload
    dense = (rng.normal(size=(T_ROWS, f)) + 3).astype(np.float32)
    return ids, payload, msg, dense


def transfer_sum(ids, payload, dense):
    """(ref, mag, terms per row) of dense[id - T_START] += payload."""
    r = ids.astype(np.int64) - T_START
    ref, mag = dense.astype(np.float64), np.abs(dense.astype(np.float64))
    np.add.at(ref, r, payload.astype(np.float64))
    np.add.at(mag, r, np.abs(payload.astype(np.float64)))
    return ref, mag, np.bincount(r, minlength=T_ROWS)


def _transfer(entry, f):
    repeat = entry in ("aggregate_comm_result", "scatter_add_rows")

    def run(env):
        ids, payload, msg, dense = transfer_case(f, repeat)
        st = env.st
        d_msg, d_ids, d_pay = env.up(msg), env.up32(ids), env.up(payload)
        out = env.buf(dense.shape, dense)
        none = env.buf(dense.shape, dense)     # count = 0 writes nothing
        res = {}
        if entry == "deserialize_to_gpu":
            st.deserialize_to_gpu(out.ptr, d_msg.data_ptr(), T_COUNT, f,
                                  T_START, T_START + T_ROWS, sync=True)
            st.deserialize_to_gpu(none.ptr, d_msg.data_ptr(), 0, f, T_START,
                                  T_START + T_ROWS, sync=True)
            # sync = 0, then a dependent call on the same stream
            dep, packed = env.buf(dense.shape, dense), env.buf((T_COUNT, f))
            st.deserialize_to_gpu(dep.ptr, d_msg.data_ptr(), T_COUNT, f,
                                  T_START, T_START + T_ROWS, sync=False)
            st.gather_rows(dep.ptr, packed.ptr, d_ids.data_ptr(), T_COUNT,
                           T_START, f)
            res["dependent"] = packed.read("dependent gather_rows")
        elif entry == "aggregate_comm_result":
            st.aggregate_comm_result(out.ptr, d_msg.data_ptr(), T_COUNT, f,
                                     T_START, T_START + T_ROWS, sync=True)
            st.aggregate_comm_result(none.ptr, d_msg.data_ptr(), 0, f,
                                     T_START, T_START + T_ROWS, sync=True)
            dep, packed = env.buf(dense.shape, dense), env.buf((T_COUNT, f))
            st.aggregate_comm_result(dep.ptr, d_msg.data_ptr(), T_COUNT, f,
                                     T_START, T_START + T_ROWS, sync=False)
            st.gather_rows(dep.ptr, packed.ptr, d_ids.data_ptr(), T_COUNT,
                           T_START, f)
            res["dependent"] = packed.read("dependent gather_rows")
        elif entry == "gather_rows":
            d_dense = env.up(dense)
            out = env.buf((T_COUNT, f))
            none = env.buf((T_COUNT, f), payload)
            st.gather_rows(d_dense.data_ptr(), out.ptr, d_ids.data_ptr(),
                           T_COUNT, T_START, f)
            st.gather_rows(d_dense.data_ptr(), none.ptr, d_ids.data_ptr(), 0,
                           T_START, f)
        else:
            call = getattr(st, entry)
            call(out.ptr, d_pay.data_ptr(), d_ids.data_ptr(), T_COUNT,
                 T_START, f)
            call(none.ptr, d_pay.data_ptr(), d_ids.data_ptr(), 0, T_START, f)
        res["out"] = out.read(entry)
        res["count0"] = none.read(entry + " count 0")
        return res

    def expect():
        ids, payload, msg, dense = transfer_case(f, repeat)
        r = ids.astype(np.int64) - T_START
        one = np.ones(T_COUNT, dtype=np.int64)
        if entry == "gather_rows":
            return {"out": Expect(dense[r], deg=one),
                    "count0": Expect(payload)}
        e = {"count0": Expect(dense)}
        if repeat:
            # the project tolerance, as test_gpu_parity.py holds these entries
            ref, mag, terms = transfer_sum(ids, payload, dense)
            bound = TP.RTOL * np.abs(ref) + TP.ATOL
            e["out"] = Expect(ref, bound, deg=terms, atomic=True,
                              prefill=dense)
            if entry == "aggregate_comm_result":
                e["dependent"] = Expect(ref[r], bound[r])
            return e
        ref = dense.copy()
        ref[r] = payload
        e["out"] = Expect(ref, deg=np.bincount(r, minlength=T_ROWS),
                          prefill=dense)
        if entry == "deserialize_to_gpu":
            e["dependent"] = Expect(payload, deg=one)
        return e

    add(f"{entry}_f{f}", entry, run, expect, lambda split: T_COUNT * f,
        "thread")


TRANSFER_ENTRIES = ("deserialize_to_gpu", "aggregate_comm_result",
                    "gather_rows", "scatter_rows", "scatter_add_rows")
for _entry in TRANSFER_ENTRIES:
    for _f in (37, 1):
        _transfer(_entry, _f)


# --------------------------------------------------------------------------
# the driver
# --------------------------------------------------------------------------
def resolve(only):
    """The case names of an --only list; an unknown name is an error."""
    if not only:
        return list(CASES)
    names = [n for n in only.split(",") if n]
    unknown = [n for n in names if n not in CASES]
    if unknown:
        raise SystemExit(f"unknown case(s): {', '.join(unknown)}")
    return names


def check_latched(shim):
    """The plan functions read the statics the launches read: at a shape
    whose uncapped grid is above the cap the reported grid is the cap."""
    want = env_u32("NTS_MAX_BLOCKS", DEFAULT_CAP)
    got = shim.gather_plan(**LATCH_SHAPE)["grid"]
    assert got == want, (f"NTS_MAX_BLOCKS not latched: plan grid {got}, "
                         f"environment says {want}")
    return got


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True, help="the .npz to write")
    ap.add_argument("--only", default="", help="comma-separated case names")
    args = ap.parse_args(argv)
    names = resolve(args.only)

    t0 = time.time()
    env = make_env()
    split = env_u32("NTS_SPLIT", DEFAULT_SPLIT)
    g = graph()
    meta = {"env": env_seen(), "split": split,
            "max_blocks": check_latched(env.shim), "cases": {}}
    arrays = {}
    for name in names:
        case = CASES[name]
        t1 = time.time()
        outs = case.run(env)          # the first exception ends the process
        env.torch.cuda.synchronize()
        for key, a in outs.items():
            arrays[f"{name}/{key}"] = a
        plan = case.plan(env.shim) if case.plan else None
        meta["cases"][name] = {
            "batch": case.size[0] if case.size else g.batch,
            "edges": case.size[1] if case.size else g.edges,
            "work": case.work(split),
            "unit": case.unit, "plan": plan,
            "seconds": round(time.time() - t1, 3)}
    meta["seconds"] = round(time.time() - t0, 3)
    arrays["__meta__"] = np.array(json.dumps(meta))
    np.savez(args.out, **arrays)
    print(f"grid_cases: {len(names)} cases in {meta['seconds']} s, "
          f"environment {meta['env']}")


if __name__ == "__main__":
    main()
