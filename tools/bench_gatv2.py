#!/usr/bin/env python
"""GAT against GATv2 layers, and the GATv2 kernels against their yardsticks,
in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times forward + backward layer steps of

    g1, g8  GATLayer at K=1 (the single-head layer) and K=8 heads
    v1, v8  GATv2Layer at K=1 and K=8

step by step in turn (g1, g8, v1, v8, g1, ...) after a warm-up of every
variant, so drift of the machine hits all alike.  Kernel time is the sum of
the nts_stream_kernel_ns tags (HIP events around the launches) of the
variant's stream wrappers; wall time is the whole step, torch allocation and
zeroing included.  --rounds R repeats the alternation R times and reports
every round: the run-to-run spread to judge the differences by.

Then, per K, single entries on the same inputs, again alternating call by
call, in ms per call:

    score     nts_edge_gatv2_score
    dot       nts_edge_dot_heads: the same two row reads per edge and the same
              [E, K] write, so the yardstick of the score kernel
    bwd_csc   nts_edge_gatv2_backward over the CSC with grad_att
    bwd_csr   nts_edge_gatv2_backward over the CSR without it
    gather    nts_gather_by_dst_from_src_heads: one row read and one [E, K]
              read per edge, the yardstick of a backward walk

Byte prior (nobody measured it before this tool): a GATv2 step is a heads-GAT
step plus one dot-like pass (the score) and two gather-like passes (the
walks).

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_gatv2.py --steps 5 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAGS = ("fwd", "bwd", "deser", "aggmsg", "items", "edge")
KNOWN = {"g1": ("gat", 1), "g8": ("gat", 8), "v1": ("gatv2", 1),
         "v8": ("gatv2", 8)}
ENTRIES = ("score", "dot", "bwd_csc", "bwd_csr", "gather")


def log(msg):
    print(f"[bench_gatv2] {msg}", file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    ap.add_argument("--variants", default="g1,g8,v1,v8")
    ap.add_argument("--entry-heads", default="1,8",
                    help="K of the single-entry comparison ('' = skip it)")
    args = ap.parse_args(argv)

    import torch

    from neutronstarlite_amd import graph as G
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.gat import GATLayer, GATv2Layer

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)

    v, e = (232_965, 114_000_000) if args.graph == "reddit" else (
        10_000, 200_000)
    t0 = time.time()
    edges = G.rmat_edges(v, e, seed=7)
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    ch = G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]
    e_total = len(edges)
    del edges, w
    log(f"graph V={v} E={e_total} built in {time.time() - t0:.1f}s")

    t0 = time.time()
    base = GATLayer(ch, v, dev)     # topology and slot maps, shared below
    log(f"layer topology built in {time.time() - t0:.1f}s")

    def variant(kind, heads):
        """A layer on base's device topology with its own stream wrappers
        (its own timing tags)."""
        cls = GATLayer if kind == "gat" else GATv2Layer
        layer = cls.__new__(cls)
        layer.__dict__.update(base.__dict__)
        layer.heads = heads
        if kind == "gat":
            layer._heads_path = heads > 1
        layer.stream = shim.Stream.wrap_torch_current()
        layer.scalar_stream = shim.Stream.wrap_torch_current()
        for st in (layer.stream, layer.scalar_stream):
            st.timing(True)
        return layer

    names = [n for n in args.variants.split(",") if n]
    layers = {n: variant(*KNOWN[n]) for n in names}

    f = args.f
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    x = up(rng.uniform(-1, 1, size=(v, f)))
    x_r = up(rng.uniform(-1, 1, size=(v, f)))
    gy = up(rng.uniform(-1, 1, size=(v, f)))
    inputs = {}
    for n in names:
        kind, heads = KNOWN[n]
        c_per = f // heads
        if kind == "gat":
            a_src = up(rng.uniform(-1, 1, size=(heads, c_per)))
            a_dst = up(rng.uniform(-1, 1, size=(heads, c_per)))
            x3 = x.view(v, heads, c_per)
            s_src, s_dst = (x3 * a_src).sum(-1), (x3 * a_dst).sum(-1)
            if heads == 1:          # the single-head layer takes [V]
                s_src, s_dst = (s_src[:, 0].contiguous(),
                                s_dst[:, 0].contiguous())
            inputs[n] = (x, s_src, s_dst)
        else:
            att = up(rng.normal(size=(heads, c_per)) / np.sqrt(c_per))
            inputs[n] = (x, x_r, att)

    def kernel_ns(layer):
        return [layer.stream.kernel_ns(t) + layer.scalar_stream.kernel_ns(t)
                for t in range(len(TAGS))]

    def step(n):
        """One forward + backward; returns (per-tag kernel ms, wall ms)."""
        layer = layers[n]
        torch.cuda.synchronize()
        k0, t = kernel_ns(layer), time.perf_counter()
        y, saved = layer.forward(*inputs[n])
        layer.backward(gy, saved)
        del y, saved
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        return [(b - a) / 1e6 for a, b in zip(k0, kernel_ns(layer))], wall

    for _ in range(args.warmup):
        for n in names:
            step(n)
    log("warm-up done")

    rounds = []
    for _ in range(args.rounds):
        acc = {n: [np.zeros(len(TAGS)), 0.0] for n in names}
        for _ in range(args.steps):
            for n in names:
                k, wall = step(n)
                acc[n][0] += k
                acc[n][1] += wall
        rounds.append({n: (acc[n][0] / args.steps, acc[n][1] / args.steps)
                       for n in names})
    log("layer steps done")

    def report(n):
        ks = [float(r[n][0].sum()) for r in rounds]
        tags = sum(r[n][0] for r in rounds) / len(rounds)
        return {"layer": KNOWN[n][0], "heads": KNOWN[n][1],
                "ms_per_step": round(sum(ks) / len(ks), 3),
                "rounds_ms_per_step": [round(k, 3) for k in ks],
                "wall_ms_per_step": round(
                    sum(r[n][1] for r in rounds) / len(rounds), 3),
                "tags_ms_per_step": {t: round(float(m), 3)
                                     for t, m in zip(TAGS, tags) if m}}

    out = {"tool": "bench_gatv2", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {n: report(n) for n in names}}
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()

    # ---- single entries on the same inputs ----
    c, E = base.ch, base.E
    st = shim.Stream.wrap_torch_current()
    st.timing(True)
    st.items_reuse(1)
    out["entries_ms_per_call"] = {}
    for heads in [int(k) for k in args.entry_heads.split(",") if k]:
        att = up(rng.normal(size=(heads, f // heads)))
        ek = torch.empty(E, heads, device=dev)
        wk = torch.rand(E, heads, device=dev)
        g_r, g_l = torch.zeros(v, f, device=dev), torch.zeros(v, f, device=dev)
        g_att = torch.zeros(f, device=dev)
        y = torch.zeros(v, f, device=dev)
        p = lambda t: t.data_ptr()
        calls = {
            "score": lambda: st.edge_gatv2_score(
                p(ek), p(x_r), p(x), p(att), 0.2, p(c.row_indices),
                p(c.column_offset), c.src_s, c.dst_n, E, f, heads),
            "dot": lambda: st.edge_dot_heads(
                p(ek), p(x_r), p(x), p(c.row_indices), p(c.column_offset),
                c.src_s, c.dst_n, E, f, heads),
            "bwd_csc": lambda: st.edge_gatv2_backward(
                p(g_r), p(g_att), p(wk), p(x_r), p(x), p(att), 0.2,
                p(c.column_offset), p(c.row_indices), c.src_s, c.dst_n, E, f,
                heads),
            "bwd_csr": lambda: st.edge_gatv2_backward(
                p(g_l), None, p(wk), p(x), p(x_r), p(att), 0.2,
                p(c.row_offset), p(c.column_indices), c.dst_s, c.src_n, E, f,
                heads),
            "gather": lambda: st.gather_by_dst_from_src_heads(
                p(x), p(y), p(wk), p(c.row_indices), p(c.column_offset),
                c.src_s, c.src_e, c.dst_s, c.dst_e, E, c.dst_n, f, heads)}
        tag = {"score": 5, "dot": 5, "bwd_csc": 5, "bwd_csr": 5, "gather": 0}

        def timed(name):
            torch.cuda.synchronize()
            k0 = st.kernel_ns(tag[name])
            calls[name]()
            torch.cuda.synchronize()
            return (st.kernel_ns(tag[name]) - k0) / 1e6

        for _ in range(args.warmup):
            for name in ENTRIES:
                timed(name)
        per_round = []
        for _ in range(args.rounds):
            acc = {name: 0.0 for name in ENTRIES}
            for _ in range(args.steps):
                for name in ENTRIES:
                    acc[name] += timed(name)
            per_round.append({n: acc[n] / args.steps for n in ENTRIES})
        res = {n: {"ms": round(sum(r[n] for r in per_round) / len(per_round), 3),
                   "rounds": [round(r[n], 3) for r in per_round]}
               for n in ENTRIES}
        res["score_over_dot"] = round(res["score"]["ms"] / res["dot"]["ms"], 4)
        res["bwd_csc_over_gather"] = round(
            res["bwd_csc"]["ms"] / res["gather"]["ms"], 4)
        res["bwd_csr_over_gather"] = round(
            res["bwd_csr"]["ms"] / res["gather"]["ms"], 4)
        out["entries_ms_per_call"][f"K={heads}"] = res
        log(f"entries at K={heads} done")
    st.destroy()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
