#!/usr/bin/env python
"""A DotAttentionLayer training step with cached edge state against one that
recomputes the attention weights, in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times the two steps

    cached      y, saved = layer.forward(...);           layer.backward(gy, saved)
    recompute   y, saved = layer.forward_recompute(...); layer.backward(gy, saved)

of

    k1, k1s   one head, default softmax and DotAttentionLayer(stable=True)
    k8, k8s   K=8 heads at the same total width, default and stable

each with float32 rows and (suffix b) with bfloat16 rows, step by step in turn
(k1 cached, k1 recompute, k1s cached, ...) after a warm-up of every variant,
so drift of the machine hits all alike.  The baseline of a recompute figure is
the cached step of the same variant in the same process, never a recorded
number.  Kernel time is the sum of the nts_stream_kernel_ns tags (HIP events
around the launches) of the variant's stream wrapper, reported per tag: EDGE
(cached: the two edge dots, softmax and softmax backward; recompute: the
record pass), FWD (cached: the two CSC gathers, y in the forward and grad_q in
the backward; recompute: the one-pass fused forward), BWD (cached: the two CSR
gathers, grad_v and grad_k; recompute: the CSC and the CSR walk) and ITEMS.  The q scaling and the two gradient scalings of the
cached step are torch kernels and appear in wall_ms only.  The peak-memory
figure is the rise of torch.cuda.max_memory_allocated() over one step (the
stream's own scratch is the library's).  --rounds R repeats the alternation R
times and reports every round and the spread (max - min over the rounds,
relative to their mean).  During the warm-up the gradients of the two steps
are compared (largest absolute difference beside the largest magnitude) and
logged.

"gathers" is the yardstick of the two walks: what the byte model counts for
them is four row gathers per edge, so four plain heads gathers with [E, K]
weights (k and v over the CSC, q and grad_y over the CSR) are timed in the
same alternation, per head count and row type; walks_over_gathers is the
recompute step's BWD tag over their sum.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 900 python tools/bench_dot_recompute.py --steps 3 --warmup 1
"""
import argparse
import copy
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAGS = ("fwd", "bwd", "deser", "aggmsg", "items", "edge")
COLS = ("fwd_ms", "bwd_ms", "edge_ms", "items_ms", "kernel_ms", "wall_ms",
        "peak_mb")
GRADS = ("grad_q", "grad_k", "grad_v")


def log(msg):
    print(f"[bench_dot_recompute] {msg}", file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    ap.add_argument("--variants",
                    default="k1,k1s,k8,k8s,k1b,k1sb,k8b,k8sb")
    args = ap.parse_args(argv)

    import torch

    from neutronstarlite_amd import graph as G
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.gat import DotAttentionLayer

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
    base = DotAttentionLayer(ch, v, dev)  # topology and slot maps, shared below
    log(f"layer topology built in {time.time() - t0:.1f}s")
    dc = base.ch                          # the chunk's device arrays

    def variant(heads, stable):
        """A layer on base's device topology with its own stream wrapper (its
        own timing tags and its own softmax mode)."""
        layer = copy.copy(base)
        layer.heads = heads
        layer.stable = stable
        layer.stream = shim.Stream.wrap_torch_current()
        layer.stream.edge_softmax_stable(stable)
        layer.stream.timing(True)
        return layer

    known = {}
    for heads in (1, 8):
        for stable in (False, True):
            for bf16 in (False, True):
                known[f"k{heads}{'s' if stable else ''}{'b' if bf16 else ''}"] = (
                    heads, stable, bf16)
    names = [n for n in args.variants.split(",") if n]
    layers = {n: variant(*known[n][:2]) for n in names}

    f = args.f
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    q, k, vv, gy = (up(rng.uniform(-1, 1, size=(v, f))) for _ in range(4))
    rows = {False: (q, k, vv),
            True: tuple(t.to(torch.bfloat16) for t in (q, k, vv))}

    def kernel_ns(stream):
        return np.array([stream.kernel_ns(t) for t in range(len(TAGS))],
                        dtype=np.float64)

    def step(n, kind, keep=False):
        """One forward + backward: the COLS figures and, with keep, the three
        gradients."""
        layer = layers[n]
        heads, stable, bf16 = known[n]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        m0 = torch.cuda.max_memory_allocated()
        k0, t = kernel_ns(layer.stream), time.perf_counter()
        forward = (layer.forward if kind == "cached"
                   else layer.forward_recompute)
        y, saved = forward(*rows[bf16])
        assert ("recompute" in saved) == (kind == "recompute")
        grads = layer.backward(gy, saved)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        kn = (kernel_ns(layer.stream) - k0) / 1e6
        rise = (torch.cuda.max_memory_allocated() - m0) / 2 ** 20
        assert layer.stream.edge_softmax_stable_last() == int(stable)
        del y, saved
        fig = np.array([kn[TAGS.index("fwd")], kn[TAGS.index("bwd")],
                        kn[TAGS.index("edge")], kn[TAGS.index("items")],
                        kn.sum(), wall, rise])
        return (fig, grads) if keep else fig

    # the yardstick: four plain heads gathers per (heads, row type)
    gst = shim.Stream.wrap_torch_current()
    gst.timing(True)
    gst.items_reuse(1)
    combos = sorted({(known[n][0], known[n][2]) for n in names})
    wts = {heads: torch.rand(e_total, heads, device=dev)
           for heads in sorted({c[0] for c in combos})}
    g_out = torch.zeros(v, f, device=dev)

    def gathers(heads, bf16):
        """Kernel ms (all tags but ITEMS) of the four gathers."""
        qq, kk, vr = rows[bf16]
        wt = wts[heads].data_ptr()
        csc = (dc.row_indices.data_ptr(), dc.column_offset.data_ptr(),
               dc.src_s, dc.src_e, dc.dst_s, dc.dst_e,
               e_total, dc.dst_n, f, heads)
        csr = (dc.row_offset.data_ptr(), dc.column_indices.data_ptr(),
               dc.src_s, dc.src_e, dc.dst_s, dc.dst_e,
               e_total, dc.src_n, f, heads)
        by_dst = (gst.gather_by_dst_from_src_heads_bf16 if bf16
                  else gst.gather_by_dst_from_src_heads)
        by_src = (gst.gather_by_src_from_dst_heads_bf16 if bf16
                  else gst.gather_by_src_from_dst_heads)
        torch.cuda.synchronize()
        k0 = kernel_ns(gst)
        by_dst(kk.data_ptr(), g_out.data_ptr(), wt, *csc)
        by_dst(vr.data_ptr(), g_out.data_ptr(), wt, *csc)
        by_src(qq.data_ptr(), g_out.data_ptr(), wt, *csr)
        gst.gather_by_src_from_dst_heads(gy.data_ptr(), g_out.data_ptr(), wt,
                                         *csr)
        torch.cuda.synchronize()
        kn = (kernel_ns(gst) - k0) / 1e6
        return float(kn.sum() - kn[TAGS.index("items")])

    agree = {}
    for i in range(max(1, args.warmup)):
        for n in names:
            _, g_c = step(n, "cached", keep=True)
            _, g_r = step(n, "recompute", keep=True)
            if i == 0:
                agree[n] = {
                    name: {"max_abs_diff": float((a - b).abs().max()),
                           "max_abs": float(a.abs().max())}
                    for name, a, b in zip(GRADS, g_c, g_r)}
                log(f"{n}: cached vs recompute " + ", ".join(
                    f"{k} {d['max_abs_diff']:.3e} of {d['max_abs']:.3e}"
                    for k, d in agree[n].items()))
            del g_c, g_r
        for c in combos:
            gathers(*c)
    log("warm-up done")

    kinds = ("cached", "recompute")
    rounds, g_rounds = [], []
    for _ in range(args.rounds):
        acc = {(n, k): np.zeros(len(COLS)) for n in names for k in kinds}
        g_acc = {c: 0.0 for c in combos}
        for _ in range(args.steps):
            for n in names:
                for k in kinds:
                    acc[n, k] += step(n, k)
            for c in combos:
                g_acc[c] += gathers(*c)
        rounds.append({key: a / args.steps for key, a in acc.items()})
        g_rounds.append({c: a / args.steps for c, a in g_acc.items()})

    def report(n, k):
        per = np.array([r[n, k] for r in rounds])          # rounds x COLS
        mean = per.mean(axis=0)
        out = {}
        for i, c in enumerate(COLS):
            out[c] = round(float(mean[i]), 3)
            out[c + "_rounds"] = [round(float(p), 3) for p in per[:, i]]
            out[c + "_spread"] = round(
                float((per[:, i].max() - per[:, i].min()) / mean[i]), 4) \
                if mean[i] else 0.0
        return out

    kcol, bcol = COLS.index("kernel_ms"), COLS.index("bwd_ms")
    out = {"tool": "bench_dot_recompute", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {}, "gathers": {}}
    for heads, bf16 in combos:
        per = [r[heads, bf16] for r in g_rounds]
        out["gathers"][f"k{heads}{'b' if bf16 else ''}"] = {
            "four_gathers_ms": round(float(np.mean(per)), 3),
            "four_gathers_ms_rounds": [round(p, 3) for p in per]}
    for n in names:
        heads, stable, bf16 = known[n]
        rep = {"heads": heads, "stable": stable, "bf16": bf16,
               "agreement": agree[n]}
        for k in kinds:
            rep[k] = report(n, k)
        rep["recompute_over_cached"] = {
            "kernel_ms": round(rep["recompute"]["kernel_ms"]
                               / rep["cached"]["kernel_ms"], 4),
            "kernel_ms_rounds": [
                round(float(r[n, "recompute"][kcol] / r[n, "cached"][kcol]), 4)
                for r in rounds]}
        rep["walks_over_gathers"] = [
            round(float(r[n, "recompute"][bcol] / g[heads, bf16]), 4)
            for r, g in zip(rounds, g_rounds)]
        out["variants"][n] = rep
    print(json.dumps(out), flush=True)
    for layer in layers.values():
        layer.stream.destroy()
    gst.destroy()


if __name__ == "__main__":
    main()
