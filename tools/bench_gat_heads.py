#!/usr/bin/env python
"""Single-head against multi-head GAT layers, in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times forward + backward layer steps of

    a       the single-head layer (fused CSR gather + edge dot)
    b       the heads call chain at K=1: unfused gather + dot, one weight
            column (GATLayer's private _heads_path switch)
    k4, k8  K=4 and K=8 heads at the same total width
    k4g, k8g  the same with the general forms of the heads edge kernels
            (nts_heads_dbg_general), i.e. without the power-of-two fast paths

step by step in turn (a, b, k4, ... , a, b, ...) after a warm-up of every
variant, so drift of the machine hits all alike.  Kernel time is the sum of
the nts_stream_kernel_ns tags (HIP events around the launches) of the
variant's two stream wrappers; wall time is the whole step, torch allocation
and zeroing included.  --rounds R repeats the alternation R times and reports
every round: the run-to-run spread to judge the ratios by.

Byte model of one step, edge terms only (V-sized terms are under 1 %): three
row passes (CSC gather, CSR gather, edge dot) of 4f bytes per edge, six index
or slot-map reads of 4 bytes, and 18 passes over an [E, K] fp32 array (6
forward, 12 backward), so E * (12 f + 24 + 72 K) bytes.  Against b (K=1) a
K-head step adds 72 (K-1) bytes per edge: 1.13x at K=4, 1.31x at K=8, f=128.
a - b is the price of leaving the fused gather-dot single-head.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_gat_heads.py --steps 5 --warmup 2
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


def log(msg):
    print(f"[bench_gat_heads] {msg}", file=sys.stderr, flush=True)


def model_bytes(e, f, heads):
    """Edge terms of one forward + backward step (see the module docstring)."""
    return e * (12 * f + 24 + 72 * heads)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    ap.add_argument("--variants", default="a,b,k4,k8,k4g,k8g")
    args = ap.parse_args(argv)

    import torch

    from neutronstarlite_amd import graph as G
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.gat import GATLayer

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

    def variant(heads, heads_path, general):
        """A layer on base's device topology with its own stream wrappers
        (its own timing tags)."""
        layer = copy.copy(base)
        layer.heads = heads
        layer._heads_path = heads_path
        layer.stream = shim.Stream.wrap_torch_current()
        layer.scalar_stream = shim.Stream.wrap_torch_current()
        for st in (layer.stream, layer.scalar_stream):
            st.timing(True)
            st.heads_dbg_general(general)
        return layer

    known = {"a": (1, False, False), "b": (1, True, False),
             "k4": (4, True, False), "k8": (8, True, False),
             "k4g": (4, True, True), "k8g": (8, True, True)}
    names = [n for n in args.variants.split(",") if n]
    layers = {n: variant(*known[n]) for n in names}

    f = args.f
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    x = up(rng.uniform(-1, 1, size=(v, f)))
    gy = up(rng.uniform(-1, 1, size=(v, f)))
    scalars = {}
    for n in names:
        heads, heads_path, _ = known[n]
        a_src = up(rng.uniform(-1, 1, size=(heads, f // heads)))
        a_dst = up(rng.uniform(-1, 1, size=(heads, f // heads)))
        x3 = x.view(v, heads, f // heads)
        s_src, s_dst = (x3 * a_src).sum(-1), (x3 * a_dst).sum(-1)
        if not heads_path:          # the single-head layer takes [V]
            s_src, s_dst = s_src[:, 0].contiguous(), s_dst[:, 0].contiguous()
        scalars[n] = (s_src, s_dst)

    def kernel_ns(layer):
        return [layer.stream.kernel_ns(t) + layer.scalar_stream.kernel_ns(t)
                for t in range(len(TAGS))]

    def step(n):
        """One forward + backward; returns (per-tag kernel ms, wall ms)."""
        layer = layers[n]
        torch.cuda.synchronize()
        k0, t = kernel_ns(layer), time.perf_counter()
        y, saved = layer.forward(x, *scalars[n])
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

    def report(n):
        ks = [float(r[n][0].sum()) for r in rounds]
        tags = sum(r[n][0] for r in rounds) / len(rounds)
        heads = known[n][0]
        return {"heads": heads, "heads_path": known[n][1],
                "general_forms": known[n][2],
                "ms_per_step": round(sum(ks) / len(ks), 3),
                "rounds_ms_per_step": [round(k, 3) for k in ks],
                "wall_ms_per_step": round(
                    sum(r[n][1] for r in rounds) / len(rounds), 3),
                "tags_ms_per_step": {t: round(float(m), 3)
                                     for t, m in zip(TAGS, tags) if m},
                "model_bytes_per_step": model_bytes(e_total, f, heads)}

    out = {"tool": "bench_gat_heads", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {n: report(n) for n in names}}
    if "b" in names:
        b = out["variants"]["b"]
        out["ratio_vs_b"] = {
            n: {"measured": round(r["ms_per_step"] / b["ms_per_step"], 4),
                "rounds": [round(float(rd[n][0].sum() / rd["b"][0].sum()), 4)
                           for rd in rounds],
                "model": round(r["model_bytes_per_step"]
                               / b["model_bytes_per_step"], 4)}
            for n, r in out["variants"].items() if n != "b"}
    print(json.dumps(out), flush=True)
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()


if __name__ == "__main__":
    main()
