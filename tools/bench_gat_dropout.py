#!/usr/bin/env python
"""Attention dropout against no dropout on GAT and GATv2 layers, in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times forward + backward layer steps of

    k1    GATLayer at K=1 (the single-head layer, fused gather-dot backward)
    k8    GATLayer at K=8 heads
    v8    GATv2Layer at K=8 heads

each with dropout=0.0 and with dropout=0.6 (--p), step by step in turn
(k1 p=0, k1 p=0.6, k8 p=0, k8 p=0.6, v8 p=0, ...) after a warm-up of every
combination, so drift of the machine hits all alike.  The baseline of a
dropout step is the dropout=0.0 step of the same layer in the same process,
never a recorded number.  Kernel time is the sum of the nts_stream_kernel_ns
tags (HIP events around the launches) of the layer's two stream wrappers,
taken apart into the forward call, the backward call and, over both, the
NTS_KTAG_EDGE tag (the only part dropout changes).  --rounds R repeats the
alternation R times and reports every round and the spread (max - min over
the rounds, relative to their mean).

Byte model: the forward's normalize pass writes the softmax AND the dropped
weights in CSC order (4*E*K more bytes: 3.6 GB at K=8, 0.46 GB at K=1); the
backward moves the bytes it moves without dropout and regenerates the mask
(two 64-bit multiplies per value) in its pass 1.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_gat_dropout.py --steps 5 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

TAGS = ("fwd", "bwd", "deser", "aggmsg", "items", "edge")
EDGE = TAGS.index("edge")
KNOWN = {"k1": ("gat", 1), "k8": ("gat", 8), "v8": ("gatv2", 8)}
SEED = 11


def log(msg):
    print(f"[bench_gat_dropout] {msg}", file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--p", type=float, default=0.6)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    ap.add_argument("--variants", default="k1,k8,v8")
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
    combos = [(n, p) for n in names for p in (0.0, args.p)]

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
        return np.array(
            [layer.stream.kernel_ns(t) + layer.scalar_stream.kernel_ns(t)
             for t in range(len(TAGS))], dtype=np.float64)

    def step(n, p):
        """One forward + backward: (forward kernel ms, backward kernel ms,
        edge-tag ms of both, wall ms)."""
        layer = layers[n]
        torch.cuda.synchronize()
        k0, t = kernel_ns(layer), time.perf_counter()
        y, saved = layer.forward(*inputs[n], 0.2, p, SEED)
        torch.cuda.synchronize()
        k1 = kernel_ns(layer)
        layer.backward(gy, saved)
        assert ("p" in saved) == (p > 0)
        del y, saved
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        k2 = kernel_ns(layer)
        return np.array([(k1 - k0).sum() / 1e6, (k2 - k1).sum() / 1e6,
                         (k2 - k0)[EDGE] / 1e6, wall])

    for _ in range(args.warmup):
        for c in combos:
            step(*c)
    log("warm-up done")

    rounds = []
    for _ in range(args.rounds):
        acc = {c: np.zeros(4) for c in combos}
        for _ in range(args.steps):
            for c in combos:
                acc[c] += step(*c)
        rounds.append({c: acc[c] / args.steps for c in combos})

    cols = ("forward_ms", "backward_ms", "edge_tag_ms", "wall_ms")

    def report(c):
        per = np.array([r[c] for r in rounds])          # rounds x 4
        mean = per.mean(axis=0)
        out = {"layer": KNOWN[c[0]][0], "heads": KNOWN[c[0]][1],
               "dropout": c[1]}
        for i, col in enumerate(cols):
            out[col] = round(float(mean[i]), 3)
            out[col + "_rounds"] = [round(float(q), 3) for q in per[:, i]]
            out[col + "_spread"] = round(
                float((per[:, i].max() - per[:, i].min()) / mean[i]), 4)
        return out

    out = {"tool": "bench_gat_dropout", "V": v, "E": e_total, "f": f,
           "p": args.p, "steps": args.steps, "warmup": args.warmup,
           "rounds": args.rounds,
           "variants": {f"{n}@{p}": report((n, p)) for n, p in combos}}
    extra = {}
    for n in names:
        d, z = (n, args.p), (n, 0.0)
        extra[n] = {
            col: {"ms": round(float(np.mean([r[d][i] - r[z][i]
                                             for r in rounds])), 3),
                  "rounds_ms": [round(float(r[d][i] - r[z][i]), 3)
                                for r in rounds],
                  "ratio": round(float(np.mean([r[d][i] for r in rounds])
                                       / np.mean([r[z][i] for r in rounds])),
                                 4)}
            for i, col in enumerate(cols)}
    out["dropout_minus_none"] = extra
    print(json.dumps(out), flush=True)
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()


if __name__ == "__main__":
    main()
