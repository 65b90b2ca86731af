#!/usr/bin/env python
"""Default against stable (max-subtracted) softmax GAT layers, in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times forward + backward layer steps of

    k1, k1s   the single-head layer, default and GATLayer(stable=True)
    k8, k8s   K=8 heads at the same total width, default and stable

step by step in turn (k1, k1s, k8, k8s, k1, ...) after a warm-up of every
variant, so drift of the machine hits all alike.  The baseline of a stable
variant is the default variant of the same process, never a recorded number.
Kernel time is the sum of the nts_stream_kernel_ns tags (HIP events around
the launches) of the variant's two stream wrappers, taken apart into the
forward call, the backward call and, over both, the NTS_KTAG_EDGE tag (the
attention forward's two passes are its only part the mode changes).  --rounds
R repeats the alternation R times and reports every round and the spread
(max - min over the rounds, relative to their mean).

Byte model: the stable form moves the bytes of the default one (pass 1 reads
the index list and the scalars and writes m_sum and the stash, pass 2 reads
the stash and writes the softmax twice); its per-destination state is 8 bytes
where the default's is 4 (V*K-sized, under 1 % of the E*K-sized terms).  It
adds one exp per value in pass 2 and, for destinations split into several
work items, a sum pass that re-reads their stash (E*K*4 bytes at most).

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_gat_stable.py --steps 5 --warmup 2
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
EDGE = TAGS.index("edge")


def log(msg):
    print(f"[bench_gat_stable] {msg}", file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    ap.add_argument("--variants", default="k1,k1s,k8,k8s")
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

    def variant(heads, stable):
        """A layer on base's device topology with its own stream wrappers
        (its own timing tags and its own softmax mode)."""
        layer = copy.copy(base)
        layer.heads = heads
        layer._heads_path = heads > 1
        layer.stable = stable
        layer.stream = shim.Stream.wrap_torch_current()
        layer.scalar_stream = shim.Stream.wrap_torch_current()
        layer.stream.edge_softmax_stable(stable)
        for st in (layer.stream, layer.scalar_stream):
            st.timing(True)
        return layer

    known = {"k1": (1, False), "k1s": (1, True),
             "k8": (8, False), "k8s": (8, True)}
    names = [n for n in args.variants.split(",") if n]
    layers = {n: variant(*known[n]) for n in names}

    f = args.f
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    x = up(rng.uniform(-1, 1, size=(v, f)))
    gy = up(rng.uniform(-1, 1, size=(v, f)))
    scalars = {}
    for heads in sorted({known[n][0] for n in names}):
        # the same scalars for a default variant and its stable twin
        a_src = up(rng.uniform(-1, 1, size=(heads, f // heads)))
        a_dst = up(rng.uniform(-1, 1, size=(heads, f // heads)))
        x3 = x.view(v, heads, f // heads)
        s_src, s_dst = (x3 * a_src).sum(-1), (x3 * a_dst).sum(-1)
        if heads == 1:              # the single-head layer takes [V]
            s_src, s_dst = s_src[:, 0].contiguous(), s_dst[:, 0].contiguous()
        scalars[heads] = (s_src, s_dst)

    def kernel_ns(layer):
        return np.array(
            [layer.stream.kernel_ns(t) + layer.scalar_stream.kernel_ns(t)
             for t in range(len(TAGS))], dtype=np.float64)

    def step(n):
        """One forward + backward: (forward kernel ms, backward kernel ms,
        edge-tag ms of both, wall ms)."""
        layer = layers[n]
        torch.cuda.synchronize()
        k0, t = kernel_ns(layer), time.perf_counter()
        y, saved = layer.forward(x, *scalars[known[n][0]])
        torch.cuda.synchronize()
        k1 = kernel_ns(layer)
        layer.backward(gy, saved)
        del y, saved
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        k2 = kernel_ns(layer)
        assert layer.stream.edge_softmax_stable_last() == int(known[n][1])
        return np.array([(k1 - k0).sum() / 1e6, (k2 - k1).sum() / 1e6,
                         (k2 - k0)[EDGE] / 1e6, wall])

    for _ in range(args.warmup):
        for n in names:
            step(n)
    log("warm-up done")

    rounds = []
    for _ in range(args.rounds):
        acc = {n: np.zeros(4) for n in names}
        for _ in range(args.steps):
            for n in names:
                acc[n] += step(n)
        rounds.append({n: acc[n] / args.steps for n in names})

    cols = ("forward_ms", "backward_ms", "edge_tag_ms", "wall_ms")

    def report(n):
        per = np.array([r[n] for r in rounds])          # rounds x 4
        mean = per.mean(axis=0)
        out = {"heads": known[n][0], "stable": known[n][1]}
        for i, c in enumerate(cols):
            out[c] = round(float(mean[i]), 3)
            out[c + "_rounds"] = [round(float(p), 3) for p in per[:, i]]
            out[c + "_spread"] = round(
                float((per[:, i].max() - per[:, i].min()) / mean[i]), 4)
        return out

    out = {"tool": "bench_gat_stable", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {n: report(n) for n in names}}
    ratios = {}
    for n in names:
        if known[n][1] and n[:-1] in names:
            d = n[:-1]
            ratios[n + "/" + d] = {
                c: {"mean": round(out["variants"][n][c]
                                  / out["variants"][d][c], 4),
                    "rounds": [round(float(r[n][i] / r[d][i]), 4)
                               for r in rounds]}
                for i, c in enumerate(cols)}
    out["stable_over_default"] = ratios
    print(json.dumps(out), flush=True)
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()


if __name__ == "__main__":
    main()
