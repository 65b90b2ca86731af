#!/usr/bin/env python
"""DotAttentionLayer.forward against DotAttentionLayer.forward_fused, in one
process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times the two forwards of

    k1, k1s   the single-head layer, default and DotAttentionLayer(stable=True)
    k8, k8s   K=8 heads at the same total width, default and stable

each with float32 rows and (suffix b) with bfloat16 rows, call by call in turn
(k1 forward, k1 fused, k1s forward, k1s fused, ...) after a warm-up of every
variant, so drift of the machine hits all alike.  The baseline of a fused
figure is the forward of the same variant in the same process, never a
recorded number.  Kernel time is the sum of the nts_stream_kernel_ns tags (HIP
events around the launches) of the variant's stream wrapper, reported apart
for NTS_KTAG_EDGE (forward: the edge dot and the two softmax passes; fused:
nothing) and NTS_KTAG_FWD (forward: the heads gather of v; fused: the row pass
and the merge of split destinations).  forward's V-sized scaling of q is a
torch kernel and shows in wall_ms only.  The peak-memory figure is the rise of
torch.cuda.max_memory_allocated() over one call; the fused forward's stream
scratch (the records of shared work items) is the library's own and is
reported beside it as scratch_mb, from the plan entry.  --rounds R repeats the
alternation R times and reports every round and the spread (max - min over
the rounds, relative to their mean).  During the warm-up the two outputs of a
variant are compared (largest difference; the summation orders differ, so
they are not bit-equal).

Byte model per edge: forward 8f + 12 + 28K (the edge dot reads the index and
the k row and writes K scores, the softmax reads and writes them and emits two
orders, the gather reads index, K weights and the v row), fused 8f + 4 (one
index, one k row and one v row): 1260 against 1028 bytes at f=128, K=8 in
float32, 1044 against 1028 at K=1; the fused forward saves the [E, K] traffic
and two index reads, not a row read.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_dot_attention.py --steps 5 --warmup 2
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
FWD, EDGE = TAGS.index("fwd"), TAGS.index("edge")


def log(msg):
    print(f"[bench_dot_attention] {msg}", file=sys.stderr, flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
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
    base = DotAttentionLayer(ch, v, dev)   # topology and slot maps, shared below
    log(f"layer topology built in {time.time() - t0:.1f}s")

    def variant(heads, stable):
        """A layer on base's device topology with its own stream wrapper
        (its own timing tags and its own softmax mode)."""
        layer = copy.copy(base)
        layer.heads = heads
        layer.stable = stable
        layer.stream = shim.Stream.wrap_torch_current()
        layer.scalar_stream = shim.Stream.wrap_torch_current()
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
    q, k, val = (up(rng.uniform(-1, 1, size=(v, f))) for _ in range(3))
    rows = {False: (q, k, val),
            True: tuple(t.to(torch.bfloat16) for t in (q, k, val))}

    def kernel_ns(layer):
        return np.array([layer.stream.kernel_ns(t) for t in range(len(TAGS))],
                        dtype=np.float64)

    def call(n, which, keep=False):
        """One forward or forward_fused call: (edge-tag ms, fwd-tag ms, all
        tags ms, wall ms, peak-memory rise in MB) and, with keep, y."""
        layer = layers[n]
        heads, stable, bf16 = known[n]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        m0 = torch.cuda.max_memory_allocated()
        k0, t = kernel_ns(layer), time.perf_counter()
        if which == "forward":
            y, saved = layer.forward(*rows[bf16])
        else:
            y, saved = layer.forward_fused(*rows[bf16]), None
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        k = kernel_ns(layer) - k0
        rise = (torch.cuda.max_memory_allocated() - m0) / 2 ** 20
        assert layer.stream.edge_softmax_stable_last() == int(stable)
        del saved
        fig = np.array([k[EDGE] / 1e6, k[FWD] / 1e6, k.sum() / 1e6, wall, rise])
        return (fig, y) if keep else fig

    agree = {}
    for i in range(max(1, args.warmup)):
        for n in names:
            _, y_f = call(n, "forward", keep=True)
            _, y_i = call(n, "fused", keep=True)
            if i == 0:
                agree[n] = {
                    "max_abs_diff": float((y_f - y_i).abs().max()),
                    "max_abs": float(y_f.abs().max())}
            del y_f, y_i
    log("warm-up done")

    kinds = ("forward", "fused")
    rounds = []
    for _ in range(args.rounds):
        acc = {(n, k): np.zeros(5) for n in names for k in kinds}
        for _ in range(args.steps):
            for n in names:
                for k in kinds:
                    acc[n, k] += call(n, k)
        rounds.append({key: a / args.steps for key, a in acc.items()})

    cols = ("edge_ms", "fwd_ms", "kernel_ms", "wall_ms", "peak_mb")

    def report(n, k):
        per = np.array([r[n, k] for r in rounds])          # rounds x 5
        mean = per.mean(axis=0)
        out = {}
        for i, c in enumerate(cols):
            out[c] = round(float(mean[i]), 3)
            out[c + "_rounds"] = [round(float(p), 3) for p in per[:, i]]
            out[c + "_spread"] = round(
                float((per[:, i].max() - per[:, i].min()) / mean[i]), 4) \
                if mean[i] else 0.0
        return out

    out = {"tool": "bench_dot_attention", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {}}
    for n in names:
        heads, stable, bf16 = known[n]
        plan = shim.dot_attention_forward_fused_plan(
            f, heads, 2 if bf16 else 4, 256, 256, v, e_total)
        rep = {"heads": heads, "stable": stable, "bf16": bf16,
               "agreement": agree[n], "plan": plan,
               "scratch_mb": round(plan["scratch_bytes"] / 2 ** 20, 1)}
        for k in kinds:
            rep[k] = report(n, k)
        rep["fused_over_forward"] = {
            "kernel_ms": round(rep["fused"]["kernel_ms"]
                               / rep["forward"]["kernel_ms"], 4),
            "kernel_ms_rounds": [
                round(float(r[n, "fused"][2] / r[n, "forward"][2]), 4)
                for r in rounds]}
        out["variants"][n] = rep
    print(json.dumps(out), flush=True)
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()


if __name__ == "__main__":
    main()
