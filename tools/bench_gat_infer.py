#!/usr/bin/env python
"""GATLayer.forward against GATLayer.infer, in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times the two forwards of

    k1, k1s   the single-head layer, default and GATLayer(stable=True)
    k8, k8s   K=8 heads at the same total width, default and stable

each with float32 rows and (suffix b) with bfloat16 rows, call by call in turn
(k1 forward, k1 infer, k1s forward, k1s infer, ...) after a warm-up of every
variant, so drift of the machine hits all alike.  The baseline of an infer
figure is the forward of the same variant in the same process, never a
recorded number.  Kernel time is the sum of the nts_stream_kernel_ns tags (HIP
events around the launches) of the variant's stream wrapper, reported apart
for NTS_KTAG_EDGE (forward: score pass + normalize pass; infer: the
denominator pass) and NTS_KTAG_FWD (forward: the heads gather; infer: the
gather that computes its weights).  The peak-memory figure is the rise of
torch.cuda.max_memory_allocated() over one call (the stream's V*K-sized
scratch is the library's own and is the same for both).  --rounds R repeats the
alternation R times and reports every round and the spread (max - min over
the rounds, relative to their mean).  During the warm-up the two outputs of a
variant are compared: bit-equal on destinations of at most NTS_SPLIT edges.

Byte model per edge: forward 4f + 12 + 24K (pass 1 reads the index and writes
m_sum and the stash, pass 2 reads the stash and writes the softmax twice, the
gather reads index, K weights and the row), infer 4f + 8 (two index reads and
the row; the scalars are V*K-sized): 716 against 520 bytes at f=128, K=8 in
float32.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_gat_infer.py --steps 5 --warmup 2
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
SPLIT = 256


def log(msg):
    print(f"[bench_gat_infer] {msg}", file=sys.stderr, flush=True)


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
    unsplit = torch.from_numpy(
        np.diff(ch.column_offset.astype(np.int64)) <= SPLIT).to(dev)

    def variant(heads, stable):
        """A layer on base's device topology with its own stream wrapper
        (its own timing tags and its own softmax mode)."""
        layer = copy.copy(base)
        layer.heads = heads
        layer._heads_path = heads > 1
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
    x = up(rng.uniform(-1, 1, size=(v, f)))
    rows = {False: x, True: x.to(torch.bfloat16)}
    scalars = {}
    for heads in sorted({known[n][0] for n in names}):
        # the same scalars for every variant of a head count
        a_src = up(rng.uniform(-1, 1, size=(heads, f // heads)))
        a_dst = up(rng.uniform(-1, 1, size=(heads, f // heads)))
        x3 = x.view(v, heads, f // heads)
        s_src, s_dst = (x3 * a_src).sum(-1), (x3 * a_dst).sum(-1)
        if heads == 1:              # the single-head layer takes [V]
            s_src, s_dst = s_src[:, 0].contiguous(), s_dst[:, 0].contiguous()
        scalars[heads] = (s_src, s_dst)

    def kernel_ns(layer):
        return np.array([layer.stream.kernel_ns(t) for t in range(len(TAGS))],
                        dtype=np.float64)

    def call(n, which, keep=False):
        """One forward or infer call: (edge-tag ms, fwd-tag ms, all tags ms,
        wall ms, peak-memory rise in MB) and, with keep, y."""
        layer = layers[n]
        heads, stable, bf16 = known[n]
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        m0 = torch.cuda.max_memory_allocated()
        k0, t = kernel_ns(layer), time.perf_counter()
        if which == "forward":
            y, saved = layer.forward(rows[bf16], *scalars[heads])
        else:
            y, saved = layer.infer(rows[bf16], *scalars[heads]), None
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
            _, y_i = call(n, "infer", keep=True)
            if i == 0:
                same = torch.equal(y_f[unsplit].view(torch.int32),
                                   y_i[unsplit].view(torch.int32))
                agree[n] = {
                    "unsplit_bit_equal": bool(same),
                    "max_abs_diff": float((y_f - y_i).abs().max()),
                    "max_abs": float(y_f.abs().max())}
            del y_f, y_i
    log("warm-up done")

    kinds = ("forward", "infer")
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

    out = {"tool": "bench_gat_infer", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {}}
    for n in names:
        heads, stable, bf16 = known[n]
        rep = {"heads": heads, "stable": stable, "bf16": bf16,
               "agreement": agree[n]}
        for k in kinds:
            rep[k] = report(n, k)
        rep["infer_over_forward"] = {
            "kernel_ms": round(rep["infer"]["kernel_ms"]
                               / rep["forward"]["kernel_ms"], 4),
            "kernel_ms_rounds": [
                round(float(r[n, "infer"][2] / r[n, "forward"][2]), 4)
                for r in rounds]}
        out["variants"][n] = rep
    print(json.dumps(out), flush=True)
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()


if __name__ == "__main__":
    main()
