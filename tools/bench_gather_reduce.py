#!/usr/bin/env python
"""Max neighbour aggregation against the unweighted sum gather, in one process.

Builds the headline graph of `bench.py` with the package's own graph
functions (RMAT V=232 965, E=114 M plus self-loops, seed 7; BASELINE config
#5 runs on the same graph) and times, at f=602 (headline) and f=128 (config
#5), forward + backward of

    sum         csc_forward + csr_backward with with_weight=0, automatic
                column schedule (what a user of the sum gets)
    sum_native  the same under the request (0, -1): the native item-order
                launch, which is the only launch the max gather has
    max         csc_reduce + reduce_backward (arg-recording gather, scatter)

step by step in turn (sum, sum_native, max, sum, ...) after a warm-up of every
variant, so drift of the machine hits all alike.  Kernel time is read from the
stream's NTS_KTAG_FWD / NTS_KTAG_BWD tags (HIP events around the launches);
every variant has its own stream wrapper.  --rounds R repeats the alternation
R times and reports every round: the run-to-run spread to judge a ratio by.

Byte model printed beside the times (E edges, V vertices, f columns):
    sum fwd, sum bwd   E * (4f + 4) + V * 8f     row + index per edge; the
                                                 += output is read and written
    max fwd            E * (4f + 4) + V * 8f     the two written rows (value,
                                                 arg) replace that read + write
    max bwd            12 * V * f  (+ V * f fp32 atomics)
The hub merge of the max forward adds 8 bytes of 64-bit atomic per (work item
of a split vertex, column) and two passes over the split vertices' key rows.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 900 python tools/bench_gather_reduce.py --steps 5 --warmup 2
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

VARIANTS = ("sum", "sum_native", "max")


def log(msg):
    print(f"[bench_gather_reduce] {msg}", file=sys.stderr, flush=True)


def model_bytes(variant, e, v, f):
    """(forward, backward) bytes of one step (see the module docstring)."""
    gather = e * (4 * f + 4) + v * 8 * f
    return (gather, 12 * v * f) if variant == "max" else (gather, gather)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--widths", default="602,128")
    ap.add_argument("--op", default="max", choices=["max", "min"])
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    args = ap.parse_args(argv)

    import torch

    from neutronstarlite_amd import graph as G
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine

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
    dch = DeviceChunk(ch, dev)
    split = int((np.diff(ch.column_offset.astype(np.int64)) > 256).sum())
    log(f"graph V={v} E={e_total} ({split} destinations above 256 in-edges) "
        f"built in {time.time() - t0:.1f}s")

    engines = {n: HipEngine() for n in VARIANTS}
    for eng in engines.values():
        eng.stream.timing(True)
    engines["sum_native"].stream.gather_schedule(0, -1)

    def step(n, x, gy, bufs):
        """One forward + backward; returns (fwd ms, bwd ms) of kernel time."""
        eng = engines[n]
        st = eng.stream
        k0 = (st.kernel_ns(shim.KTAG_FWD), st.kernel_ns(shim.KTAG_BWD))
        y, arg, gx = bufs
        gx.zero_()
        if n == "max":
            eng.csc_reduce(dch, x, y, arg, args.op)
            eng.reduce_backward(dch, gy, arg, gx)
        else:
            y.zero_()
            eng.csc_forward(dch, x, y, with_weight=False)
            eng.csr_backward(dch, gy, gx, with_weight=False)
        torch.cuda.synchronize()
        return ((st.kernel_ns(shim.KTAG_FWD) - k0[0]) / 1e6,
                (st.kernel_ns(shim.KTAG_BWD) - k0[1]) / 1e6)

    out = {"tool": "bench_gather_reduce", "V": v, "E": e_total, "op": args.op,
           "split_destinations": split, "steps": args.steps,
           "warmup": args.warmup, "rounds": args.rounds, "widths": {}}
    for f in [int(s) for s in args.widths.split(",") if s]:
        gen = torch.Generator(device=dev).manual_seed(7 + f)
        x = torch.rand(v, f, device=dev, generator=gen) * 2 - 1
        gy = torch.rand(v, f, device=dev, generator=gen) * 2 - 1
        bufs = (torch.empty(v, f, device=dev),
                torch.empty(v, f, dtype=torch.int32, device=dev),
                torch.empty(v, f, device=dev))
        for _ in range(args.warmup):
            for n in VARIANTS:
                step(n, x, gy, bufs)
        ran = {n: engines[n].stream.gather_schedule_last() for n in VARIANTS}
        log(f"f={f}: warm-up done")
        rounds = []
        for _ in range(args.rounds):
            acc = {n: np.zeros(2) for n in VARIANTS}
            for _ in range(args.steps):
                for n in VARIANTS:
                    acc[n] += step(n, x, gy, bufs)
            rounds.append({n: acc[n] / args.steps for n in VARIANTS})
        plan = shim.reduce_plan(f, 16, v, e_total, args.op)
        rep = {"reduce_plan": plan, "variants": {}}
        for n in VARIANTS:
            fwd = [float(r[n][0]) for r in rounds]
            bwd = [float(r[n][1]) for r in rounds]
            mb = model_bytes(n, e_total, v, f)
            rep["variants"][n] = {
                "schedule_ran": list(ran[n]),
                "fwd_ms": round(sum(fwd) / len(fwd), 3),
                "bwd_ms": round(sum(bwd) / len(bwd), 3),
                "rounds_fwd_ms": [round(t, 3) for t in fwd],
                "rounds_bwd_ms": [round(t, 3) for t in bwd],
                "model_bytes_fwd": mb[0], "model_bytes_bwd": mb[1],
                "model_gbps_fwd": round(mb[0] / (sum(fwd) / len(fwd)) / 1e6, 1),
                "model_gbps_bwd": round(mb[1] / (sum(bwd) / len(bwd)) / 1e6, 1),
            }
        for base in ("sum", "sum_native"):
            rep[f"max_fwd_over_{base}_fwd"] = {
                "mean": round(rep["variants"]["max"]["fwd_ms"]
                              / rep["variants"][base]["fwd_ms"], 4),
                "rounds": [round(float(r["max"][0] / r[base][0]), 4)
                           for r in rounds]}
        out["widths"][str(f)] = rep
        del x, gy, bufs
    print(json.dumps(out), flush=True)
    for eng in engines.values():
        eng.stream.destroy()


if __name__ == "__main__":
    main()
