#!/usr/bin/env python
"""fp32 against bfloat16 feature rows on the gather SpMM, in one process.

Builds the BASELINE config #2 workload with the package's own graph
functions (RMAT V=232 965, E=114 M plus self-loops, seed 7, f=602), then
times forward + backward gather steps for each variant in turn, step by step
(fp32, bf16, fp32, bf16, ...), so drift of the machine hits both alike.
Kernel time is the FWD + BWD tags of nts_stream_kernel_ns (HIP events around
the gather launches); wall time is the whole step, output zeroing included.

Prints ONE JSON line: ms/step per dtype, their ratio, and the achieved
bytes/s against each dtype's byte model, per step (forward + backward)

    fp32:  2 * (E * (4 f + 8) + V * 8 f)
    bf16:  2 * (E * (2 f + 8) + V * 8 f)

--f 608 repeats the run at the padded width (16-byte rows: the 8-wide bf16
lanes instead of the 2-wide ones of f=602).  --schedule / --window forward a
request to the kernel for both dtypes; --sweep-bf16 "0:-1,1:0,1:64" times
further bf16 requests (schedule:window) in the same alternation, and
--sweep-stage "1:0:0,1:1:128,-1:1:0" further fp32 requests with a row-staging
mode in front (stage:schedule:window; 1 force, -1 never, 0 automatic; the
first two variants run with staging off), and --sweep-stripe
"128:128:0,128:32:0,128:32:8,256:32:0" further staged fp32 PHASE launches with
stripes forced (window:stripe floats:tasks per wave, 0 = the fewest that fit
the grid cap; R = 1 at the headline shape needs NTS_GATHER_BLOCKS=4194304),
after one variant that is the automatic launch with stripes off (-1) and one
that is fully automatic.  --rounds R
repeats the whole alternation R times and reports every round, which is the
run-to-run spread to judge the ratio by.

Run it under its own time limit, one GPU process:

    timeout -k 10 300 python tools/bench_gather_dtype.py --steps 10 --warmup 3
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK_GBPS = 8000.0  # HBM peak the roofline of bench.py is quoted against


def log(msg):
    print(f"[bench_gather_dtype] {msg}", file=sys.stderr, flush=True)


def model_bytes(v, e, f, elem_bytes):
    """Byte model of one step (forward + backward gather)."""
    return 2 * (e * (elem_bytes * f + 8) + v * 8 * f)


def parse_request(text):
    sched, window = text.split(":")
    return int(sched), int(window)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--f", type=int, default=602)
    ap.add_argument("--schedule", type=int, default=0)
    ap.add_argument("--window", type=int, default=0)
    ap.add_argument("--sweep-bf16", default="",
                    help="comma list of schedule:window requests, bf16 only")
    ap.add_argument("--sweep-stage", default="",
                    help="comma list of stage:schedule:window requests, "
                         "fp32 only")
    ap.add_argument("--sweep-stripe", default="",
                    help="comma list of window:stripe:run requests, staged "
                         "fp32 PHASE only")
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    args = ap.parse_args(argv)

    import torch

    from neutronstarlite_amd import graph as G
    from neutronstarlite_amd import shim
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine

    assert torch.cuda.is_available(), "needs an MI355X"
    dev = torch.device("cuda", 0)
    torch.manual_seed(7)

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

    dch = DeviceChunk(ch, dev)
    eng = HipEngine()
    eng.stream.timing(True)
    eng.stream.items_reuse(1)  # the chunk is static, as in bench.py

    f = args.f
    x32 = torch.rand(v, f, device=dev) * 2 - 1
    g32 = torch.rand(v, f, device=dev) * 2 - 1
    inputs = {"fp32": (x32, g32),
              "bf16": (x32.to(torch.bfloat16), g32.to(torch.bfloat16))}
    y = torch.zeros(v, f, device=dev)
    gx = torch.zeros(v, f, device=dev)

    request = (args.schedule, args.window)
    # (dtype, schedule request, staging mode, (stripe floats, tasks per wave));
    # all but the stripe sweep run with stripes off
    off = (-1, 0)
    variants = [("fp32", request, -1, off), ("bf16", request, -1, off)]
    if args.sweep_bf16:
        variants += [("bf16", parse_request(r), -1, off)
                     for r in args.sweep_bf16.split(",")]
    n_bf16 = len(variants)
    if args.sweep_stage:
        for r in args.sweep_stage.split(","):
            stage, req = r.split(":", 1)
            variants.append(("fp32", parse_request(req), int(stage), off))
    n_stage = len(variants)
    if args.sweep_stripe:
        variants.append(("fp32", (0, 0), 0, off))     # the launch without
        variants.append(("fp32", (0, 0), 0, (0, 0)))  # the automatic launch
        for r in args.sweep_stripe.split(","):
            window, stripe, run = (int(x) for x in r.split(":"))
            variants.append(("fp32", (1, window), 1, (stripe, run)))

    def gather_ns():
        return (eng.stream.kernel_ns(shim.KTAG_FWD)
                + eng.stream.kernel_ns(shim.KTAG_BWD))

    def step(dtype, req, stage, stripe):
        """One forward + backward; returns (kernel ms, wall ms, what ran)."""
        x, g = inputs[dtype]
        eng.stream.gather_schedule(*req)
        eng.stream.gather_staging(stage)
        eng.stream.gather_stripes(*stripe)
        torch.cuda.synchronize()
        k0, t = gather_ns(), time.perf_counter()
        y.zero_()
        eng.csc_forward(dch, x, y)
        gx.zero_()
        eng.csr_backward(dch, g, gx)
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t) * 1e3
        ran = (eng.stream.gather_schedule_last()
               + eng.stream.gather_staging_last()[1:]
               + eng.stream.gather_stripes_last())
        return (gather_ns() - k0) / 1e6, wall, ran

    for _ in range(args.warmup):
        for variant in variants:
            step(*variant)

    rounds = []
    for _ in range(args.rounds):
        acc = [[0.0, 0.0, None] for _ in variants]
        for _ in range(args.steps):
            for i, variant in enumerate(variants):
                k, wall, ran = step(*variant)
                acc[i][0] += k
                acc[i][1] += wall
                acc[i][2] = ran
        rounds.append([(k / args.steps, wall / args.steps, ran)
                       for k, wall, ran in acc])

    def report(i):
        dtype, req, stage, stripe = variants[i]
        ks = [r[i][0] for r in rounds]
        walls = [r[i][1] for r in rounds]
        k = sum(ks) / len(ks)
        model = model_bytes(v, e_total, f, 4 if dtype == "fp32" else 2)
        gbps = model / (k * 1e-3) / 1e9
        return {"dtype": dtype, "request": list(req), "stage": stage,
                "stripe": list(stripe),
                # schedule, window, pitch, stripe floats, tasks per wave
                "ran": list(rounds[-1][i][2]),
                "ms_per_step": round(k, 3),
                "wall_ms_per_step": round(sum(walls) / len(walls), 3),
                "rounds_ms_per_step": [round(x, 3) for x in ks],
                "model_bytes_per_step": model,
                "achieved_GBps": round(gbps, 1),
                "model_frac_of_peak": round(gbps / PEAK_GBPS, 4)}

    fp32, bf16 = report(0), report(1)
    out = {"tool": "bench_gather_dtype", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "fp32": fp32, "bf16": bf16,
           "ratio_bf16_over_fp32": round(
               bf16["ms_per_step"] / fp32["ms_per_step"], 4),
           "rounds_ratio": [round(r[1][0] / r[0][0], 4) for r in rounds],
           "model_ratio": round(bf16["model_bytes_per_step"]
                                / fp32["model_bytes_per_step"], 4),
           "sweep_bf16": [report(i) for i in range(2, n_bf16)],
           "sweep_stage": [report(i) for i in range(n_bf16, n_stage)],
           "sweep_stripe": [report(i) for i in range(n_stage, len(variants))]}
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
