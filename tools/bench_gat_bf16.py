#!/usr/bin/env python
"""The attention layers and their f-wide entries with fp32 against bf16
feature rows, in one process.

Builds the BASELINE config #5 workload of `bench.py --model gat --feat 128`
with the package's own graph functions (RMAT V=232 965, E=114 M plus
self-loops, seed 7, f=128), then times forward + backward layer steps of

    g1, g8  GATLayer at K=1 (fp32: the fused single-head layer; bf16: the
            heads call chain, the fused gather-dot being fp32 only) and K=8
    v1, v8  GATv2Layer at K=1 and K=8

each with fp32 rows (`g1` ...) and with the same values as bf16 rows
(`g1_bf16` ...): the rows are drawn, rounded to bf16, and the fp32 variants
get them widened, so both read the same numbers.  Steps alternate variant by
variant after a warm-up of every variant, so drift of the machine hits all
alike.  Kernel time is the sum of the nts_stream_kernel_ns tags (HIP events
around the launches) of the variant's stream wrappers; wall time is the whole
step.  --rounds R repeats the alternation R times and reports every round:
the run-to-run spread to judge the differences by.

Then, per K, single entries on the same values, fp32 against bf16, again
alternating call by call, in ms per call:

    gather    nts_gather_by_dst_from_src_heads[_bf16]      one row per edge
    dot       nts_edge_dot_heads[_bf16]                    fp32 row + bf16 row
    score     nts_edge_gatv2_score[_bf16]                  two rows
    bwd_csc   nts_edge_gatv2_backward[_bf16], CSC, with grad_att   two rows
    bwd_csr   nts_edge_gatv2_backward[_bf16], CSR, without it      two rows

with the ratio bf16 / fp32 and the byte model's prediction next to it: per
edge a one-row pass moves a row, K weights or results and an index,
(2f + 4K + 4) / (4f + 4K + 4); the dot keeps its fp32 row per destination and
is counted as a one-row pass; the all-bf16 two-row passes read the own row
once per vertex and the neighbour row once per edge, so the same ratio.

Prints ONE JSON line.  Run it under its own time limit, one GPU process:

    timeout -k 10 800 python tools/bench_gat_bf16.py --steps 5 --warmup 2
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
ENTRIES = ("gather", "dot", "score", "bwd_csc", "bwd_csr")


def log(msg):
    print(f"[bench_gat_bf16] {msg}", file=sys.stderr, flush=True)


def spread(values):
    return round(max(values) - min(values), 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--f", type=int, default=128)
    ap.add_argument("--graph", default="reddit", choices=["reddit", "small"])
    ap.add_argument("--variants", default="g1,g8,v1,v8",
                    help="each runs with fp32 and with bf16 rows")
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

    kinds = [n for n in args.variants.split(",") if n]
    names = [n + sfx for n in kinds for sfx in ("", "_bf16")]
    layers = {n: variant(*KNOWN[n.split("_")[0]]) for n in names}

    f = args.f
    rng = np.random.default_rng(7)
    up = lambda a: torch.from_numpy(a.astype(np.float32)).to(dev)
    # the same values for both: drawn, rounded to bf16, widened for fp32
    x16 = up(rng.uniform(-1, 1, size=(v, f))).to(torch.bfloat16)
    xr16 = up(rng.uniform(-1, 1, size=(v, f))).to(torch.bfloat16)
    x, x_r = x16.float(), xr16.float()
    gy = up(rng.uniform(-1, 1, size=(v, f)))
    inputs = {}
    for n in kinds:
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
            inputs[n + "_bf16"] = (x16, s_src, s_dst)
        else:
            att = up(rng.normal(size=(heads, c_per)) / np.sqrt(c_per))
            inputs[n] = (x, x_r, att)
            inputs[n + "_bf16"] = (x16, xr16, att)

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
        kind, heads = KNOWN[n.split("_")[0]]
        return {"layer": kind, "heads": heads,
                "rows": "bf16" if n.endswith("_bf16") else "fp32",
                "ms_per_step": round(sum(ks) / len(ks), 3),
                "rounds_ms_per_step": [round(k, 3) for k in ks],
                "spread_ms": spread(ks),
                "wall_ms_per_step": round(
                    sum(r[n][1] for r in rounds) / len(rounds), 3),
                "tags_ms_per_step": {t: round(float(m), 3)
                                     for t, m in zip(TAGS, tags) if m}}

    out = {"tool": "bench_gat_bf16", "V": v, "E": e_total, "f": f,
           "steps": args.steps, "warmup": args.warmup, "rounds": args.rounds,
           "variants": {n: report(n) for n in names}}
    out["bf16_over_fp32_step"] = {
        n: round(out["variants"][n + "_bf16"]["ms_per_step"]
                 / out["variants"][n]["ms_per_step"], 4) for n in kinds}
    for layer in layers.values():
        layer.stream.destroy()
        layer.scalar_stream.destroy()

    # ---- single entries on the same values ----
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

        def calls(bf16):
            sfx = "_bf16" if bf16 else ""
            rl, rr = (x16, xr16) if bf16 else (x, x_r)
            ent = lambda name: getattr(st, name + sfx)
            return {
                "gather": lambda: ent("gather_by_dst_from_src_heads")(
                    p(rl), p(y), p(wk), p(c.row_indices), p(c.column_offset),
                    c.src_s, c.src_e, c.dst_s, c.dst_e, E, c.dst_n, f, heads),
                # dst_rows stays fp32 (the layers pass grad_y there)
                "dot": lambda: ent("edge_dot_heads")(
                    p(ek), p(gy), p(rl), p(c.row_indices), p(c.column_offset),
                    c.src_s, c.dst_n, E, f, heads),
                "score": lambda: ent("edge_gatv2_score")(
                    p(ek), p(rr), p(rl), p(att), 0.2, p(c.row_indices),
                    p(c.column_offset), c.src_s, c.dst_n, E, f, heads),
                "bwd_csc": lambda: ent("edge_gatv2_backward")(
                    p(g_r), p(g_att), p(wk), p(rr), p(rl), p(att), 0.2,
                    p(c.column_offset), p(c.row_indices), c.src_s, c.dst_n, E,
                    f, heads),
                "bwd_csr": lambda: ent("edge_gatv2_backward")(
                    p(g_l), None, p(wk), p(rl), p(rr), p(att), 0.2,
                    p(c.row_offset), p(c.column_indices), c.dst_s, c.src_n, E,
                    f, heads)}

        table = {"fp32": calls(False), "bf16": calls(True)}
        tag = {"gather": 0, "dot": 5, "score": 5, "bwd_csc": 5, "bwd_csr": 5}
        order = [(name, rows) for name in ENTRIES for rows in ("fp32", "bf16")]

        def timed(name, rows):
            torch.cuda.synchronize()
            k0 = st.kernel_ns(tag[name])
            table[rows][name]()
            torch.cuda.synchronize()
            return (st.kernel_ns(tag[name]) - k0) / 1e6

        for _ in range(args.warmup):
            for key in order:
                timed(*key)
        per_round = []
        for _ in range(args.rounds):
            acc = {key: 0.0 for key in order}
            for _ in range(args.steps):
                for key in order:
                    acc[key] += timed(*key)
            per_round.append({key: acc[key] / args.steps for key in order})
        model = round((2 * f + 4 * heads + 4) / (4 * f + 4 * heads + 4), 4)
        res = {}
        for name in ENTRIES:
            row = {}
            for rows in ("fp32", "bf16"):
                rs = [r[(name, rows)] for r in per_round]
                row[rows] = {"ms": round(sum(rs) / len(rs), 3),
                             "rounds": [round(t, 3) for t in rs],
                             "spread_ms": spread(rs)}
            row["bf16_over_fp32"] = round(row["bf16"]["ms"] / row["fp32"]["ms"],
                                          4)
            row["byte_model"] = model
            res[name] = row
        out["entries_ms_per_call"][f"K={heads}"] = res
        log(f"entries at K={heads} done")
    st.destroy()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
