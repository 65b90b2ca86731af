#!/usr/bin/env python3
"""Benchmark of the MI355X-native NeutronStarLite aggregation hot path.

Driver contract: `python bench.py --gpus N --steps K --warmup W` (N>1 via
torch.distributed.run, one rank per GPU over RCCL).  One "step" = one forward
CSC aggregation + one backward CSR aggregation of the GCN layer over the full
graph (BASELINE.json metric: aggregated edges/sec; 2E edges per step).

Default workload (fits one GPU) = BASELINE config #2: Reddit-scale synthetic
power-law RMAT (a,b,c,d)=(0.57,0.19,0.19,0.05), V=232 965, E=114M (+V self
loops), seed 7, feat=602, fp32, weights = 1/sqrt(outdeg*indeg), features
seeded U(-1,1) (seed 42), random-init-equivalent synthetic data (no datasets
on the box).  config #1 (Cora) is a parity-test case, not a bench line.

A plain run sets up, warms up, times the K steps and prints the result line;
`--dump-outputs DIR` additionally writes what the last timed step returned as
DIR/<name>.npy (float32, a fixed seeded row sample when an output is large).
Everything that needs work beyond the timed steps (today: the cpu_baseline
leg) runs only under `--full`.

Rank 0 prints ONE JSON line, including:
  roofline     — the dominant kernel (forward CSC aggregation): ALGORITHMIC
                 bytes/launch = E*(4f+8) + V*8f (SURVEY.md §8d byte model,
                 stated in DESIGN.md) divided by that kernel's average launch
                 duration measured live with HIP events on the launching
                 stream (via the C-ABI's nts_stream_kernel_ns); peak = 8 TB/s
                 HBM3E.  `traffic` = measured HBM bytes/launch from a separate
                 rocprofv3 --pmc pass (profiles/), injected with
                 --traffic-bytes-per-launch; null when not provided.
  cpu_baseline — the CPU oracle (oracle/oracle.c, kind "port") timed on this
                 box's host cores over a bounded sample of the same workload
                 (~10-30 s of CPU work), rank 0 at N=1 under --full only;
                 null otherwise.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)


def log(msg):
    print(f"[bench] {msg}", file=sys.stderr, flush=True)


def build_workload(args):
    from neutronstarlite_amd import graph as G
    t0 = time.time()
    if args.cfg:
        from neutronstarlite_amd.config import read_cfg
        info = read_cfg(args.cfg)
        path = info.edge_file
        if not os.path.isabs(path):
            path = os.path.join(os.path.dirname(os.path.abspath(args.cfg)),
                                path)
        edges = G.load_gemini_edges(path)
        v = info.vertices
        outd, ind = G.degrees(edges, v)
        w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
        log(f"cfg workload: {args.cfg} V={v} E={len(edges)}")
        return v, edges, w
    if args.graph == "reddit":
        v, e = 232_965, 114_000_000
    elif args.graph == "rmat26":
        v, e = 1 << 26, 1_000_000_000
    elif args.graph == "small":
        v, e = 10_000, 200_000
    else:
        raise SystemExit(f"unknown graph {args.graph}")
    edges = G.rmat_edges(v, e, seed=7)
    if args.relabel == "degree":
        outd_raw = np.bincount(edges[:, 0], minlength=v)
        new_of_old = np.empty(v, dtype=np.uint32)
        new_of_old[np.argsort(-outd_raw, kind="stable")] = np.arange(
            v, dtype=np.uint32)
        edges = new_of_old[edges]
    elif args.relabel == "rcm":
        # bandwidth-minimizing clustering relabel (reverse Cuthill-McKee on
        # the symmetrized adjacency): destinations processed in RCM order
        # read source rows clustered in a narrow band -> better Infinity
        # Cache / L2 reuse of the gathered feature rows (the DESIGN §9.3
        # "needs clustering, not sorting" experiment).
        import scipy.sparse as sp
        from scipy.sparse.csgraph import reverse_cuthill_mckee
        ones = np.ones(len(edges), dtype=np.int8)
        A = sp.csr_matrix((ones, (edges[:, 0], edges[:, 1])), shape=(v, v))
        order = reverse_cuthill_mckee(A, symmetric_mode=False)
        new_of_old = np.empty(v, dtype=np.uint32)
        new_of_old[order] = np.arange(v, dtype=np.uint32)
        edges = new_of_old[edges]
        log(f"rcm relabel done in {time.time()-t0:.1f}s")
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    log(f"graph generated: V={v} E={len(edges)} in {time.time()-t0:.1f}s")
    return v, edges, w


def cpu_baseline_leg(chunks, f, target_sec=15.0):
    """Time the CPU oracle (test-infrastructure restatement of the
    reference's ForwardCPUfuseOp loops) on a bounded sample of the same
    workload. Returns the cpu_baseline JSON object."""
    import oracle
    ch = chunks[0]
    v = ch.dst_n
    rng = np.random.default_rng(42)
    # bounded sample: prefix of destinations covering ~target edge count;
    # calibrate on a small probe first.
    probe_d = max(1, min(v, 2000))
    x = rng.uniform(-1, 1, size=(ch.src_n, f)).astype(np.float32)
    t0 = time.time()
    oracle.csc_forward(ch.column_offset[:probe_d + 1], ch.row_indices,
                       ch.edge_weight_forward, x, ch.src_s, probe_d, f)
    dt = max(time.time() - t0, 1e-3)
    probe_edges = int(ch.column_offset[probe_d])
    eps = probe_edges / dt  # edges/sec estimate
    # Prefer the FULL pass (degree-representative; VERDICT r01 flagged the
    # prefix extrapolation's ~19% spread): take it whenever the estimate
    # fits the time budget, and fall back to a prefix only for workloads
    # whose full pass would not (e.g. RMAT-26's 1B edges).
    total_edges = int(ch.column_offset[v])
    if 2 * total_edges / eps <= 3 * target_sec:
        n_d = v
    else:
        n_d = int(np.searchsorted(ch.column_offset, int(eps * target_sec)))
        n_d = max(probe_d, min(v, n_d))
    e_f = int(ch.column_offset[n_d])
    t0 = time.time()
    oracle.csc_forward(ch.column_offset[:n_d + 1], ch.row_indices,
                       ch.edge_weight_forward, x, ch.src_s, n_d, f)
    t_fwd = time.time() - t0
    # backward leg on a source prefix of similar size
    n_s = int(np.searchsorted(ch.row_offset, e_f))
    n_s = max(1, min(ch.src_n, n_s))
    e_b = int(ch.row_offset[n_s])
    g = rng.uniform(-1, 1, size=(v, f)).astype(np.float32)
    t0 = time.time()
    oracle.csr_backward(ch.row_offset[:n_s + 1], ch.column_indices,
                        ch.edge_weight_backward, g, ch.dst_s, n_s, f)
    t_bwd = time.time() - t0
    value = (e_f + e_b) / (t_fwd + t_bwd)
    what = "FULL pass" if n_d == v else "prefix sample"
    return {
        "value": round(value, 1), "unit": "aggregated_edges_per_sec",
        "cores": oracle.num_threads(), "kind": "port",
        "sample": (f"{what}: fwd {e_f} edges ({n_d} dsts) + bwd {e_b} edges "
                   f"({n_s} srcs) of the f={f} workload, "
                   f"{t_fwd + t_bwd:.1f}s on host cores"),
    }


# names of what one step() of each --model returns, in order
OUTPUT_NAMES = {
    "gcn": ["y", "gx"],
    "gat": ["grad_h", "grad_score_src", "grad_score_dst"],
    "gcn-layer": ["gw", "gx"],
    "gcn-sample": ["h", "g"],
    "gcn-sample-train": ["loss"],
    "gcn-train": ["loss"],
}

DUMP_BYTES = 60_000_000  # all dumped arrays together stay under 64 MB


def dump_outputs(out_dir, named):
    """Write each tensor as out_dir/<name>.npy (float32).  An output whose
    share of DUMP_BYTES is too small for it is reduced to a fixed, seeded,
    sorted sample of its rows — the same rows on every run and build."""
    import torch
    os.makedirs(out_dir, exist_ok=True)
    share = DUMP_BYTES // max(1, len(named))
    for name, t in named.items():
        t = t.detach()
        if t.numel() * 4 > share:
            rows = t.shape[0]
            keep = max(1, share // (4 * (t.numel() // rows)))
            idx = np.sort(np.random.default_rng(0).choice(
                rows, size=min(keep, rows), replace=False))
            t = t[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(out_dir, name + ".npy"),
                t.float().cpu().numpy())


def main(argv=None, _test_engine_factory=None, _test_backend=None,
         _test_device=None):
    """Product entry point: HIP engine, RCCL, cuda devices.  The _test_*
    hooks exist ONLY so tests/test_bench_dist_cpu.py can drive this exact
    orchestration (env parsing, process group, barriers, max-over-ranks
    timing, JSON contract) under gloo on CPU with a test-owned engine; the
    product defaults never touch them."""
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--feat", type=int, default=None,
                    help="feature width (default 602, or LAYERS[0] of --cfg)")
    ap.add_argument("--cfg", default=None,
                    help="reference-format cfg file (InputInfo KEY:VALUE): "
                         "takes VERTICES, LAYERS and EDGE_FILE (Gemini "
                         "binary, resolved relative to the cfg) as the "
                         "workload instead of --graph")
    ap.add_argument("--model", default="gcn",
                    choices=["gcn", "gat", "gcn-layer", "gcn-sample",
                             "gcn-sample-train", "gcn-train"],
                    help="gcn = fused norm-degree aggregation (configs #2-4);"
                         " gat = attention-weighted layer with edge softmax "
                         "(config #5, single GPU, --feat 128); gcn-layer = "
                         "whole GCN layer with the feature-projection GEMM "
                         "ordered BEFORE the aggregation (SURVEY 8f-2: one "
                         "HBM pass at f_out instead of f_in when f_out<<f_in);"
                         " gcn-sample = mini-batch step: GPU-resident "
                         "reservoir sampling + 2-layer sampled aggregation "
                         "(the reference's GCN_CPU_SAMPLE workload, 8f-3);"
                         " gcn-train = full 2-layer GCN training epoch "
                         "(agg+mm+relu+agg+mm+nll fwd/bwd + Adam, the "
                         "ALGORITHM:GCN train loop, GCN.hpp:237-306)")
    ap.add_argument("--batch-size", type=int, default=4096,
                    help="targets per step for --model gcn-sample")
    ap.add_argument("--fanout", default="25,10",
                    help="per-layer fan-outs for --model gcn-sample")
    ap.add_argument("--feat-out", type=int, default=128,
                    help="projection width for --model gcn-layer")
    ap.add_argument("--graph", default="reddit",
                    choices=["reddit", "rmat26", "small"])
    ap.add_argument("--full", action="store_true",
                    help="also run the legs that are not needed for the "
                         "headline figure (the cpu_baseline oracle timing)")
    ap.add_argument("--no-cpu-baseline", action="store_true",
                    help="with --full: skip the cpu_baseline leg")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="after the timed steps, write the arrays the last "
                         "timed step returned as DIR/<name>.npy (float32; a "
                         "fixed seeded row sample of outputs too large to "
                         "keep whole, 64 MB in all at most)")
    ap.add_argument("--cache-dir", default=None,
                    help="cache built graph/chunk arrays (npz) to skip the "
                         "~1 min host-side setup on repeated runs")
    ap.add_argument("--mirror-filtered", action="store_true",
                    help="lock-free exchange: send each peer only the rows "
                         "its chunks reference (the reference's LOCK_FREE "
                         "path; static index lists exchanged at setup)")
    ap.add_argument("--relabel", default="none",
                    choices=["none", "degree", "rcm"],
                    help="preprocessing: renumber vertices by descending "
                         "out-degree so hot source rows are contiguous "
                         "(Infinity-Cache locality); arithmetic unchanged")
    ap.add_argument("--traffic-bytes-per-launch", type=float, default=None,
                    help="measured HBM bytes per forward launch from a "
                         "rocprofv3 --pmc pass (see profiles/)")
    args = ap.parse_args(argv)

    if args.feat is None:
        if args.cfg:
            from neutronstarlite_amd.config import read_cfg
            ls = read_cfg(args.cfg).layer_sizes
            args.feat = ls[0] if ls else 602
        else:
            args.feat = 602

    # roofline.traffic: ONLY a live value passed via --traffic-bytes-per-launch
    # (taken from a rocprofv3 --pmc run of this same command) is reported;
    # the default is null so stale committed-profile constants are never
    # presented as measured traffic.  The committed per-config
    # measurements live in profiles/bench_lines.md.

    import torch
    import torch.distributed as dist
    from neutronstarlite_amd import graph as G, shim
    from neutronstarlite_amd.ops import DeviceChunk, HipEngine
    from neutronstarlite_amd.ring import RingGraph, ring_backward, ring_forward

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    n = max(args.gpus, world)
    distributed = world > 1
    if args.gpus > 1 and world == 1:
        raise SystemExit("--gpus N>1 must be launched via torch.distributed.run")

    if _test_device == "cpu":
        dev = torch.device("cpu")
    else:
        assert torch.cuda.is_available(), "bench needs an MI355X"
        torch.cuda.set_device(local_rank)
        dev = torch.device("cuda", local_rank)
    if distributed:
        dist.init_process_group(_test_backend or "nccl")

    def device_sync():
        if dev.type == "cuda":
            torch.cuda.synchronize()

    f = args.feat
    cache = None
    if args.cache_dir:
        os.makedirs(args.cache_dir, exist_ok=True)
        # key includes the cfg basename so a --cfg workload never collides
        # with a --graph workload in the same cache dir
        cfg_tag = ("cfg_" + os.path.splitext(os.path.basename(args.cfg))[0]
                   if args.cfg else args.graph)
        cache = os.path.join(args.cache_dir,
                             f"g_{cfg_tag}_{args.relabel}_w{world}_r{rank}.npz")
    if cache and os.path.exists(cache):
        t0 = time.time()
        z = np.load(cache)
        v, e_total_cached, offs = int(z["v"]), int(z["e_total"]), z["offs"]
        chunks = []
        for k in range(len(offs) - 1):
            chunks.append(G.Chunk(
                src_s=int(offs[k]), src_e=int(offs[k + 1]),
                dst_s=int(offs[rank]), dst_e=int(offs[rank + 1]),
                column_offset=z[f"co{k}"], row_indices=z[f"ri{k}"],
                edge_weight_forward=z[f"wf{k}"], row_offset=z[f"ro{k}"],
                column_indices=z[f"ci{k}"], edge_weight_backward=z[f"wb{k}"]))
        edges_len = e_total_cached
        log(f"rank {rank}: loaded cached graph in {time.time()-t0:.1f}s")
    else:
        # every rank generates the same seeded graph, so offsets agree
        v, edges, w = build_workload(args)
        if distributed:
            offs = G.partition_offsets(edges, v, world)
        else:
            offs = np.array([0, v], dtype=np.uint32)
        t0 = time.time()
        chunks = G.build_chunks(edges, w, offs, rank)
        edges_len = len(edges)
        log(f"rank {rank}: chunks built in {time.time()-t0:.1f}s")
        if cache:
            arrs = {"v": v, "e_total": edges_len, "offs": offs}
            for k, ch in enumerate(chunks):
                arrs.update({f"co{k}": ch.column_offset, f"ri{k}": ch.row_indices,
                             f"wf{k}": ch.edge_weight_forward,
                             f"ro{k}": ch.row_offset, f"ci{k}": ch.column_indices,
                             f"wb{k}": ch.edge_weight_backward})
            np.savez(cache, **arrs)

    e_total = edges_len
    lo, hi = int(offs[rank]), int(offs[rank + 1])
    if _test_engine_factory is None:
        dchunks = [DeviceChunk(ch, dev) for ch in chunks]
        engine = HipEngine()
    else:
        dchunks = chunks
        engine = _test_engine_factory()
    engine.stream.timing(True)
    if _test_engine_factory is None and not args.model.startswith("gcn-sample"):
        # chunks are static for the full-batch modes -> work-item reuse is
        # safe (sampled subgraphs change every step, so gcn-sample keeps
        # the rebuild-per-call default)
        engine.stream.items_reuse(1)
    rg = RingGraph(offs, rank, dchunks, dev)
    if distributed and args.mirror_filtered:
        from neutronstarlite_amd.ring import setup_mirror_lists
        setup_mirror_lists(rg)

    rng = np.random.default_rng(42 + rank)
    torch.manual_seed(42 + rank)  # gcn-sample draws its inputs on device
    x_np = None
    if args.cfg:
        # use the cfg's FEATURE_FILE when it exists (GNNDatum text format);
        # otherwise fall back to the synthetic convention
        from neutronstarlite_amd.config import read_cfg
        from neutronstarlite_amd import data as D
        info = read_cfg(args.cfg)
        fpath = info.feature_file
        if fpath and not os.path.isabs(fpath):
            fpath = os.path.join(os.path.dirname(os.path.abspath(args.cfg)),
                                 fpath)
        if fpath and os.path.exists(fpath):
            x_np = D.read_feature_table(fpath, lo, hi, f)
            log(f"features from {fpath}")
    if x_np is None:
        x_np = rng.uniform(-1, 1, size=(hi - lo, f)).astype(np.float32)
    x = torch.from_numpy(x_np).to(dev)
    gy = torch.from_numpy(
        rng.uniform(-1, 1, size=(hi - lo, f)).astype(np.float32)).to(dev)

    if args.model == "gcn-train":
        # end-to-end training epoch like GCN_impl::run (toolkits/GCN.hpp:237):
        # layer0 aggregate(f=602) -> W0 -> relu -> layer1 aggregate(128) ->
        # W1 -> log_softmax -> nll; backward through the autograd-bridged
        # aggregation; Adam step.  A "step" here is one full epoch.
        assert not distributed, "training bench is single-GPU here"
        from neutronstarlite_amd.ops import aggregate
        f1, ncls = args.feat_out, 41   # LAYERS 602-128-41 (gcn_reddit.cfg)
        dch = dchunks[0]
        gw = torch.Generator(device="cpu").manual_seed(7)
        W0 = (torch.rand(f, f1, generator=gw) * 0.2 - 0.1).to(dev).requires_grad_(True)
        W1 = (torch.rand(f1, ncls, generator=gw) * 0.2 - 0.1).to(dev).requires_grad_(True)
        labels = torch.randint(ncls, (hi - lo,),
                               generator=gw).to(dev)
        opt = torch.optim.Adam([W0, W1], lr=1e-2)
        # the reference's tape always runs every graph op's backward
        # (ntsContext::self_backward, ntsContext.hpp:276-359) — require grad
        # on the features so layer 0's backward aggregation runs here too
        # and the counted 2x(fwd+bwd) passes are all real
        x_t = x.clone().requires_grad_(True)

        def step():
            opt.zero_grad(set_to_none=True)
            if x_t.grad is not None:
                x_t.grad = None
            a0 = aggregate(x_t, dch, engine)
            h0 = torch.relu(a0 @ W0)
            a1 = aggregate(h0, dch, engine)
            out = torch.log_softmax(a1 @ W1, 1)
            loss = torch.nn.functional.nll_loss(out, labels)
            loss.backward()
            opt.step()
            return loss
    elif args.model in ("gcn-sample", "gcn-sample-train"):
        # mini-batch step: sample a 2-layer subgraph on device
        # (reservoir kernel + torch compaction), then aggregate innermost ->
        # outermost with the same gather kernels.  Value still counts
        # aggregated edges (the sampled edges of both layers, fwd+bwd).
        # gcn-sample-train is the END-TO-END training step:
        # sampled feature gather from the resident feature matrix + 2-layer
        # GCN (agg -> W0 -> relu -> agg -> W1 -> nll) through the autograd
        # bridge + Adam — the reference's GCN_CPU_SAMPLE per-epoch loop
        # (toolkits/GCN_CPU_SAMPLE.hpp:195-260) on GPU-resident sampling.
        assert not distributed, "sampled bench is single-GPU here"
        from neutronstarlite_amd.ops import MiniBatchFuseOp, _u32_cuda
        from neutronstarlite_amd.sampler_gpu import sample_subgraph_gpu
        fanouts = [int(t) for t in args.fanout.split(",") if t]
        ch0 = chunks[0]
        d_coff = _u32_cuda(ch0.column_offset, dev)
        d_rows = _u32_cuda(ch0.row_indices, dev)
        import neutronstarlite_amd.graph as _G
        outd_np, ind_np = _G.degrees(
            np.stack([ch0.row_indices,
                      np.repeat(np.arange(v, dtype=np.uint32),
                                np.diff(ch0.column_offset.astype(np.int64)))],
                     axis=1), v)
        d_outd = torch.from_numpy(outd_np.astype(np.int64)).to(dev)
        d_ind = torch.from_numpy(ind_np.astype(np.int64)).to(dev)
        sampled_edges = [0]
        step_idx = [0]
        gen = np.random.default_rng(42)
        target_pool = gen.permutation(v).astype(np.int32)

        if args.model == "gcn-sample-train":
            from neutronstarlite_amd.ops import minibatch_aggregate
            f1, ncls = args.feat_out, 41  # LAYERS 602-128-41 convention
            gw = torch.Generator().manual_seed(7)
            W0 = ((torch.rand(f, f1, generator=gw) * 0.2 - 0.1)
                  .to(dev).requires_grad_(True))
            W1 = ((torch.rand(f1, ncls, generator=gw) * 0.2 - 0.1)
                  .to(dev).requires_grad_(True))
            opt = torch.optim.Adam([W0, W1], lr=1e-2)
            label_pool = torch.from_numpy(
                gen.integers(0, ncls, v).astype(np.int64)).to(dev)

            def step():
                i = step_idx[0]
                step_idx[0] += 1
                lo_t = (i * args.batch_size) % max(1, v - args.batch_size)
                targets = torch.from_numpy(
                    target_pool[lo_t:lo_t + args.batch_size]).to(dev)
                layers = sample_subgraph_gpu(engine.stream, d_coff, d_rows,
                                             targets, fanouts, d_outd, d_ind,
                                             seed=1000 + i)
                ops_ = [MiniBatchFuseOp(ly, dev, engine) for ly in layers]
                # sampled feature gather from the RESIDENT matrix
                x_s = x.index_select(0, layers[-1].src)
                opt.zero_grad(set_to_none=True)
                h = minibatch_aggregate(x_s, ops_[-1])
                h = torch.relu(h @ W0)
                h = minibatch_aggregate(h, ops_[0])
                out = torch.log_softmax(h @ W1, 1)
                loss = torch.nn.functional.nll_loss(
                    out, label_pool[targets.to(torch.int64)])
                loss.backward()
                opt.step()
                for ly in layers:
                    sampled_edges[0] += 2 * ly.e_size  # fwd + bwd
                return loss
        else:
            def step():
                i = step_idx[0]
                step_idx[0] += 1
                lo_t = (i * args.batch_size) % max(1, v - args.batch_size)
                targets = torch.from_numpy(
                    target_pool[lo_t:lo_t + args.batch_size]).to(dev)
                layers = sample_subgraph_gpu(engine.stream, d_coff, d_rows,
                                             targets, fanouts, d_outd, d_ind,
                                             seed=1000 + i)
                h = torch.randn(layers[-1].n_src, f, device=dev)
                for ly in reversed(layers):
                    op = MiniBatchFuseOp(ly, dev, engine)
                    h = op.forward(h.contiguous())
                    sampled_edges[0] += ly.e_size
                gy = torch.randn(layers[0].n_dst, f, device=dev)
                g = gy
                for ly in layers:
                    op = MiniBatchFuseOp(ly, dev, engine)
                    g = op.backward(g.contiguous())
                    sampled_edges[0] += ly.e_size
                return h, g
    elif args.model == "gcn-layer":
        # the layer's dense projection (x·W, the reference's
        # P[layer]->forward at NtsScheduler.hpp:737-740) ordered BEFORE the
        # aggregation: for 602->128 the gather streams 4.7x fewer bytes.
        # The GEMM itself is rocBLAS via torch.mm (plain library GEMM).
        assert not distributed, "gcn-layer bench is single-GPU here"
        f_out = args.feat_out
        rngw = np.random.default_rng(1)
        W = torch.from_numpy((rngw.uniform(-0.1, 0.1, size=(f, f_out)))
                             .astype(np.float32)).to(dev)
        y_buf = torch.zeros(hi - lo, f_out, device=dev)
        gh_buf = torch.zeros(hi - lo, f_out, device=dev)
        gy_s = torch.from_numpy(
            rng.uniform(-1, 1, size=(hi - lo, f_out)).astype(np.float32)).to(dev)
        dch = dchunks[0]

        def step():
            h = (x @ W).contiguous()
            y_buf.zero_()
            engine.csc_forward(dch, h, y_buf)
            gh_buf.zero_()
            engine.csr_backward(dch, gy_s, gh_buf)
            gw = x.t() @ gh_buf
            gx = gh_buf @ W.t()
            return gw, gx
    elif args.model == "gat":
        # BASELINE config #5: 1-GPU attention-weighted layer; the hot SpMM
        # runs with per-edge softmax weights; edge kernels (a14) feed it.
        assert not distributed, "GAT bench is the single-GPU config (#5)"
        from neutronstarlite_amd.gat import GATLayer
        layer = GATLayer(chunks[0], v, dev)
        a_src = torch.from_numpy(
            rng.uniform(-1, 1, size=f).astype(np.float32)).to(dev)
        a_dst = torch.from_numpy(
            rng.uniform(-1, 1, size=f).astype(np.float32)).to(dev)
        # reuse the engine's timing stream for the roofline numbers
        layer.stream = engine.stream

        def step():
            y, saved = layer.forward(x, x @ a_src, x @ a_dst)
            return layer.backward(gy, saved)
    else:
        def step():
            y = ring_forward(rg, x, engine)
            gx = ring_backward(rg, gy, engine)
            return y, gx

    log(f"rank {rank}/{n}: warmup {args.warmup}")
    for _ in range(args.warmup):
        step()
    device_sync()
    if distributed:
        dist.barrier()
    engine.stream.timing_reset()

    t0 = time.time()
    last = None
    for _ in range(args.steps - 1):
        step()
    if args.steps > 0:
        last = step()  # kept only for --dump-outputs
    device_sync()
    if distributed:
        dist.barrier()
    elapsed = time.time() - t0
    if distributed:
        t = torch.tensor([elapsed], device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    # per-kernel-tag breakdown over the timed region (HIP events)
    tag_names = ["fwd", "bwd", "deser", "aggmsg", "items", "edge"]
    log("kernel ns/step: " + "  ".join(
        f"{nm}={engine.stream.kernel_ns(i) / args.steps / 1e6:.3f}ms"
        f"(x{engine.stream.kernel_launches(i) // max(1, args.steps)})"
        for i, nm in enumerate(tag_names)))

    # roofline for the dominant (forward) kernel, from HIP events on the
    # launching stream; at N=1 there is exactly one fwd launch per step.
    fwd_ns = engine.stream.kernel_ns(shim.KTAG_FWD)
    fwd_launches = engine.stream.kernel_launches(shim.KTAG_FWD)
    local_edges = sum(ch.edge_size for ch in chunks)
    # algorithmic bytes per launch: per edge f floats of source
    # row + u32 index + f32 weight; per output row one read + one write.
    # (for gcn-layer the gather runs at the projected width)
    f_roof = args.feat_out if args.model == "gcn-layer" else f
    edges_per_launch = local_edges / max(1, len(chunks))
    algo_bytes_launch = (edges_per_launch * (4 * f_roof + 8)
                         + (hi - lo) * 8 * f_roof / max(1, len(chunks)))
    avg_launch_ns = fwd_ns / max(1, fwd_launches)
    achieved = algo_bytes_launch / max(avg_launch_ns, 1e-9)  # GB/s
    roofline = {
        "bound": "hbm",
        "achieved": round(achieved, 1),
        "peak": 8000.0,
        "unit": "GB/s",
        "frac": round(achieved / 8000.0, 4),
        "traffic": args.traffic_bytes_per_launch,
    }

    if args.dump_outputs:
        named = dict(zip(OUTPUT_NAMES[args.model],
                         last if isinstance(last, (tuple, list)) else [last]))
        if args.model in ("gcn-train", "gcn-sample-train"):
            named.update(W0=W0, W1=W1)
        if distributed:
            named = {f"{k}.rank{rank}": t for k, t in named.items()}
        dump_outputs(args.dump_outputs, named)
    del last

    cpu_baseline = None
    if args.full and rank == 0 and n == 1 and not args.no_cpu_baseline:
        log("cpu baseline (oracle, bounded sample)")
        cpu_baseline = cpu_baseline_leg(chunks, f)

    if args.model == "gcn-train":
        # one epoch = 2 layers x (fwd + bwd) aggregation
        value = args.steps * 4.0 * e_total / elapsed
    elif args.model.startswith("gcn-sample"):
        # count the edges actually sampled+aggregated during the timed steps
        # (warmup's share removed via the step counter)
        value = sampled_edges[0] * (args.steps /
                                    max(1, step_idx[0])) / elapsed
    else:
        value = args.steps * 2.0 * e_total / elapsed  # fwd+bwd, all ranks
    if rank == 0:
        out = {
            "metric": "aggregated_edges_per_sec",
            "value": round(value, 1),
            "unit": "edges/s",
            "n_gpus": n,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": (
                    (f"cfg {os.path.basename(args.cfg)}: " if args.cfg
                     else f"{args.graph}: RMAT ") + f"V={v} E={e_total} feat={f} "
                    + ("GAT layer (edge softmax + attention-weighted "
                       "aggregation) fwd+bwd (BASELINE config #5)"
                       if args.model == "gat" else
                       f"GCN layer project({f}->{args.feat_out}) then "
                       "aggregate, fwd+bwd (SURVEY 8f-2 fused-layer order)"
                       if args.model == "gcn-layer" else
                       f"2-layer GCN training epoch ({f}-{args.feat_out}-41,"
                       " agg+mm fwd/bwd + Adam; ALGORITHM:GCN loop)"
                       if args.model == "gcn-train" else
                       f"mini-batch GCN: GPU-resident sampling batch="
                       f"{args.batch_size} fanout={args.fanout} + sampled "
                       "aggregation fwd+bwd (SURVEY 8f-3)"
                       if args.model == "gcn-sample" else
                       f"mini-batch GCN TRAINING step: GPU-resident "
                       f"sampling batch={args.batch_size} fanout="
                       f"{args.fanout} + feature gather + 2-layer "
                       f"({f}-{args.feat_out}-41) agg+mm fwd/bwd + Adam "
                       "(GCN_CPU_SAMPLE loop on device)"
                       if args.model == "gcn-sample-train" else
                       "GCN-layer aggregation fwd+bwd"
                       + (" (BASELINE config #2)" if args.graph == "reddit"
                          else ""))),
                "model": args.model, "V": v, "E": e_total, "feat": f,
                "relabel": args.relabel,
                "parallelism": f"graph-partitioned dp{n}",
                "edges_per_step": 2 * e_total,
            },
            "roofline": (None if args.model.startswith("gcn-sample")
                         else roofline),
            "cpu_baseline": cpu_baseline,
        }
        print(json.dumps(out), flush=True)
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
