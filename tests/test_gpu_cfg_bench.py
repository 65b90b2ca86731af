"""End-to-end: bench.py consumes a reference-format cfg + Gemini edge file
(Cora, written from the committed fixture) and produces a valid JSON line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.conftest import REPO

pytestmark = pytest.mark.gpu


@pytest.mark.timeout(300)
def test_bench_runs_reference_cfg(tmp_path):
    edges = np.load(os.path.join(REPO, "tests", "golden",
                                 "cora.2708.edge.self.npy"))
    edge_path = tmp_path / "cora.2708.edge.self"
    edges.astype(np.uint32).tofile(edge_path)
    cfg = tmp_path / "gcn_cora.cfg"
    cfg.write_text(
        "ALGORITHM:GCN\nVERTICES:2708\nLAYERS:1433-128-7\nEPOCHS:10\n"
        f"EDGE_FILE:{edge_path}\nPROC_CUDA:1\n")
    dump = tmp_path / "dump"
    r = subprocess.run(
        [sys.executable, os.path.join(REPO, "bench.py"), "--cfg", str(cfg),
         "--steps", "3", "--warmup", "1", "--dump-outputs", str(dump)],
        capture_output=True, text=True, timeout=280, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["metric"] == "aggregated_edges_per_sec"
    assert d["value"] > 0
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    assert d["cpu_baseline"] is None  # that leg runs only under --full
    assert d["config"]["V"] == 2708 and d["config"]["feat"] == 1433
    assert d["config"]["E"] == 13566

    # --dump-outputs: the last timed step's y and gx, whole at this size,
    # against the oracle on the bench's seeded inputs
    import oracle
    from neutronstarlite_amd import graph as G
    v, f = 2708, 1433
    outd, ind = G.degrees(edges, v)
    w = G.norm_weights(edges[:, 0], edges[:, 1], outd, ind)
    ch = G.build_chunks(edges, w, np.array([0, v], dtype=np.uint32), 0)[0]
    rng = np.random.default_rng(42)
    x = rng.uniform(-1, 1, size=(v, f)).astype(np.float32)
    gy = rng.uniform(-1, 1, size=(v, f)).astype(np.float32)
    refs = {
        "y": oracle.csc_forward(ch.column_offset, ch.row_indices,
                                ch.edge_weight_forward, x, 0, v, f),
        "gx": oracle.csr_backward(ch.row_offset, ch.column_indices,
                                  ch.edge_weight_backward, gy, 0, v, f),
    }
    assert sorted(os.listdir(dump)) == ["gx.npy", "y.npy"]
    for name, ref in refs.items():
        got = np.load(dump / (name + ".npy"))
        assert got.dtype == np.float32 and got.shape == (v, f)
        err = np.abs(got - ref)
        assert (err <= 1e-4 * np.abs(ref) + 1e-5).all(), name
