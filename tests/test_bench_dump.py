"""bench.py --dump-outputs writer: float32 .npy files, small outputs whole,
large ones cut to the same seeded row sample on every call, 64 MB in all."""
import os

import numpy as np
import torch

import bench


def test_dump_outputs_sampling_and_budget(tmp_path):
    gen = torch.Generator().manual_seed(3)
    big = torch.rand(40_000, 602, generator=gen)          # 96 MB: sampled
    small = torch.rand(7, 5, generator=gen, dtype=torch.float64)
    loss = torch.tensor(1.25)
    named = {"big": big, "small": small, "loss": loss}
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), named)
    bench.dump_outputs(str(b), named)
    assert sorted(os.listdir(a)) == ["big.npy", "loss.npy", "small.npy"]
    total = sum(os.path.getsize(a / fn) for fn in os.listdir(a))
    assert total <= 64 * 1000 * 1000
    got = {k: np.load(a / (k + ".npy")) for k in named}
    assert all(g.dtype == np.float32 for g in got.values())
    assert np.array_equal(got["small"], small.float().numpy())
    assert got["loss"].shape == () and got["loss"] == np.float32(1.25)
    # the sample: distinct rows of `big` in their original order, and the
    # same ones on the second call
    assert got["big"].shape[1] == 602 and 1 < got["big"].shape[0] < 40_000
    assert np.array_equal(got["big"], np.load(b / "big.npy"))
    keys = {r.tobytes(): i for i, r in enumerate(big.numpy())}
    pos = [keys[r.tobytes()] for r in got["big"]]
    assert pos == sorted(set(pos))
