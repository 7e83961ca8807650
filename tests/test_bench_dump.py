"""bench.dump_outputs (bench.py --dump-outputs) on host tensors: whole arrays while they fit, else the same fixed, seeded sample
of rows for every row-indexed output -- the files never pass the budget, and two dumps pick the same rows."""
import os

import numpy as np
import torch

import bench


def _dump(path, N):
    g = torch.Generator().manual_seed(0)
    out = torch.randn(N, 24, generator=g, dtype=torch.float64)
    dX = torch.randn(N, 8, generator=g)
    whole = {"dW": torch.randn(2, 8, 12, generator=g), "da": torch.randn(2, 24, generator=g)}
    by_row = {"out": (24, lambda i: out.index_select(0, i)), "dX": (8, lambda i: dX.index_select(0, i))}
    rec = bench.dump_outputs(str(path), whole, by_row, N, torch.device("cpu"))
    got = {f[:-4]: np.load(os.path.join(path, f), allow_pickle=False) for f in sorted(os.listdir(path))}
    size = sum(os.path.getsize(os.path.join(path, f)) for f in os.listdir(path))
    return rec, got, size, out.float().numpy(), dX.numpy(), whole


def test_dump_whole_arrays(tmp_path):
    rec, got, size, out, dX, whole = _dump(tmp_path, 300)
    assert rec["rows"] == "all" and size <= bench.DUMP_BUDGET
    assert sorted(got) == ["dW", "dX", "da", "out"] and all(v.dtype == np.float32 for v in got.values())
    assert np.array_equal(got["out"], out) and np.array_equal(got["dX"], dX)
    assert np.array_equal(got["dW"], whole["dW"].numpy()) and np.array_equal(got["da"], whole["da"].numpy())


def test_dump_samples_rows_within_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 64 << 10)
    N = 5000
    rec, got, size, out, dX, whole = _dump(tmp_path / "a", N)
    assert size <= 64 << 10
    k = got["out"].shape[0]
    assert 0 < k < N and got["dX"].shape == (k, 8) and rec["rows"].startswith(f"{k} of {N}")
    rows = np.sort(np.random.default_rng(0).choice(N, size=k, replace=False))
    assert np.array_equal(got["out"], out[rows]) and np.array_equal(got["dX"], dX[rows])
    assert np.array_equal(got["dW"], whole["dW"].numpy())
    _, again, _, _, _, _ = _dump(tmp_path / "b", N)
    assert all(np.array_equal(got[n], again[n]) for n in got)
