"""bench.py --dump-outputs: what the last timed step computed, written as float32 .npy files.  The inputs are seeded, so the
stream-launched level, its HIP-graph replay and the head-parallel run over two ranks (out of the internal node order, gathered
from both ranks) must dump the same output and gradients."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ["--scale", "12", "--draws", "20000", "--steps", "3", "--warmup", "1", "--no-cpu", "--no-epoch", "--no-v2", "--no-alt"]


def _bench(out_dir, extra, env_extra=None):
    env = dict(os.environ, **(env_extra or {}))
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + SMALL + ["--dump-outputs", str(out_dir)] + extra,
                       capture_output=True, text=True, env=env, timeout=420)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout[-2000:]
    line = json.loads(lines[0])
    assert line["steps"] == 3 and line["ms_per_step"] > 0
    files = sorted(os.listdir(out_dir))
    assert files == sorted(f"{n}.npy" for n in line["dump_outputs"]["arrays"])
    assert sum(os.path.getsize(os.path.join(out_dir, f)) for f in files) <= 64 << 20
    got = {f[:-4]: np.load(os.path.join(out_dir, f), allow_pickle=False) for f in files}
    for name, v in got.items():
        assert v.dtype == np.float32 and list(v.shape) == line["dump_outputs"]["arrays"][name], name
        assert np.isfinite(v).all(), name
    return line, got


def _close(p, q, what, tol=5e-5):
    assert p.shape == q.shape, what
    assert float(np.abs(p - q).max()) <= tol * max(1.0, float(np.abs(p).max())), what


def test_bench_dump_outputs(tmp_path):
    line, a = _bench(tmp_path / "eager", [])
    N, Fin, H, Fo = (line["config"][k] for k in ("nodes", "fin", "heads", "f_out"))
    assert line["dump_outputs"]["rows"] == "all"
    assert sorted(a) == ["dW", "da", "out"]
    assert a["out"].shape == (N, H * Fo) and a["dW"].shape == (H, Fin, Fo) and a["da"].shape == (H, 2 * Fo)
    assert np.abs(a["dW"]).max() > 0 and np.abs(a["da"]).max() > 0

    _, b = _bench(tmp_path / "graphed", ["--hip-graph", "--dx"])       # same seeded inputs, replayed from HIP graphs
    assert b["dX"].shape == (N, Fin) and np.abs(b["dX"]).max() > 0
    for name in ("out", "dW", "da"):
        _close(a[name], b[name], f"graphed {name}")

    # two ranks sharing the one card over gloo (RCCL refuses two ranks on a device), 4 heads each: rank 0 dumps the gathered
    # output and the gradients of its own heads
    _, c = _bench(tmp_path / "ranks", ["--gpus", "2"], {"BENCH_BACKEND": "gloo", "HSA_ENABLE_IPC_MODE_LEGACY": "0"})
    _close(a["out"], c["out"], "2 ranks out")
    _close(a["dW"][:H // 2], c["dW"], "2 ranks dW")
    _close(a["da"][:H // 2], c["da"], "2 ranks da")
