"""Graphs and probes of the tests of the self-loop-only tail (ops.TAIL, ops.TAIL_FUSED; csrc/k12_tail.hip): imported by
tests/test_gpu_tail_fused.py and tests/test_gpu_tail_oracle.py."""
import numpy as np


def _iso_csr(N, iso, seed):
    """A connected part + N * iso nodes with nothing but their self loop, ids shuffled (the R-MAT workload's 55 %)."""
    from oracle import gat_oracle as O
    n0 = int(N * (1 - iso))
    rp0, c0 = O.random_symmetric_csr(n0, 6, seed, hub=(4, min(n0 - 1, 1200)))
    rp0, c0 = np.asarray(rp0, dtype=np.int64), np.asarray(c0, dtype=np.int64)
    relabel = np.random.default_rng(seed + 1).permutation(N)
    rows = np.concatenate([np.repeat(np.arange(n0), np.diff(rp0)), np.arange(n0, N)])
    cols = np.concatenate([c0, np.arange(n0, N)])
    r2, c2 = relabel[rows], relabel[cols]
    o = np.lexsort((c2, r2))
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(r2, minlength=N))]).astype(np.int32)
    return rowptr, c2[o].astype(np.int32)


def _spy(monkeypatch):
    """Count the calls of the fused entry point and of the two tail streams."""
    from pygat_amd import ops
    seen = {"project_tail": 0, "fwd_stream": 0, "bwd_stream": 0}

    class Spy:
        def __init__(self, lib):
            self._lib = lib

        def __getattr__(self, name):
            fn = getattr(self._lib, name)
            key = {"pygat_project_tail_blocked": "project_tail", "pygat_gat_forward_tail": "fwd_stream",
                   "pygat_gat_backward_tail": "bwd_stream"}.get(name)
            if key is None:
                return fn

            def wrapped(*a):
                seen[key] += 1
                return fn(*a)
            return wrapped
    monkeypatch.setattr(ops, "lib", Spy(getattr(ops.lib, "_lib", ops.lib)))
    return seen
