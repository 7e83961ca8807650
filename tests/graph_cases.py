"""The graphs of tests/test_graph_ref.py (CPU rehearsal of the reference) and tests/test_gpu_graph_structures.py (the GPU
structures against it): built once per process, never modified."""
import functools
import os

import numpy as np

from ladder_case import _ladder_graph

SLOT_EDGES = (4, 8, 32, 64)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _i64(rowptr, col):
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    rowptr.setflags(write=False)
    col.setflags(write=False)
    return rowptr, col


def from_bool(dense):
    """(rowptr, col) of a boolean matrix."""
    dense = np.asarray(dense, dtype=bool)
    return _i64(np.concatenate([[0], np.cumsum(dense.sum(1))]), np.nonzero(dense)[1])


@functools.lru_cache(maxsize=None)
def graph(name):
    from oracle import gat_oracle as O
    if name == "ladder":        # degrees 3 .. 180: chains of 2 .. 45 pieces at 4-edge slots
        return _i64(*_ladder_graph())
    if name == "hub":           # n = 1 mod 4, one row of 702 edges: 176 pieces at 4-edge slots, 89 at 8-edge ones
        return _i64(*O.random_symmetric_csr(1001, 5, 11, hub=(7, 700)))
    if name == "tail":          # 327 rows with only their self loop
        return _i64(*O.random_symmetric_csr(1000, 1.0, 9, hub=(3, 150)))
    if name == "cora":
        z = np.load(os.path.join(GOLDEN, "cora_csr.npz"), allow_pickle=False)
        return _i64(z["rowptr"], z["col"])
    if name == "hub_minus_edge":    # the hub graph without the off-diagonal entry (7, j): asymmetric, no row empty
        rowptr, col = graph("hub")
        k = int(rowptr[7]) + 20
        assert col[k] != 7
        rp = rowptr.copy()
        rp[8:] -= 1
        return _i64(rp, np.delete(col, k))
    if name == "asym65":        # random asymmetric pattern with self loops
        rng = np.random.default_rng(0)
        return from_bool((rng.random((65, 65)) < 0.08) | np.eye(65, dtype=bool))
    if name == "identity64":    # no cut row at any slot length; every row is self-loop-only
        return from_bool(np.eye(64, dtype=bool))
    if name == "shared_slot":   # degree-ordered already; its only degree-1 row (3) shares the last 4-edge slot with row 2
        return _i64([0, 3, 5, 7, 8], [0, 1, 2, 0, 1, 0, 2, 3])
    if name == "pieces32":      # 4-edge slots: row 0 (128 edges) touches exactly 32 slots, row 1 (130 edges) 33 -- the two sides
        n = 140                 # of the `wide` split of the cut list (more than 32 pieces); the other rows hold a self loop
        dense = np.eye(n, dtype=bool)
        dense[0, :128] = True
        dense[1, :130] = True
        return from_bool(dense)
    raise KeyError(name)
