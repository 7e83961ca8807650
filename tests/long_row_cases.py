"""Patterns for the long-row rule of csrc/long_rows.h: a row of more than 512 entries is summed per 2048-entry
chunk of the entry array into at most 5 partial records per chunk -- slot 0 for the row that runs in from the chunk before, slot
1 + d // 512 for the row that starts at offset d of the chunk -- and its owner adds them in chunk order.  Plain NumPy builders,
(rowptr, col) int32 with sorted rows, shared by tests/test_long_row_cases.py (what the patterns cover, on the CPU) and the GPU tests
of K14, K15 and K17 (test_gpu_attention_grad.py, test_gpu_edge_logit.py, test_gpu_spmm.py)."""
import numpy as np


def nine_hubs():
    """600 nodes; nodes 0..8 are each linked to nodes 0..520, symmetrised, a self loop on every node: 9 888 entries, rows 0..8 of
    521 entries back to back, every other row of at most 10.  Chunk 0 holds slots 1-4 (rows 0-3), chunk 1 all five (row 3 running
    in, rows 4-7), chunk 2 slots 0 and 1.  The pattern is its own transpose, so the column passes see the same."""
    N = 600
    r, c = np.repeat(np.arange(9), 521), np.tile(np.arange(521), 9)
    rr, cc = np.concatenate([r, c, np.arange(N)]), np.concatenate([c, r, np.arange(N)])
    key = np.unique(rr.astype(np.int64) * N + cc)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(key // N, minlength=N))]).astype(np.int32)
    return rowptr, (key % N).astype(np.int32)


def three_chunk_hub():
    """4 500 nodes, node 7 linked to 4 200 others: a row and a column of three 2048-entry chunks."""
    from oracle import gat_oracle as O
    rowptr, col = O.random_symmetric_csr(4500, 4, 9, hub=(7, 4200))
    assert int(np.diff(rowptr).max()) >= 4097
    return rowptr, col
