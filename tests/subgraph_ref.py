"""Plain NumPy restatement of the induced subgraph and the random walk (pygat_amd/subgraph.py, csrc/k23_subgraph.hip): no torch, no GPU.

    induced_subgraph_ref  only the SET of `nodes` counts.  Local ids are ranks in ascending global id: nodes_out = the distinct ids
                          ascending, index[i] = the rank of nodes[i].  Row r holds, in ascending position, the positions p of graph
                          row nodes_out[r] whose col[p] is in the set; its local column is the rank of col[p]; edge_ids = those
                          positions (strictly increasing over the whole sub-pattern).
    random_walk_ref       walks[w, 0] = start[w]; for t = 1 .. length, with cur = walks[w, t - 1], [b, e) its row and d = e - b:
                          k = word (t & 3) of Philox-4x32-10 with counter (w, hop, STREAM_WALK, t >> 2) and key (seed & 0xFFFFFFFF,
                          seed >> 32); walks[w, t] = col[b + ((k * d) >> 32)]; a walker on a row without entries stays.

tests/test_gpu_subgraph.py compares the kernels with this integer for integer; a change of the layout changes this file in the same
commit.
"""
from collections import namedtuple

import numpy as np

from philox_ref import philox4x32_10, _key

STREAM_WALK = 5

Sub = namedtuple("Sub", "rowptr col edge_rc edge_ids nodes index n nnz n_empty_rows")


def induced_subgraph_ref(rowptr, col, nodes):
    rowptr, col, nodes = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(nodes, dtype=np.int64)
    N = rowptr.size - 1
    if nodes.ndim != 1 or nodes.size < 1 or nodes.min() < 0 or nodes.max() >= N:
        raise ValueError("induced_subgraph_ref: nodes must hold node ids of the graph")
    out_nodes = np.unique(nodes)                                    # ascending, distinct
    rank = np.full(N, -1, dtype=np.int64)
    rank[out_nodes] = np.arange(out_nodes.size)
    sub_rowptr, cols, ids = [0], [], []
    for i in out_nodes:
        p = np.arange(rowptr[i], rowptr[i + 1], dtype=np.int64)
        p = p[rank[col[p]] >= 0]
        ids.append(p)
        cols.append(rank[col[p]])
        sub_rowptr.append(sub_rowptr[-1] + p.size)
    sub_rowptr = np.asarray(sub_rowptr, dtype=np.int64)
    sub_col, edge_ids = np.concatenate(cols), np.concatenate(ids)
    row_of = np.repeat(np.arange(out_nodes.size, dtype=np.int64), np.diff(sub_rowptr))
    return Sub(sub_rowptr, sub_col, np.stack([row_of, sub_col], 1), edge_ids, out_nodes, rank[nodes], int(out_nodes.size),
               int(edge_ids.size), int((np.diff(sub_rowptr) == 0).sum()))


def step_keys(seed, hop, n_walk, t):
    """uint32 [n_walk]: the key of step t of every walker."""
    w = np.arange(n_walk, dtype=np.uint64)
    ctr = np.stack([w, np.full_like(w, int(hop)), np.full_like(w, STREAM_WALK), np.full_like(w, int(t) >> 2)], axis=-1)
    return philox4x32_10(ctr, _key(seed))[:, int(t) & 3]


def random_walk_ref(rowptr, col, start, length, seed, hop=0):
    rowptr, col, start = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(start, dtype=np.int64)
    N = rowptr.size - 1
    if start.ndim != 1 or start.size < 1 or start.min() < 0 or start.max() >= N or length < 1:
        raise ValueError("random_walk_ref: start must hold node ids of the graph, length >= 1")
    walks = np.empty((start.size, length + 1), dtype=np.int64)
    walks[:, 0] = cur = start
    for t in range(1, length + 1):
        k = step_keys(seed, hop, start.size, t).astype(np.uint64)
        b, d = rowptr[cur], rowptr[cur + 1] - rowptr[cur]
        pick = b + ((k * d.astype(np.uint64)) >> np.uint64(32)).astype(np.int64)          # k * d < 2^63: no overflow in uint64
        cur = np.where(d > 0, col[np.minimum(pick, col.size - 1)], cur)
        walks[:, t] = cur
    return walks
