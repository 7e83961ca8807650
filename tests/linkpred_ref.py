"""Plain NumPy restatement of the link-prediction ops (pygat_amd/linkpred.py, csrc/k24_linkpred.hip): no torch, no GPU.

    find_edges_ref        pos[i] = the position p with rowptr[row[i]] <= p < rowptr[row[i] + 1] and col[p] == colq[i], or -1.
    nth_non_neighbour     the forbidden list c_0 < ... < c_{f-1} is `cols` (a row's strictly ascending columns), with u merged in at
                          its sorted place if exclude_self and u is not already a column; the r-th smallest id of [0, N) outside it
                          is r + t*, t* = #{t : c_t - t <= r} (c_t - t is the number of allowed ids below c_t: it does not decrease).
    negative_edges_ref    neg[w, s], flat draw i = w * num_neg + s, u = src[w], m = N - f: -1 if m == 0; otherwise k = word (i & 3)
                          of Philox-4x32-10 with counter (i >> 2, hop, STREAM_NEG, 0) and key (seed & 0xFFFFFFFF, seed >> 32),
                          r = (k * m) >> 32, and the draw is nth_non_neighbour(cols of row u, u, N, r, exclude_self).
    link_batch_ref        the id bookkeeping of link_batch: u, v, seeds, the local ids, the excluded positions, pairs and labels.

tests/test_gpu_linkpred.py compares the kernels with this integer for integer; a change of the layout changes this file in the same
commit.
"""
from collections import namedtuple

import numpy as np

from philox_ref import philox4x32_10, _key

STREAM_NEG = 6

Batch = namedtuple("Batch", "u v neg seeds pos_src pos_dst neg_dst excluded pair_rows pair_cols labels")


def find_edges_ref(rowptr, col, row, colq):
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    row, colq = np.asarray(row, dtype=np.int64), np.asarray(colq, dtype=np.int64)
    N = rowptr.size - 1
    if row.shape != colq.shape or row.ndim != 1 or row.size < 1 or min(row.min(), colq.min()) < 0 or max(row.max(), colq.max()) >= N:
        raise ValueError("find_edges_ref: row and col must hold node ids of the graph, one pair per index")
    pos = np.full(row.size, -1, dtype=np.int64)
    for i, (r, c) in enumerate(zip(row, colq)):
        b, e = rowptr[r], rowptr[r + 1]
        hit = np.nonzero(col[b:e] == c)[0]
        if hit.size:
            pos[i] = b + hit[0]
    return pos


def forbidden(cols, u, exclude_self):
    """The forbidden list of a row: its columns, with u merged in if exclude_self (sorted, distinct)."""
    cols = np.asarray(cols, dtype=np.int64)
    return np.union1d(cols, [u]) if exclude_self else cols


def nth_non_neighbour(cols, u, N, r, exclude_self=True):
    c = forbidden(cols, u, exclude_self)
    if not 0 <= r < N - c.size:
        raise ValueError(f"nth_non_neighbour: r={r} outside [0, {N - c.size})")
    t_star = int(np.count_nonzero(c - np.arange(c.size) <= r))
    return r + t_star


def draw_keys(seed, hop, n_draws):
    """uint32 [n_draws]: the key of every flat draw."""
    q = np.arange((n_draws + 3) // 4, dtype=np.uint64)
    ctr = np.stack([q, np.full_like(q, int(hop)), np.full_like(q, STREAM_NEG), np.zeros_like(q)], axis=-1)
    return philox4x32_10(ctr, _key(seed)).reshape(-1)[:n_draws]


def negative_edges_ref(rowptr, col, src, num_neg, seed, hop=0, exclude_self=True):
    """-> (neg [n_src, num_neg] int64, full): full = some row had no candidate (its draws are -1)."""
    rowptr, col, src = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(src, dtype=np.int64)
    N = rowptr.size - 1
    if src.ndim != 1 or src.size < 1 or src.min() < 0 or src.max() >= N or num_neg < 1:
        raise ValueError("negative_edges_ref: src must hold node ids of the graph, num_neg >= 1")
    keys = draw_keys(seed, hop, src.size * num_neg).reshape(src.size, num_neg)
    neg = np.full((src.size, num_neg), -1, dtype=np.int64)
    full = False
    for w, u in enumerate(src):
        c = forbidden(col[rowptr[u]:rowptr[u + 1]], u, exclude_self)
        m = N - c.size
        if m == 0:
            full = True
            continue
        shifted = c - np.arange(c.size)                                  # non-decreasing
        r = ((keys[w].astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)       # k * m < 2^63: no overflow in uint64
        neg[w] = r + np.searchsorted(shifted, r, side="right")          # t* = #{t : c_t - t <= r}
    return neg, full


def link_batch_ref(rowptr, col, edge_ids, num_neg, seed, exclude="reverse"):
    rowptr, col, edge_ids = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(edge_ids, dtype=np.int64)
    N, B = rowptr.size - 1, edge_ids.size
    if edge_ids.ndim != 1 or B < 1 or edge_ids.min() < 0 or edge_ids.max() >= col.size:
        raise ValueError("link_batch_ref: edge_ids must hold CSR positions of the graph")
    row_of = np.repeat(np.arange(N, dtype=np.int64), np.diff(rowptr))
    u, v = row_of[edge_ids], col[edge_ids]
    neg, full = negative_edges_ref(rowptr, col, u, num_neg, seed, 0, True)
    assert not full
    seeds, inv = np.unique(np.concatenate([u, v, neg.reshape(-1)]), return_inverse=True)
    inv = inv.reshape(-1)
    pos_src, pos_dst, neg_dst = inv[:B], inv[B:2 * B], inv[2 * B:].reshape(B, num_neg)
    if exclude == "none":
        excluded = np.zeros(0, dtype=np.int64)
    elif exclude == "positive":
        excluded = np.unique(edge_ids)
    elif exclude == "reverse":
        rev = find_edges_ref(rowptr, col, v, u)
        excluded = np.unique(np.concatenate([edge_ids, rev[rev >= 0]]))
    else:
        raise ValueError(f"link_batch_ref: exclude = {exclude!r}")
    pair_rows = np.concatenate([pos_src, np.repeat(pos_src, num_neg)])
    pair_cols = np.concatenate([pos_dst, neg_dst.reshape(-1)])
    labels = np.concatenate([np.ones(B, dtype=np.float32), np.zeros(B * num_neg, dtype=np.float32)])
    return Batch(u, v, neg, seeds, pos_src, pos_dst, neg_dst, excluded, pair_rows, pair_cols, labels)
