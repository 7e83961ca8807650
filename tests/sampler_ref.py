"""Plain NumPy restatement of the neighbour sampler (pygat_amd/sampling.py, csrc/k22_sample.hip): no torch, no GPU.

    key(p, hop)  of the entry at position p of the graph's CSR = word (p & 3) of Philox-4x32-10 with counter
                 (p >> 2, hop, STREAM_SAMPLE, 0) and key (seed & 0xFFFFFFFF, seed >> 32): it depends on the position only.
    row r        = node dst[r] with positions [b, e): kept whole if e - b <= fanout, else the `fanout` entries smallest in (key, p);
                 kept entries in ascending p.
    src_nodes    = dst in the caller's order, then every other kept column once in ascending id; the local column of a node is its
                 index in src_nodes.

tests/test_gpu_sample.py compares the kernels with this entry for entry; a change of the layout changes this file in the same commit.
"""
from collections import namedtuple

import numpy as np

from philox_ref import philox4x32_10, _key

STREAM_SAMPLE = 4

Block = namedtuple("Block", "rowptr col edge_rc edge_ids src_nodes dst_nodes n_dst n_src nnz")


def keys(seed, hop, positions):
    """uint32 key of every CSR position in `positions` (any shape)."""
    p = np.asarray(positions, dtype=np.uint64)
    q = p >> np.uint64(2)
    ctr = np.stack([q, np.full_like(q, int(hop)), np.full_like(q, STREAM_SAMPLE), np.zeros_like(q)], axis=-1)
    w = philox4x32_10(ctr, _key(seed))
    return np.take_along_axis(w, (p & np.uint64(3)).astype(np.int64)[..., None], axis=-1)[..., 0]


def kept_positions(b, e, fanout, seed, hop):
    """The positions of [b, e) a row keeps, ascending."""
    p = np.arange(b, e, dtype=np.int64)
    if fanout is None or e - b <= fanout:
        return p
    k = keys(seed, hop, p)
    order = np.lexsort((p, k))              # by key, equal keys by position
    return np.sort(p[order[:fanout]])


def sample_neighbors_ref(rowptr, col, dst, fanout, seed, hop=0):
    rowptr, col, dst = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    n = rowptr.size - 1
    if dst.ndim != 1 or dst.size < 1 or dst.min() < 0 or dst.max() >= n or np.unique(dst).size != dst.size:
        raise ValueError("sample_neighbors_ref: dst must hold distinct node ids")
    rows = [kept_positions(rowptr[i], rowptr[i + 1], fanout, seed, hop) for i in dst]
    blk_rowptr = np.zeros(dst.size + 1, dtype=np.int64)
    blk_rowptr[1:] = np.cumsum([r.size for r in rows])
    edge_ids = np.concatenate(rows) if rows else np.zeros(0, dtype=np.int64)
    gcol = col[edge_ids]
    others = np.setdiff1d(gcol, dst)                                  # sorted, unique
    src_nodes = np.concatenate([dst, others])
    local = np.full(n, -1, dtype=np.int64)
    local[src_nodes] = np.arange(src_nodes.size)
    lcol = local[gcol]
    row_of = np.repeat(np.arange(dst.size, dtype=np.int64), np.diff(blk_rowptr))
    return Block(blk_rowptr, lcol, np.stack([row_of, lcol], 1), edge_ids, src_nodes, dst, int(dst.size), int(src_nodes.size),
                 int(edge_ids.size))


def sample_blocks_ref(rowptr, col, seeds, fanouts, seed):
    """Outermost hop first, as pygat_amd.sample_blocks returns them."""
    blocks, dst = [], np.asarray(seeds, dtype=np.int64)
    for t in range(len(fanouts)):
        blocks.append(sample_neighbors_ref(rowptr, col, dst, fanouts[-1 - t], seed, hop=t))
        dst = blocks[-1].src_nodes
    return blocks[::-1]
