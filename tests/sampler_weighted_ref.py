"""Plain NumPy restatement, in fp64, of the neighbour sampler weighted by edge (pygat_amd.sample_neighbors_weighted,
csrc/k22_sample.hip's WEIGHTED instantiations): no torch, no GPU.

    k(p, hop)    the uint32 Philox word of sampler_ref.keys: the unweighted sampler's key of the entry at CSR position p.
    w = weight[p], one float per entry at its CSR position:
      w == 0               the entry is never sampled;
      w > 0 (+inf too)     its clock is c(p) = E(k) / w, E(k) = -ln(1 - (k + 0.5) / 2^32): a unit exponential variate;
      w < 0 or NaN         ValueError if the row is sampled (rows that no call visits are not looked at).
    row r        = node dst[r]: the `fanout` entries smallest in (c, p) among those with w > 0, all of them if they number at most
                 `fanout` (fanout None: all of them); kept entries in ascending p.  w = +inf gives c = 0: always kept, and of more
                 than `fanout` such entries the first by position.
    src_nodes, local columns, edge_rc: as in sampler_ref.

The kernels compute the clock in fp32, a few ulps (some 2e-7 relative) from this one, and order its bit pattern.  Where a row is cut,
this file also returns the relative gap (c_(f+1) - c_(f)) / c_(f+1) between the last clock kept and the first one dropped: a case
whose gaps are all far above the fp32 error has ONE answer, and the kernels must give it entry for entry (tests/sample_weighted_case.py
asks for 1e-4).  A cut between two clocks that are both exactly 0 (two +inf weights) is decided by position on both sides: its gap
is reported as +inf.
"""
import numpy as np

import sampler_ref as R
from sampler_ref import Block


def clocks(seed, hop, positions, weight):
    """fp64 clock of every CSR position in `positions` (weights > 0 there)."""
    k = R.keys(seed, hop, positions).astype(np.float64)
    E = -np.log1p(-(k + 0.5) / 4294967296.0)
    with np.errstate(divide="ignore"):
        return E / np.asarray(weight, dtype=np.float64)[np.asarray(positions, dtype=np.int64)]


def kept_positions(b, e, fanout, seed, hop, weight):
    """-> (the positions of [b, e) a row keeps, ascending; the relative gap at the cut, NaN for a row that is not cut)."""
    w = np.asarray(weight)[b:e]
    if np.isnan(w).any() or (w < 0).any():
        raise ValueError("sampler_weighted_ref: a negative or NaN weight in a sampled row")
    p = np.arange(b, e, dtype=np.int64)[w > 0]
    if fanout is None or p.size <= fanout:
        return p, np.nan
    c = clocks(seed, hop, p, weight)
    order = np.lexsort((p, c))              # by clock, equal clocks by position
    last, first_out = c[order[fanout - 1]], c[order[fanout]]
    gap = np.inf if first_out == 0 else (first_out - last) / first_out
    return np.sort(p[order[:fanout]]), gap


def sample_neighbors_weighted_ref(rowptr, col, dst, fanout, weight, seed, hop=0):
    """-> (Block, gaps [n_dst]: every row's relative gap at the cut, NaN where the row is kept whole)."""
    rowptr, col, dst = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64), np.asarray(dst, dtype=np.int64)
    n = rowptr.size - 1
    weight = np.asarray(weight)
    if weight.shape != col.shape:
        raise ValueError("sample_neighbors_weighted_ref: one weight per entry expected")
    if dst.ndim != 1 or dst.size < 1 or dst.min() < 0 or dst.max() >= n or np.unique(dst).size != dst.size:
        raise ValueError("sample_neighbors_weighted_ref: dst must hold distinct node ids")
    rows, gaps = zip(*[kept_positions(rowptr[i], rowptr[i + 1], fanout, seed, hop, weight) for i in dst])
    blk_rowptr = np.zeros(dst.size + 1, dtype=np.int64)
    blk_rowptr[1:] = np.cumsum([r.size for r in rows])
    edge_ids = np.concatenate(rows)
    gcol = col[edge_ids]
    others = np.setdiff1d(gcol, dst)                                  # sorted, unique
    src_nodes = np.concatenate([dst, others])
    local = np.full(n, -1, dtype=np.int64)
    local[src_nodes] = np.arange(src_nodes.size)
    lcol = local[gcol]
    row_of = np.repeat(np.arange(dst.size, dtype=np.int64), np.diff(blk_rowptr))
    blk = Block(blk_rowptr, lcol, np.stack([row_of, lcol], 1), edge_ids, src_nodes, dst, int(dst.size), int(src_nodes.size),
                int(edge_ids.size))
    return blk, np.array(gaps, dtype=np.float64)


def sample_blocks_weighted_ref(rowptr, col, seeds, fanouts, weight, seed):
    """Outermost hop first, as pygat_amd.sample_blocks_weighted returns them: -> (blocks, their gaps)."""
    blocks, gaps, dst = [], [], np.asarray(seeds, dtype=np.int64)
    for t in range(len(fanouts)):
        blk, gap = sample_neighbors_weighted_ref(rowptr, col, dst, fanouts[-1 - t], weight, seed, hop=t)
        blocks.append(blk)
        gaps.append(gap)
        dst = blk.src_nodes
    return blocks[::-1], gaps[::-1]

