"""Link-prediction mini-batches on the K24 kernels (csrc/k24_linkpred.hip): where a (row, col) pair stands in the CSR, seeded negative
destinations per source node, and one call that turns a batch of positive edges into sampled blocks that do not leak them, the pair
pattern edge_dot scores and its labels.

    pos = find_edges(g, row, col)                                      # or g.find_edges / g.has_edges / g.reverse_edge_ids()
    neg = negative_edges(g, src, 5, seed=s)                            # [n_src, 5] ids that are no neighbour of src[w]
    batch = link_batch(g, edge_ids, 5, [10, 25], seed=s)               # the positives at CSR positions edge_ids, 5 negatives each
    h = x[batch.blocks[0].src_nodes]
    for blk, layer in zip(batch.blocks, layers):
        h = layer(blk.pattern, h[:blk.n_dst], h)                       # e.g. gatv2_attention; ends with one row per batch.seeds
    loss = F.binary_cross_entropy_with_logits(edge_dot(batch.pairs, h, h), batch.labels)

find_edges (tests/linkpred_ref.py restates all three in NumPy; the kernels agree with it integer for integer): pos[i] is the position
p of graph.fwd.col with rowptr[row[i]] <= p < rowptr[row[i] + 1] and col[p] == col[i], or -1 if the pair is no entry -- the positions
SampledBlock.edge_ids and InducedSubgraph.edge_ids hold.  One thread per pair, a binary search over the row.

negative_edges: neg [n_src, num_neg] int64.  For the flat draw i = w * num_neg + s, with u = src[w]: the forbidden list c_0 < ... <
c_{f-1} is the columns of row u, with u merged in at its sorted place if exclude_self and u is not already a column; m = N - f ids are
left.  The key k is word (i & 3) of Philox-4x32-10 with counter (i >> 2, hop, STREAM_NEG, 0) and key (seed & 0xFFFFFFFF, seed >> 32);
r = (k * m) >> 32; t* = #{t : c_t - t <= r}; the draw is r + t*, the r-th smallest id outside the list (c_t - t does not decrease, so
t* is one binary search: no rejection loop, the same work at any density).  A row without a candidate (m == 0) draws -1.  Uniform over
the non-neighbours up to m / 2^32; the draws of a row are independent, so ids may repeat; the same (seed, hop) gives the same bits.

Host interaction: find_edges and negative_edges make ONE read per call (their flags: one and two int32), link_batch the reads its
docstring lists.  Because of those reads all three are refused during stream capture.  There is no CPU path and no torch fallback.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from ._lib import lib, check
from ._minibatch import _at_least_one, _draw_seed, _graph, _hop, _ids, _no_capture, _seed, _stream, graph_head
from .dropout import STREAM_NEG    # noqa: F401  (the Philox stream of the draw keys; the kernels hold the same constant, csrc/rng.h)
from .graph import CSRGraph
from .sampling import SampledBlock, _fanouts, _weight, sample_blocks_weighted
from .spmm import EdgePattern


class LinkBatch(NamedTuple):
    """One link-prediction mini-batch (link_batch).  blocks: the sampled blocks around `seeds`, outermost hop first, the positive
    edges left out as `exclude` says.  seeds [n_seeds] int64: the distinct ids of every endpoint, ascending; local ids are ranks in
    it.  pos_src, pos_dst [B], neg_dst [B, num_neg]: int64 local ids (seeds[pos_src] are the positives' rows, and so on).  pairs: an
    EdgePattern (n_seeds, n_seeds) whose first B entries are (pos_src, pos_dst), then the B * num_neg entries (pos_src[b],
    neg_dst[b, s]) row-major: edge_dot(pairs, h, h) scores them in that order.  labels: float32 [B + B * num_neg], ones then zeros."""
    blocks: List[SampledBlock]
    seeds: torch.Tensor
    pos_src: torch.Tensor
    pos_dst: torch.Tensor
    neg_dst: torch.Tensor
    pairs: EdgePattern
    labels: torch.Tensor


def find_edges(graph: CSRGraph, row: torch.Tensor, col: torch.Tensor) -> torch.Tensor:
    """pos [n] int64: the CSR position of every pair (row[i], col[i]) in `graph` (graph.fwd.col[pos[i]] == col[i] inside row row[i]),
    or -1 where the pair is no entry, as the module docstring defines it.  row, col: [n] node ids, int32 or int64, on the graph's
    device, 1 <= n < 2^31.  Also CSRGraph.find_edges, has_edges (pos >= 0) and reverse_edge_ids (the position of (j, i) for every
    entry (i, j)).  Integers only; two calls give the same bits.
    An id outside [0, N) on either side raises ValueError: it is found on the device, never used as an index, and its flag is the ONE
    host read of the call (one int32).  For that read the call is refused during stream capture.  The wrong type, dtype, rank, length
    or device is a ValueError before any device work.  There is no CPU path and no fallback."""
    op = "find_edges"
    row = _ids(op, graph, row, "row", "n")
    col = _ids(op, graph, col, "col", "n")
    if row.numel() != col.numel():
        raise ValueError(f"pygat_amd {op}: row holds {row.numel()} ids and col {col.numel()}: one pair per index expected")
    _no_capture(op, "pairs cannot be looked up", "the check of row and col is", "look them up")
    n, N, dev = int(row.numel()), graph.n, graph.device
    with torch.cuda.device(dev):
        pos = torch.empty(n, dtype=torch.int64, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.pygat_find_edges(*graph_head(graph), n, row.data_ptr(), col.data_ptr(), pos.data_ptr(), info.data_ptr(), _stream()),
              "find_edges")
        outside = info.item()                                           # the one host read
    if outside:
        raise ValueError(f"pygat_amd {op}: an id in row or col lies outside the graph's nodes [0, {N})")
    return pos


def negative_edges(graph: CSRGraph, src: torch.Tensor, num_neg: int, *, seed: Optional[torch.Tensor] = None, generator=None,
                   hop: int = 0, exclude_self: bool = True, allow_full: bool = False) -> torch.Tensor:
    """Seeded negative destinations: neg [n_src, num_neg] int64, neg[w, s] an id that is no column of row src[w] of `graph` (and, with
    exclude_self, not src[w] itself), as the module docstring defines it.  src: [n_src] node ids, int32 or int64, on the graph's
    device, repeats allowed; num_neg >= 1 and n_src * num_neg < 2^31.  seed: an int64 [1] tensor on the graph's device, read by the
    kernel; None draws one with torch.randint(0, 2**62, ..., generator=generator).  hop in [0, 2^32) separates the draws of one seed.
    The same (seed, hop) gives the same draws, bit for bit, whatever the batch; there is no rejection loop.
    An id of src outside [0, N) raises ValueError: it is found on the device and never used as an index.  A row in which every id is
    forbidden has no candidate: ValueError too, unless allow_full=True, in which case its draws are returned as -1.  Both flags
    arrive in the ONE host read of the call (two int32).  For that read the call is refused during stream capture.  There is no CPU
    path and no fallback."""
    op = "negative_edges"
    _graph(op, graph)
    _at_least_one(op, "num_neg", num_neg)
    _hop(op, hop)
    for name, flag in (("exclude_self", exclude_self), ("allow_full", allow_full)):
        if not isinstance(flag, bool):
            raise ValueError(f"pygat_amd {op}: {name} = {flag!r}: True or False expected")
    if seed is not None:
        seed = _seed(op, graph.device, seed)
    src = _ids(op, graph, src, "src", "n_src")
    n_src, N, dev = int(src.numel()), graph.n, graph.device
    if n_src * num_neg >= 2 ** 31:
        raise ValueError(f"pygat_amd {op}: {n_src} source nodes x {num_neg} draws: fewer than 2^31 draws expected")
    _no_capture(op, "negatives cannot be drawn", "the check of src is", "draw them")
    with torch.cuda.device(dev):
        if seed is None:
            seed = _draw_seed(dev, generator)
        neg = torch.empty(n_src, num_neg, dtype=torch.int64, device=dev)
        info = torch.empty(2, dtype=torch.int32, device=dev)
        check(lib.pygat_draw_negatives(*graph_head(graph), n_src, src.data_ptr(), num_neg, int(exclude_self), seed.data_ptr(), hop,
                                       neg.data_ptr(), info.data_ptr(), _stream()), "draw_negatives")
        outside, full = info.tolist()                                   # the one host read
    if outside:
        raise ValueError(f"pygat_amd {op}: an id in src lies outside the graph's nodes [0, {N})")
    if full and not allow_full:
        raise ValueError(f"pygat_amd {op}: a node in src has no candidate: every one of the {N} nodes is a column of its row"
                         f"{' or the node itself' if exclude_self else ''} (allow_full=True returns -1 for its draws)")
    return neg


EXCLUDE = ("none", "positive", "reverse")


def _excluded(graph: CSRGraph, edge_ids: torch.Tensor, exclude: str) -> Optional[torch.Tensor]:
    """The CSR positions that must not carry messages, repeats and all (None: nothing): the positives, and with "reverse" the
    position of (v, u) for every positive (u, v) that has one (a positive without one stands in for it: no compaction, no read)."""
    if exclude == "none":
        return None
    if exclude == "positive":
        return edge_ids
    rev = graph.reverse_edge_ids()[edge_ids]
    return torch.cat([edge_ids, torch.where(rev >= 0, rev, edge_ids)])


def link_batch(graph: CSRGraph, edge_ids: torch.Tensor, num_neg: int, fanouts: Sequence[Optional[int]], *,
               seed: Optional[torch.Tensor] = None, generator=None, exclude: str = "reverse",
               edge_weight: Optional[torch.Tensor] = None) -> LinkBatch:
    """A link-prediction mini-batch for the B positive edges at the CSR positions `edge_ids` [B] (int32 or int64, on the graph's
    device, repeats allowed) -> LinkBatch(blocks, seeds, pos_src, pos_dst, neg_dst, pairs, labels):
      1. u = the rows, v = the columns of the positives;
      2. neg = negative_edges(graph, u, num_neg, seed=seed, hop=0): num_neg non-neighbours of every u, u itself excluded;
      3. seeds = the distinct ids of u, v and neg, ascending; pos_src, pos_dst, neg_dst are their ranks in it (the local ids of
         induced_subgraph);
      4. blocks = sample_blocks_weighted(graph, seeds, fanouts, w, seed=seed), w = 1 everywhere and 0 at the excluded positions:
         exclude="none" nothing, "positive" the positives, "reverse" (the default) also the position of (v, u) for every positive
         (u, v) that has one -- so that no block carries a message along an edge that is being scored.  w is a table of ones kept with
         the graph, zeroed at the excluded positions for the sampling and set back after it, also when the sampling raises: a batch
         costs O(batch), not O(nnz).  edge_weight [graph.nnz] float32 (sample_neighbors_weighted's) replaces the ones: it is copied
         once per call, and the copy is zeroed in the same way;
      5. pairs and labels as LinkBatch describes them; score = edge_dot(batch.pairs, h, h) over h = the layers over batch.blocks.
    One seed serves the negatives and every hop (the Philox streams differ).  The same seed gives the same batch, bit for bit.
    A GAT pattern holds self loops: leave their positions out of edge_ids -- a self loop is no link to predict, its reverse is
    itself, and excluding it takes the node's own message away.
    Host reads, all of them: the range check of edge_ids (an id outside [0, nnz) is a ValueError before anything is written);
    negative_edges' ONE host read (two flags); the size of torch.unique's result; on a pattern that is not symmetric, once per graph,
    find_edges' read inside graph.reverse_edge_ids(); one read per hop of sample_blocks_weighted (and, once per graph, its largest
    degree); the index check of EdgePattern.from_indices.  Because of them the call is refused during stream capture.  The wrong
    type, dtype, rank or device is a ValueError before any device work.  There is no CPU path and no fallback."""
    op = "link_batch"
    _graph(op, graph)
    _at_least_one(op, "num_neg", num_neg)
    _fanouts(op, fanouts)
    if exclude not in EXCLUDE:
        raise ValueError(f"pygat_amd {op}: exclude = {exclude!r}: one of \"none\", \"positive\", \"reverse\" expected")
    if seed is not None:
        seed = _seed(op, graph.device, seed)
    if edge_weight is not None:
        _weight(op, graph, edge_weight)
    edge_ids = _ids(op, graph, edge_ids, "edge_ids", "B")
    B, nnz, dev = int(edge_ids.numel()), graph.nnz, graph.device
    if B * (2 + num_neg) >= 2 ** 31:
        raise ValueError(f"pygat_amd {op}: {B} positives x (2 + {num_neg}) ids: fewer than 2^31 expected")
    _no_capture(op, "a batch cannot be built", "its checks and counts are", "build it")
    with torch.cuda.device(dev):
        if bool(((edge_ids < 0) | (edge_ids >= nnz)).any()):            # a host read
            raise ValueError(f"pygat_amd {op}: an id in edge_ids lies outside the graph's entries [0, {nnz})")
        if seed is None:
            seed = _draw_seed(dev, generator)
        u, v = graph.fwd.edge_rc[edge_ids, 0].long(), graph.fwd.col[edge_ids].long()
        neg = negative_edges(graph, u, num_neg, seed=seed, hop=0)
        seeds, inv = torch.unique(torch.cat([u, v, neg.flatten()]), sorted=True, return_inverse=True)
        pos_src, pos_dst, neg_dst = inv[:B], inv[B:2 * B], inv[2 * B:].view(B, num_neg)
        excluded = _excluded(graph, edge_ids, exclude)
        if edge_weight is not None:
            w = edge_weight.clone()
            if excluded is not None:
                w[excluded] = 0.0
            blocks = sample_blocks_weighted(graph, seeds, fanouts, w, seed=seed)
        else:
            if getattr(graph, "_link_w", None) is None:
                graph._link_w = torch.ones(nnz, dtype=torch.float32, device=dev)
            w = graph._link_w
            try:
                if excluded is not None:
                    w[excluded] = 0.0
                blocks = sample_blocks_weighted(graph, seeds, fanouts, w, seed=seed)
            finally:
                if excluded is not None:
                    w[excluded] = 1.0
        n_seeds = int(seeds.numel())
        rows = torch.cat([pos_src, pos_src.repeat_interleave(num_neg)])
        cols = torch.cat([pos_dst, neg_dst.flatten()])
        pairs = EdgePattern.from_indices(torch.stack([rows, cols]), (n_seeds, n_seeds))
        labels = torch.cat([torch.ones(B, dtype=torch.float32, device=dev), torch.zeros(B * num_neg, dtype=torch.float32, device=dev)])
    return LinkBatch(blocks, seeds, pos_src, pos_dst, neg_dst, pairs, labels)
