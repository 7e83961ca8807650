"""Seeded neighbour sampling on the K22 kernels (csrc/k22_sample.hip): the block -- destination nodes x sampled sources -- that the
pattern ops (dot_attention, additive_attention, gatv2_attention and their variants, spmm, edge_softmax) take as an EdgePattern.

    blk = sample_neighbors(graph, dst, fanout=10, seed=seed)            # one block around `dst`
    out = gatv2_attention(blk.pattern, x[blk.dst_nodes], x[blk.src_nodes], a)
    blocks = sample_blocks(graph, seeds, [10, 25], seed=seed)           # a mini-batch of two layers, outermost hop first
    h = x[blocks[0].src_nodes]
    for blk, layer in zip(blocks, layers):
        h = layer(blk.pattern, h[:blk.n_dst], h)

What is sampled (tests/sampler_ref.py restates it in NumPy; the kernels agree with it entry for entry):
  - the entry at position p of the graph's CSR (graph.fwd.col[p]) has the 32-bit key: word (p & 3) of Philox-4x32-10 with counter
    (p >> 2, hop, STREAM_SAMPLE, 0) and key (seed & 0xFFFFFFFF, seed >> 32).  It depends on the position only;
  - row r of the block is node dst[r].  A row of at most `fanout` entries is kept whole; otherwise the `fanout` entries smallest in
    (key, p) are kept.  Kept entries stay in ascending position, so their global columns ascend.  Every fanout-subset of a row is
    equally likely, and with one seed the sample at a smaller fanout is a subset of the sample at a larger one;
  - src_nodes = dst in the caller's order, then every other kept column once in ascending id; the local column of a node is its index
    in src_nodes, so x_dst = x_src[:n_dst] (the block convention of DGL and PyG).

Weighted by edge (sample_neighbors_weighted / sample_blocks_weighted; tests/sampler_weighted_ref.py restates it in fp64): with
edge_weight [graph.nnz] float32, one weight per entry at its CSR position (the index of blk.edge_ids), the entry at position p with the
key k above and w = edge_weight[p] is never sampled if w == 0; if w > 0 (finite or +inf) its clock is E(k) / w, E(k) = -ln(1 - (k +
0.5) / 2^32) a unit exponential variate, and a row keeps its `fanout` entries smallest in (clock, p) among those of positive weight --
all of them if they number at most `fanout`.  That is weighted sampling without replacement (Efraimidis-Spirakis): the first entry
drawn is entry i with probability w_i / sum w, the next among the rest in the same way.  w = +inf gives the clock 0: the entry is
always kept ("always keep the self loop").  A negative or NaN weight in a sampled row is a ValueError.  The kernels compute the clock
in fp32 (csrc/rng.h: sample_weighted_key), a few ulps from the exact value, and order its bit pattern.  Everything else is as above.

    w = torch.where(is_self_loop, torch.inf, 1.0 / degree[graph.fwd.col])                       # [graph.nnz] float32
    blocks = sample_blocks_weighted(graph, seeds, [10, 25], w, seed=seed)

Host interaction: one read per hop -- the two counts (entries, sources) and the validity flags (two of dst; the weights' one), four
or five int32 in one copy -- and, once per graph, its largest degree (it bounds the output buffers, which are allocated before anything is known about the sample).
Because of that read, sampling is refused during stream capture.  There is no CPU path and no torch fallback.
"""
from __future__ import annotations

from typing import List, NamedTuple, Optional, Sequence

import torch

from . import _lib
from ._lib import lib, check
from ._minibatch import _at_least_one, _draw_seed, _graph, _hop, _ids, _no_capture, _seed, _stream, _trim, graph_head
from .dropout import STREAM_SAMPLE    # noqa: F401  (the Philox stream of the keys above; the kernels hold the same constant, csrc/rng.h)
from .graph import CSRGraph
from .spmm import EdgePattern

KEEP_ALL = 2 ** 31 - 1     # the fanout the kernels take for "whole rows"


class SampledBlock(NamedTuple):
    """One sampled block.  pattern: an EdgePattern of shape (n_dst, n_src) whose rowptr / col / edge_rc the kernels wrote (perm is
    None: the entry order is the CSR order, as in CSRGraph.edge_pattern(); its transpose is built on first use by transposed()).
    src_nodes [n_src], dst_nodes [n_dst]: int64 global ids, src_nodes[:n_dst] == dst_nodes.  edge_ids [nnz]: int64, the graph's CSR
    position of every entry -- e_full[blk.edge_ids] gathers per-edge inputs for gatv2_attention_edge / dot_attention_edge."""
    pattern: EdgePattern
    src_nodes: torch.Tensor
    dst_nodes: torch.Tensor
    edge_ids: torch.Tensor
    n_dst: int
    n_src: int
    nnz: int


def _fanout(op: str, fanout) -> int:
    return KEEP_ALL if fanout is None else _at_least_one(op, "fanout", fanout, "an int >= 1, or None for whole rows, expected")


def _max_degree(graph: CSRGraph) -> int:
    """The graph's largest degree, read once per graph."""
    if getattr(graph, "_max_degree", None) is None:
        rp = graph.fwd.rowptr
        graph._max_degree = int((rp[1:] - rp[:-1]).max().item())
    return graph._max_degree


def _checked(op: str, graph, dst, fanout, seed, hop):
    """Every refusal that needs no device work -> (dst int64 contiguous, fanout as the kernels take it, seed or None)."""
    _graph(op, graph)
    fanout = _fanout(op, fanout)
    _hop(op, hop)
    if seed is not None:
        seed = _seed(op, graph.device, seed)
    return _ids(op, graph, dst, "dst", "n_dst", limit=False), fanout, seed     # (n_dst is held against graph.n in _sample)


def _weight(op: str, graph, w):
    """The refusals of edge_weight, none of which needs device work."""
    if not isinstance(w, torch.Tensor):
        raise ValueError(f"pygat_amd {op}: edge_weight must be a float32 tensor [graph.nnz], not {type(w).__name__}")
    if w.dtype != torch.float32:
        raise ValueError(f"pygat_amd {op}: edge_weight must be float32, not {w.dtype}")
    if tuple(w.shape) != (graph.nnz,):
        raise ValueError(f"pygat_amd {op}: edge_weight {tuple(w.shape)}: one weight per entry of the graph, [{graph.nnz}], expected")
    if w.device != graph.device:
        raise ValueError(f"pygat_amd {op}: edge_weight lives on {w.device}, the graph on {graph.device}")
    if not w.is_contiguous():
        raise ValueError(f"pygat_amd {op}: edge_weight must be contiguous (it is read in place, never copied)")
    return w


def _sample(op: str, graph, dst, fanout, weight, seed, generator, hop) -> SampledBlock:
    """One block, uniform (weight None: pygat_sample_block) or weighted by edge (pygat_weighted_block, whose info has a fifth word)."""
    dst, fanout, seed = _checked(op, graph, dst, fanout, seed, hop)
    if weight is not None:
        weight = _weight(op, graph, weight)
    n_dst, N, nnz, dev = int(dst.numel()), graph.n, graph.nnz, graph.device
    if n_dst > N:
        raise ValueError(f"pygat_amd {op}: dst holds {n_dst} ids but the graph has {N} nodes: some id repeats")
    _no_capture(op, "a block cannot be sampled", "its counts and the check of dst are", "sample")
    with torch.cuda.device(dev):
        if seed is None:
            seed = _draw_seed(dev, generator)
        cap = max(1, min(n_dst * min(fanout, _max_degree(graph)), nnz))
        src_cap = n_dst + min(cap, N)
        i32 = dict(dtype=torch.int32, device=dev)
        rowptr, col, edge_rc = torch.empty(n_dst + 1, **i32), torch.empty(cap, **i32), torch.empty(cap, 2, **i32)
        edge_ids = torch.empty(cap, dtype=torch.int64, device=dev)
        src_nodes = torch.empty(src_cap, dtype=torch.int64, device=dev)
        info = torch.empty(4 if weight is None else 5, **i32)
        ws = torch.empty(_lib._workspace_bytes("sample_workspace_bytes", N, n_dst), dtype=torch.uint8, device=dev)
        head = (*graph_head(graph), n_dst, dst.data_ptr(), fanout)
        tail = (seed.data_ptr(), hop, cap, src_cap, rowptr.data_ptr(), col.data_ptr(), edge_rc.data_ptr(), edge_ids.data_ptr(),
                src_nodes.data_ptr(), info.data_ptr(), ws.data_ptr(), _stream())
        if weight is None:
            check(lib.pygat_sample_block(*head, *tail), "sample_block")
        else:
            check(lib.pygat_weighted_block(*head, weight.data_ptr(), *tail), "weighted_block")
        E, n_src, outside, repeat, *bad = info.tolist()               # the one host read
    if outside:
        raise ValueError(f"pygat_amd {op}: an id in dst lies outside the graph's nodes [0, {N})")
    if repeat:
        raise ValueError(f"pygat_amd {op}: an id repeats in dst (the destination nodes of a block are distinct)")
    if bad and bad[0]:
        raise ValueError(f"pygat_amd {op}: edge_weight is negative or NaN at an entry of a sampled row (weights are >= 0; 0 never "
                         f"samples an entry, inf always keeps it)")
    assert 0 <= E <= cap and n_dst <= n_src <= src_cap, (E, cap, n_src, src_cap)
    col, edge_rc, edge_ids, src_nodes = _trim(col, E), _trim(edge_rc, E), _trim(edge_ids, E), _trim(src_nodes, n_src)
    pattern = EdgePattern((n_dst, n_src), edge_rc, rowptr, col, None)
    return SampledBlock(pattern, src_nodes, dst, edge_ids, n_dst, n_src, E)


def _fanouts(op: str, fanouts) -> None:
    if isinstance(fanouts, (str, bytes)) or not hasattr(fanouts, "__len__") or len(fanouts) < 1:
        raise ValueError(f"pygat_amd {op}: fanouts: a non-empty list of fanouts (one per layer) expected")
    for f in fanouts:
        _fanout(op, f)


def _hops(graph, seeds, fanouts, weight, seed, generator) -> List[SampledBlock]:
    """The chain of hops of sample_blocks / sample_blocks_weighted, outermost first."""
    op = "sample_neighbors" if weight is None else "sample_neighbors_weighted"
    if seed is None:
        with torch.cuda.device(graph.device):
            seed = _draw_seed(graph.device, generator)
    blocks, dst = [], seeds
    for t in range(len(fanouts)):
        blocks.append(_sample(op, graph, dst, fanouts[-1 - t], weight, seed, None, t))
        dst = blocks[-1].src_nodes
    return blocks[::-1]


def sample_neighbors(graph: CSRGraph, dst: torch.Tensor, fanout: Optional[int], *, seed: Optional[torch.Tensor] = None, generator=None,
                     hop: int = 0) -> SampledBlock:
    """The block of `dst` [n_dst] (distinct node ids of `graph`, int32 or int64, on its device) with at most `fanout` neighbours per
    node (an int >= 1; None keeps whole rows), as the module docstring defines it.  seed: an int64 [1] tensor on the graph's device,
    read by the kernels; None draws one with torch.randint(0, 2**62, ..., generator=generator).  hop in [0, 2^32) separates the draws
    of one seed.  The same (seed, hop) gives the same block, bit for bit; nothing is sorted and all arithmetic is integer.
    A repeated id in dst, or one outside [0, N), raises ValueError: both are found on the device -- an id outside the graph is never
    used as an index -- and their flags arrive with the block's two counts in the ONE host read of the call.  For that read sampling
    is refused during stream capture.  There is no CPU path and no fallback."""
    return _sample("sample_neighbors", graph, dst, fanout, None, seed, generator, hop)


def sample_neighbors_weighted(graph: CSRGraph, dst: torch.Tensor, fanout: Optional[int], edge_weight: torch.Tensor, *,
                              seed: Optional[torch.Tensor] = None, generator=None, hop: int = 0) -> SampledBlock:
    """sample_neighbors with the neighbours drawn in proportion to `edge_weight`, without replacement, as the module docstring defines
    it: edge_weight is float32 [graph.nnz] on the graph's device, contiguous (a strided one is refused, not copied), one weight per
    entry at its CSR position (graph.fwd.col order, the index of edge_ids).  0 never samples an entry, +inf always keeps it, and a row
    keeps at most `fanout` entries of positive weight (None: all of them).  The same (seed, hop, weights) gives the same block, bit
    for bit; with one seed the sample at a smaller fanout is a subset of the one at a larger fanout.
    A negative or NaN weight raises ValueError if it lies in a row of `dst`: it is found on the device, is never selected, and its flag
    arrives in the ONE host read of the call with the counts and the flags of dst.  Rows that the call does not visit are NOT checked:
    a bad weight elsewhere in the graph goes unnoticed.  The wrong dtype, shape or device is a ValueError before any device work.
    Refused during stream capture; no CPU path and no fallback."""
    if edge_weight is None:
        raise ValueError("pygat_amd sample_neighbors_weighted: edge_weight must be a float32 tensor [graph.nnz], not NoneType")
    return _sample("sample_neighbors_weighted", graph, dst, fanout, edge_weight, seed, generator, hop)


def sample_blocks(graph: CSRGraph, seeds: torch.Tensor, fanouts: Sequence[Optional[int]], *, seed: Optional[torch.Tensor] = None,
                  generator=None) -> List[SampledBlock]:
    """The blocks of a len(fanouts)-layer mini-batch around `seeds`: hop 0 samples around the seeds with fanouts[-1], hop t around the
    previous hop's src_nodes with fanouts[-1 - t]; the list is returned OUTERMOST hop first, so that
        h = x[blocks[0].src_nodes]
        for blk, layer in zip(blocks, layers): h = layer(blk.pattern, h[:blk.n_dst], h)
    ends with one row per seed.  One seed serves all hops (the hop number is a word of the Philox counter).  One host read per hop."""
    op = "sample_blocks"
    _fanouts(op, fanouts)
    _checked(op, graph, seeds, fanouts[-1], seed, 0)
    return _hops(graph, seeds, fanouts, None, seed, generator)


def sample_blocks_weighted(graph: CSRGraph, seeds: torch.Tensor, fanouts: Sequence[Optional[int]], edge_weight: torch.Tensor, *,
                           seed: Optional[torch.Tensor] = None, generator=None) -> List[SampledBlock]:
    """sample_blocks with every hop drawn by sample_neighbors_weighted: ONE weight tensor [graph.nnz] serves all hops (a hop reads the
    weights of the rows it visits), one seed serves all hops, one host read per hop."""
    op = "sample_blocks_weighted"
    _fanouts(op, fanouts)
    _checked(op, graph, seeds, fanouts[-1], seed, 0)
    _weight(op, graph, edge_weight)                                 # (None included: no tensor)
    return _hops(graph, seeds, fanouts, edge_weight, seed, generator)
