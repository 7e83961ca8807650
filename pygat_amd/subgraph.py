"""Subgraph mini-batches on the K23 kernels (csrc/k23_subgraph.hip): the induced subgraph of a node set as a square CSRGraph -- what
every level and model of this package takes (GAT, SpGraphAttentionLayer(V2), gat_level, return_attention, edge_logits, bf16 tables,
FusedEpoch) -- and as an EdgePattern for the pattern ops; and seeded uniform random walks, GraphSAINT's node sampler.

    nodes = random_walk(g, roots, 4, seed=s).flatten()                 # [n_roots * 5], repeats and all
    sub = induced_subgraph(g, nodes)                                   # or g.subgraph(nodes)
    logits = model(x[sub.nodes], sub.graph)                            # a GAT on the subgraph
    loss = F.nll_loss(logits[sub.index.view(n_roots, 5)[:, 0]], y[roots])

induced_subgraph (tests/subgraph_ref.py restates it in NumPy; the kernels agree with it integer for integer):
  - only the SET of `nodes` counts: ids may repeat and come in any order.  Local ids are ranks in ascending global id: sub.nodes [n] is
    the distinct ids ascending, local node r is sub.nodes[r], and sub.index [n_in] gives the local id of every input id
    (sub.nodes[sub.index] == nodes).  The relabelling is monotone, so nothing is sorted: a row's kept entries, in CSR position order,
    already have strictly ascending local columns, which is what CSRGraph requires;
  - row r holds, in ascending position, the positions p of graph row sub.nodes[r] whose graph.fwd.col[p] is in the set; its local
    column is the rank of that id.  sub.edge_ids [nnz] are those positions, strictly increasing over the whole sub-pattern:
    e_full[sub.edge_ids] gathers per-edge inputs, alpha_full[sub.edge_ids] = alpha scatters returned attention back;
  - sub.pattern is EdgePattern((n, n), edge_rc, rowptr, col, None), as SampledBlock.pattern is built (lazy transpose); sub.graph is
    CSRGraph(rowptr, col, validate=False), built on first access and cached (the kernels' output is well-formed by construction); its
    edge_index() order is the order of edge_ids.  A sub-pattern with a row without entries (sub.n_empty_rows > 0; never with self
    loops in the graph) is a pattern but no graph: sub.graph raises the ValueError CSRGraph gives for a node with no neighbour.

random_walk: walks [n_walk, length + 1] int64, walks[w, 0] = start[w]; for t = 1 .. length, with cur = walks[w, t - 1], [b, e) its
row and d = e - b, the key k is word (t & 3) of Philox-4x32-10 with counter (w, hop, STREAM_WALK, t >> 2) and key (seed & 0xFFFFFFFF,
seed >> 32), and walks[w, t] = col[b + ((k * d) >> 32)]; a walker on a row without entries stays.  Uniform up to d / 2^32; the same
(seed, hop) gives the same walks bit for bit.

Host interaction: ONE read per call -- induced_subgraph: the node count, the entry count, the outside flag and the empty-row count,
four int32 in one copy, after which col / edge_rc / edge_ids are allocated at their exact size; random_walk: one int32 flag.  Because
of that read both are refused during stream capture.  There is no CPU path and no torch fallback.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from ._lib import lib, check
from .dropout import STREAM_WALK    # noqa: F401  (the Philox stream of the step keys; the kernels hold the same constant, csrc/rng.h)
from ._minibatch import _at_least_one, _draw_seed, _graph, _hop, _ids, _no_capture, _seed, _stream, _trim, graph_head
from .graph import CSRGraph
from .spmm import EdgePattern


class InducedSubgraph:
    """The sub-pattern of a graph on a node set (induced_subgraph).  nodes [n] int64: the distinct ids ascending; index [n_in] int64:
    the local id of every input id; edge_ids [nnz] int64: the graph's CSR position of every entry, strictly increasing; rowptr
    [n + 1], col [nnz], edge_rc [nnz, 2]: int32, the CSR the kernels wrote; n, nnz, n_empty_rows: ints read with the one host read.
    pattern: the EdgePattern of shape (n, n) over those tables; graph: the CSRGraph over them, built on first access and cached."""
    _fields = ("nodes", "index", "edge_ids", "rowptr", "col", "edge_rc", "n", "nnz", "n_empty_rows")

    def __init__(self, nodes, index, edge_ids, rowptr, col, edge_rc, n, nnz, n_empty_rows):
        self.nodes, self.index, self.edge_ids, self.rowptr, self.col, self.edge_rc = nodes, index, edge_ids, rowptr, col, edge_rc
        self.n, self.nnz, self.n_empty_rows = int(n), int(nnz), int(n_empty_rows)
        self._pattern = self._graph = None

    @property
    def pattern(self) -> EdgePattern:
        if self._pattern is None:
            self._pattern = EdgePattern((self.n, self.n), self.edge_rc, self.rowptr, self.col, None)
        return self._pattern

    @property
    def graph(self) -> CSRGraph:
        if self._graph is None:
            if self.n_empty_rows:
                raise ValueError(f"CSRGraph: some node has no neighbour (add self loops as utils.py:52 does): {self.n_empty_rows} of the "
                                 f"{self.n} rows of the induced subgraph hold no entry; it is a pattern (sub.pattern) but no graph")
            self._graph = CSRGraph(self.rowptr, self.col, validate=False)
        return self._graph

    def __repr__(self):
        return f"InducedSubgraph(n={self.n}, nnz={self.nnz}, n_empty_rows={self.n_empty_rows})"


def induced_subgraph(graph: CSRGraph, nodes: torch.Tensor) -> InducedSubgraph:
    """The square sub-pattern of `graph` on the set of `nodes` [n_in] (node ids of `graph`, int32 or int64, on its device, n_in >= 1;
    ids may repeat and come in any order), as the module docstring defines it: local ids are ranks in ascending global id, rows keep
    their entries in CSR position order, edge_ids are the graph's positions.  Written as a CSR by the K23 kernels: no sort, no unique,
    integers only; two calls give the same bits.
    An id outside [0, N) raises ValueError: it is found on the device, never used as an index, and its flag arrives with the three
    counts in the ONE host read of the call; a set whose sub-pattern has no entry at all raises ValueError too.  For that read the
    call is refused during stream capture.  The wrong type, dtype, rank or device is a ValueError before any device work.  There is no
    CPU path and no fallback."""
    op = "induced_subgraph"
    nodes = _ids(op, graph, nodes, "nodes", "n_in")
    _no_capture(op, "a subgraph cannot be taken", "its counts and the check of nodes are", "take it")
    n_in, N, nnz, dev = int(nodes.numel()), graph.n, graph.nnz, graph.device
    m = min(n_in, N)
    with torch.cuda.device(dev):
        i32, i64 = dict(dtype=torch.int32, device=dev), dict(dtype=torch.int64, device=dev)
        sub_nodes, index, rowptr, info = torch.empty(m, **i64), torch.empty(n_in, **i64), torch.empty(m + 1, **i32), torch.empty(4, **i32)
        ws = torch.empty(_lib._workspace_bytes("subgraph_workspace_bytes", N, n_in), dtype=torch.uint8, device=dev)
        head = (*graph_head(graph), n_in)
        check(lib.pygat_subgraph_count(*head, nodes.data_ptr(), sub_nodes.data_ptr(), index.data_ptr(), rowptr.data_ptr(),
                                       info.data_ptr(), ws.data_ptr(), _stream()), "subgraph_count")
        n, E, outside, empty = info.tolist()                            # the one host read
        if outside:
            raise ValueError(f"pygat_amd {op}: an id in nodes lies outside the graph's nodes [0, {N})")
        assert 1 <= n <= m and 0 <= E <= nnz and 0 <= empty <= n, (n, m, E, nnz, empty)
        if E == 0:
            raise ValueError(f"pygat_amd {op}: no entry of the graph joins two of the {n} nodes: the sub-pattern is empty")
        sub_nodes, rowptr = _trim(sub_nodes, n), _trim(rowptr, n + 1)
        col, edge_rc, edge_ids = torch.empty(E, **i32), torch.empty(E, 2, **i32), torch.empty(E, **i64)
        check(lib.pygat_subgraph_fill(*head, n, E, sub_nodes.data_ptr(), rowptr.data_ptr(), col.data_ptr(), edge_rc.data_ptr(),
                                      edge_ids.data_ptr(), ws.data_ptr(), _stream()), "subgraph_fill")
    return InducedSubgraph(sub_nodes, index, edge_ids, rowptr, col, edge_rc, n, E, empty)


def random_walk(graph: CSRGraph, start: torch.Tensor, length: int, *, seed: Optional[torch.Tensor] = None, generator=None,
                hop: int = 0) -> torch.Tensor:
    """Seeded uniform random walks from `start` [n_walk] (node ids of `graph`, int32 or int64, on its device; repeats allowed), `length`
    >= 1 steps each -> walks [n_walk, length + 1] int64, walks[:, 0] = start, as the module docstring defines them.  seed: an int64
    [1] tensor on the graph's device, read by the kernel; None draws one with torch.randint(0, 2**62, ..., generator=generator).
    hop in [0, 2^32) separates the draws of one seed.  The same (seed, hop) gives the same walks, bit for bit.  walks.flatten() goes
    straight into induced_subgraph: it needs no de-duplication.
    A start id outside [0, N) raises ValueError: it is found on the device, never used as an index, and its flag is the ONE host
    read of the call (one int32).  For that read the call is refused during stream capture.  There is no CPU path and no fallback."""
    op = "random_walk"
    _graph(op, graph)
    _at_least_one(op, "length", length)
    _hop(op, hop)
    if seed is not None:
        seed = _seed(op, graph.device, seed)
    start = _ids(op, graph, start, "start", "n_walk")
    _no_capture(op, "walks cannot be drawn", "the check of start is", "draw them")
    n_walk, N, dev = int(start.numel()), graph.n, graph.device
    with torch.cuda.device(dev):
        if seed is None:
            seed = _draw_seed(dev, generator)
        walks = torch.empty(n_walk, length + 1, dtype=torch.int64, device=dev)
        info = torch.empty(1, dtype=torch.int32, device=dev)
        check(lib.pygat_random_walk(*graph_head(graph), n_walk, start.data_ptr(), length, seed.data_ptr(), hop, walks.data_ptr(),
                                    info.data_ptr(), _stream()), "random_walk")
        outside = info.item()                                           # the one host read
    if outside:
        raise ValueError(f"pygat_amd {op}: an id in start lies outside the graph's nodes [0, {N})")
    return walks
