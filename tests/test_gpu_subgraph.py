"""pygat_amd.induced_subgraph / random_walk on the GPU against the NumPy restatement (tests/subgraph_ref.py), integer for integer, on
the seeded cases of tests/subgraph_case.py; the refusals; the subgraph going through the levels and models as a CSRGraph and through
the pattern ops as an EdgePattern; one GraphSAINT step end to end.  Every comparison is exact: there is no tolerance in this file."""
import os

import numpy as np
import pytest
import torch

import subgraph_case as case

pytestmark = pytest.mark.gpu
DEV = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_graphs = {}


def graph(name):
    import pygat_amd as pg
    if name not in _graphs:
        if name == "citeseer":
            z = np.load(os.path.join(GOLDEN, "citeseer_csr.npz"), allow_pickle=False)
            rowptr, col = z["rowptr"].astype(np.int64), z["col"].astype(np.int64)
        else:
            rowptr, col = case.graphs()[name]
        # (the "hole" graph has a row without entries: a CSRGraph only unvalidated)
        _graphs[name] = pg.CSRGraph(torch.as_tensor(rowptr).to(DEV), torch.as_tensor(col).to(DEV), validate=name != "hole")
    return _graphs[name]


def seed_of(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def same_sub(sub, ref, what):
    assert (sub.n, sub.nnz, sub.n_empty_rows) == (ref.n, ref.nnz, ref.n_empty_rows), (what, sub, ref.n, ref.nnz, ref.n_empty_rows)
    for name in ("rowptr", "col", "edge_rc", "edge_ids", "nodes", "index"):
        got, want = getattr(sub, name), getattr(ref, name)
        assert got.is_cuda and got.is_contiguous() and tuple(got.shape) == want.shape, (what, name, tuple(got.shape), want.shape)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (what, name)
    assert sub.rowptr.dtype == sub.col.dtype == sub.edge_rc.dtype == torch.int32
    assert sub.edge_ids.dtype == sub.nodes.dtype == sub.index.dtype == torch.int64
    p = sub.pattern
    assert p.shape == (ref.n, ref.n) and p.nnz == ref.nnz and p.perm is None and not p.has_transpose, what
    assert p.rowptr is sub.rowptr and p.col is sub.col and p.edge_rc is sub.edge_rc and sub.pattern is p


# ------------------------------------------------------------------------------------------------------ 1. equality with the reference
@pytest.mark.parametrize("name", case.SUB_NAMES)
def test_subgraph_equals_the_reference(name):
    import pygat_amd as pg
    c = case.case(name)
    g = graph(c.graph)
    nodes = torch.as_tensor(c.nodes).to(DEV)
    if name in case.INT32_CASES:
        nodes = nodes.to(torch.int32)                    # both index dtypes
    sub = pg.induced_subgraph(g, nodes) if name != "cora-300" else g.subgraph(nodes)
    ref = case.reference(name)
    same_sub(sub, ref, name)
    if c.graph == "lengths":                             # asymmetric, sub-rows come out empty: a pattern, and a graph only without them
        if ref.n_empty_rows:
            with pytest.raises(ValueError, match="CSRGraph: some node has no neighbour"):
                sub.graph
        return
    assert ref.n_empty_rows == 0
    sg = sub.graph
    assert sub.graph is sg and sg.n == ref.n and sg.nnz == ref.nnz and sg.fwd.rowptr is sub.rowptr and sg.fwd.col is sub.col
    assert torch.equal(sg.edge_index(), sub.edge_rc.t().long()), "edge_index() order is the order of edge_ids"


def test_the_whole_node_range_gives_the_graph_back():
    import pygat_amd as pg
    g = graph("cora")
    sub = pg.induced_subgraph(g, torch.arange(g.n, device=DEV))
    assert sub.n == g.n and sub.nnz == g.nnz and sub.n_empty_rows == 0
    assert torch.equal(sub.rowptr, g.fwd.rowptr) and torch.equal(sub.col, g.fwd.col) and torch.equal(sub.edge_rc, g.fwd.edge_rc)
    assert torch.equal(sub.edge_ids, torch.arange(g.nnz, device=DEV))
    assert torch.equal(sub.nodes, torch.arange(g.n, device=DEV)) and torch.equal(sub.index, sub.nodes)


def test_order_and_repeats_do_not_count():
    import pygat_amd as pg
    g = graph("relabel")
    subs = [pg.induced_subgraph(g, torch.tensor(ids, device=DEV)) for ids in ([0, 1], [1, 0], [0, 1, 0])]
    for s in subs[1:]:
        for name in ("rowptr", "col", "edge_rc", "edge_ids", "nodes"):
            assert torch.equal(getattr(s, name), getattr(subs[0], name)), name
    assert [s.index.tolist() for s in subs] == [[0, 1], [1, 0], [0, 1, 0]]
    again = pg.induced_subgraph(g, torch.tensor([0, 1], device=DEV))
    assert torch.equal(again.col, subs[0].col) and torch.equal(again.edge_ids, subs[0].edge_ids), "two calls, the same bits"


# --------------------------------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_from_the_device_flags():
    import pygat_amd as pg
    g = graph("cora")
    N = g.n
    for bad in (N, -1, 2 ** 40):                           # found on the device, never used as an index
        with pytest.raises(ValueError, match=rf"induced_subgraph: an id in nodes lies outside the graph's nodes \[0, {N}\)"):
            pg.induced_subgraph(g, torch.tensor([3, bad, 8], device=DEV))
        with pytest.raises(ValueError, match=rf"random_walk: an id in start lies outside the graph's nodes \[0, {N}\)"):
            pg.random_walk(g, torch.tensor([3, bad, 8], device=DEV), 4, seed=seed_of(1))
        ok = pg.induced_subgraph(g, torch.tensor([3, 4, 8], device=DEV))                       # and the next call is served
        assert ok.n == 3 and ok.nnz >= 3
    name, lone = case.NO_ENTRY
    with pytest.raises(ValueError, match="induced_subgraph: no entry of the graph joins two of the 1 nodes"):
        pg.induced_subgraph(graph(name), torch.as_tensor(lone).to(DEV))
    torch.cuda.synchronize()
    nodes, seed = torch.tensor([3, 4, 8], device=DEV), seed_of(1)          # (nothing is allocated inside the capture)
    for call in (lambda: pg.induced_subgraph(g, nodes), lambda: pg.random_walk(g, nodes, 4, seed=seed)):
        with pytest.raises(ValueError, match="capture"):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                call()
        torch.cuda.synchronize()
    ok = pg.induced_subgraph(g, nodes)
    assert ok.n == 3 and ok.nnz >= 3 and pg.random_walk(g, nodes, 4, seed=seed_of(1)).shape == (3, 5)


def test_refusals_before_any_device_work():
    import pygat_amd as pg
    g = graph("cora")
    ids = torch.tensor([3, 4, 8], device=DEV)
    for op, name, call in (("induced_subgraph", "nodes", lambda t: pg.induced_subgraph(g, t)),
                           ("random_walk", "start", lambda t: pg.random_walk(g, t, 4))):
        with pytest.raises(ValueError, match=f"{op}: {name} must be int32 or int64, not torch.float32"):
            call(ids.float())
        with pytest.raises(ValueError, match=f"{op}: {name} .* >= 1 expected, got \\(3, 1\\)"):
            call(ids.view(3, 1))
        with pytest.raises(ValueError, match=f"{op}: {name} .* >= 1 expected, got \\(0,\\)"):
            call(ids[:0])
        with pytest.raises(ValueError, match=f"{op}: {name} must be a tensor on the GPU"):
            call(ids.cpu())
    with pytest.raises(ValueError, match="induced_subgraph: a CSRGraph expected, not EdgePattern"):
        pg.induced_subgraph(g.edge_pattern(), ids)


# ---------------------------------------------------------------------------------------------------- 3. the subgraph is a graph
@pytest.fixture(scope="module")
def citeseer_block():
    """Citeseer as the second block of block_diag([cora, citeseer]), taken out again by induced_subgraph."""
    import pygat_amd as pg
    cora, cite = graph("cora"), graph("citeseer")
    g = pg.CSRGraph.block_diag([cora, cite])
    sub = pg.induced_subgraph(g, torch.arange(cora.n, cora.n + cite.n, device=DEV))
    return g, sub, cite, cora


def test_the_second_block_comes_out_whole(citeseer_block):
    g, sub, cite, cora = citeseer_block
    assert sub.n == cite.n and sub.nnz == cite.nnz and sub.n_empty_rows == 0
    assert torch.equal(sub.rowptr, cite.fwd.rowptr) and torch.equal(sub.col, cite.fwd.col)
    assert torch.equal(sub.edge_ids, cora.nnz + torch.arange(cite.nnz, device=DEV))
    assert torch.equal(sub.nodes, cora.n + torch.arange(cite.n, device=DEV)) and torch.equal(sub.index, torch.arange(cite.n, device=DEV))
    assert torch.equal(sub.graph.edge_index(), cite.edge_index()) and sub.graph.symmetric == cite.symmetric


def _level(fn, graph_, x, Ws, As, G):
    leaves = [t.clone().requires_grad_(True) for t in [x] + Ws + As]
    out = fn(leaves[0], graph_, leaves[1:1 + len(Ws)], leaves[1 + len(Ws):], None, 0.2, True)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, G))


@pytest.mark.parametrize("kind", ["gat_level", "gatv2_level"])
def test_a_level_on_the_subgraph_equals_the_level_on_the_graph(citeseer_block, kind):
    import pygat_amd as pg
    g, sub, cite, cora = citeseer_block
    H, Fin, Fo = 8, 32, 8
    gen = torch.Generator().manual_seed(23)
    x = torch.randn(cite.n, Fin, generator=gen).to(DEV)
    v2 = kind == "gatv2_level"
    Ws = [(torch.randn((2 if v2 else 1) * Fin, Fo, generator=gen) * 0.2).to(DEV) for _ in range(H)]
    As = [(torch.randn(1, Fo if v2 else 2 * Fo, generator=gen) * 0.3).to(DEV) for _ in range(H)]
    G = torch.randn(cite.n, H * Fo, generator=gen).to(DEV)
    fn = getattr(pg, kind)
    got, want = _level(fn, sub.graph, x, Ws, As, G), _level(fn, cite, x, Ws, As, G)
    assert len(got) == 2 + 2 * H
    for k, (a, b) in enumerate(zip(got, want)):
        assert torch.equal(a, b), (kind, k)
    assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in got)


def test_a_model_on_the_subgraph_equals_the_model_on_the_graph(citeseer_block):
    import pygat_amd as pg
    g, sub, cite, cora = citeseer_block
    torch.manual_seed(5)
    model = pg.GAT(nfeat=[32, 8, 6], nheads=[8, 1], nlayers=2, dropout=0.6, alpha=0.2, layer_type=pg.SpGraphAttentionLayer).to(DEV).eval()
    x = torch.randn(cite.n, 32, generator=torch.Generator().manual_seed(6)).to(DEV)
    with torch.no_grad():
        got, want = model(x, sub.graph), model(x, cite)
    assert got.shape == (cite.n, 6) and torch.equal(got, want) and bool(torch.isfinite(got).all())


def test_returned_attention_scatters_back_through_edge_ids():
    import pygat_amd as pg
    g = graph("cora")
    sub = pg.induced_subgraph(g, torch.as_tensor(case.case("cora-300").nodes).to(DEV))
    H, Fin, Fo = 4, 16, 8
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(g.n, Fin, generator=gen).to(DEV)
    Ws = [(torch.randn(Fin, Fo, generator=gen) * 0.2).to(DEV) for _ in range(H)]
    As = [(torch.randn(1, 2 * Fo, generator=gen) * 0.3).to(DEV) for _ in range(H)]
    out, alpha = pg.gat_level(x[sub.nodes], sub.graph, Ws, As, None, 0.2, True, return_attention=True)
    _, alpha_full = pg.gat_level(x, g, Ws, As, None, 0.2, True, return_attention=True)
    assert out.shape == (sub.n, H * Fo) and alpha.shape == (sub.nnz, H) and alpha_full.shape == (g.nnz, H)
    assert alpha_full[sub.edge_ids].shape == alpha.shape
    back = torch.zeros_like(alpha_full)
    back[sub.edge_ids] = alpha                                      # edge_ids are distinct: a plain scatter
    assert int((back.abs().sum(1) > 0).sum()) == sub.nnz
    # the row of a local edge is the local id of the row of its position in the graph, and so is its column
    full_rc = g.edge_index()[:, sub.edge_ids]
    assert torch.equal(sub.nodes[sub.edge_rc[:, 0].long()], full_rc[0]) and torch.equal(sub.nodes[sub.edge_rc[:, 1].long()], full_rc[1])


# -------------------------------------------------------------------------------------------------- 4. the subgraph is a pattern
def _run(op, pattern, leaves, G):
    leaves = [t.clone().requires_grad_(True) for t in leaves]
    out = op(pattern, *leaves)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, G))


@pytest.fixture(scope="module")
def cora_sub():
    import pygat_amd as pg
    ref = case.reference("cora-300")
    sub = pg.induced_subgraph(graph("cora"), torch.as_tensor(case.case("cora-300").nodes).to(DEV))
    via = pg.EdgePattern.from_indices(torch.as_tensor(ref.edge_rc.T.copy()).to(DEV), (ref.n, ref.n))
    gen = torch.Generator().manual_seed(8)
    H, F = 4, 16
    t = dict(x_dst=torch.randn(ref.n, H, F, generator=gen), x_src=torch.randn(ref.n, H, F, generator=gen),
             v=torch.randn(ref.n, H, F, generator=gen), a=torch.randn(H, F, generator=gen), s_dst=torch.randn(ref.n, H, generator=gen),
             s_src=torch.randn(ref.n, H, generator=gen), G=torch.randn(ref.n, H, F, generator=gen))
    return sub, via, {k: v.to(DEV) for k, v in t.items()}


@pytest.mark.parametrize("op", ["gatv2_attention", "additive_attention", "dot_attention"])
def test_the_subgraph_through_the_pattern_ops(cora_sub, op):
    import pygat_amd as pg
    sub, via, t = cora_sub
    leaves = {"gatv2_attention": [t["x_dst"], t["x_src"], t["a"], t["v"]], "additive_attention": [t["s_dst"], t["s_src"], t["v"]],
              "dot_attention": [t["x_dst"], t["x_src"], t["v"]]}[op]
    got, want = _run(getattr(pg, op), sub.pattern, leaves, t["G"]), _run(getattr(pg, op), via, leaves, t["G"])
    assert sub.pattern.has_transpose, "the backward built the lazy transpose"
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (op, k)
    assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in got)


# ------------------------------------------------------------------------------------------------- 5. walks equal the reference
@pytest.mark.parametrize("name", case.WALK_NAMES)
def test_walks_equal_the_reference(name):
    import pygat_amd as pg
    c = case.walk_case(name)
    start = torch.as_tensor(c.start).to(DEV)
    if name in case.WALK_INT32_CASES:
        start = start.to(torch.int32)
    walks = pg.random_walk(graph(c.graph), start, c.length, seed=seed_of(c.seed), hop=c.hop)
    ref = case.walk_reference(name)
    assert walks.dtype == torch.int64 and walks.is_contiguous() and tuple(walks.shape) == ref.shape == (c.start.size, c.length + 1)
    assert np.array_equal(walks.cpu().numpy(), ref), name
    if name == "tie-4096-at-0":                          # d = 2^17: the high word of k * d, not k % d or a 32-bit product
        first = walks[:, 1].cpu().numpy()
        assert np.unique(first).size > 3900 and first.max() > (1 << 16) and np.array_equal(walks[:, 2].cpu().numpy(), first)
    if name == "hole":
        w = walks.cpu().numpy()
        assert np.all(w[w[:, 0] == 2] == 2), "a walker that starts on the row without entries stays there"


def test_one_seed_one_set_of_walks_and_hops_differ():
    import pygat_amd as pg
    g = graph("cora")
    start = torch.as_tensor(case.walk_case("cora-1000-len9").start).to(DEV)
    seed = seed_of(17)
    a, b = pg.random_walk(g, start, 9, seed=seed), pg.random_walk(g, start, 9, seed=seed)
    assert torch.equal(a, b)
    other = pg.random_walk(g, start, 9, seed=seed, hop=1)
    assert torch.equal(other[:, 0], a[:, 0]) and not torch.equal(other, a)
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    c = pg.random_walk(g, start, 9, generator=gen)
    gen.manual_seed(5)
    d = pg.random_walk(g, start, 9, generator=gen)
    assert torch.equal(c, d) and not torch.equal(c, a)


# -------------------------------------------------------------------------------------------- 6. one GraphSAINT step end to end
def test_one_graphsaint_step():
    import pygat_amd as pg
    g = graph("cora")
    n_roots, length, C = 64, 4, 7
    gen = torch.Generator().manual_seed(12)
    x = torch.randn(g.n, 48, generator=gen).to(DEV)
    y = torch.randint(0, C, (g.n,), generator=gen).to(DEV)
    roots = torch.randperm(g.n, generator=gen)[:n_roots].to(DEV)
    torch.manual_seed(3)
    model = pg.GAT(nfeat=[48, 8, C], nheads=[4, 2], nlayers=2, dropout=0.0, alpha=0.2, layer_type=pg.SpGraphAttentionLayer).to(DEV).train()
    walks = pg.random_walk(g, roots, length, seed=seed_of(99))
    sub = pg.induced_subgraph(g, walks.flatten())
    assert torch.equal(sub.nodes[sub.index], walks.flatten()) and n_roots <= sub.n <= n_roots * (length + 1)
    logits = model(x[sub.nodes], sub.graph)
    assert logits.shape == (sub.n, C)
    at_roots = sub.index.view(n_roots, length + 1)[:, 0]
    assert torch.equal(sub.nodes[at_roots], roots)
    loss = torch.nn.functional.cross_entropy(logits[at_roots], y[roots])
    loss.backward()
    params = list(model.named_parameters())
    assert len(params) == 2 * (4 + 2)
    for name, p in params:
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
