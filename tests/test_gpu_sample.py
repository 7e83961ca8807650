"""pygat_amd.sample_neighbors / sample_blocks on the GPU against the NumPy restatement (tests/sampler_ref.py), integer for integer,
on the seeded cases of tests/sample_case.py; determinism, the refusals that come from the device flags, and the sampled blocks
going through the pattern ops."""
import numpy as np
import pytest
import torch

import sample_case as case

pytestmark = pytest.mark.gpu
DEV = "cuda"
_graphs = {}


def graph(name):
    import pygat_amd as pg
    if name not in _graphs:
        rowptr, col = case.graphs()[name]
        _graphs[name] = pg.CSRGraph(torch.as_tensor(rowptr).to(DEV), torch.as_tensor(col).to(DEV))
    return _graphs[name]


def seed_of(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def same_block(blk, ref, what):
    p = blk.pattern
    assert (blk.n_dst, blk.n_src, blk.nnz) == (ref.n_dst, ref.n_src, ref.nnz), what
    assert p.shape == (ref.n_dst, ref.n_src) and p.nnz == ref.nnz and p.perm is None and not p.has_transpose, what
    for name, got, want in (("rowptr", p.rowptr, ref.rowptr), ("col", p.col, ref.col), ("edge_rc", p.edge_rc, ref.edge_rc),
                            ("edge_ids", blk.edge_ids, ref.edge_ids), ("src_nodes", blk.src_nodes, ref.src_nodes),
                            ("dst_nodes", blk.dst_nodes, ref.dst_nodes)):
        assert got.is_cuda and tuple(got.shape) == want.shape, (what, name, tuple(got.shape), want.shape)
        assert np.array_equal(got.cpu().numpy().astype(np.int64), want), (what, name)
    assert p.rowptr.dtype == p.col.dtype == p.edge_rc.dtype == torch.int32
    assert blk.edge_ids.dtype == blk.src_nodes.dtype == blk.dst_nodes.dtype == torch.int64


# ------------------------------------------------------------------------------------------------------ 1. equality with the reference
@pytest.mark.parametrize("name", case.case_names())
def test_block_equals_the_reference(name):
    import pygat_amd as pg
    c = case.case(name)
    dst = torch.as_tensor(c.dst).to(DEV)
    if name.endswith("f3"):
        dst = dst.to(torch.int32)                      # both index dtypes
    blk = pg.sample_neighbors(graph(c.graph), dst, c.fanout, seed=seed_of(c.seed), hop=c.hop)
    same_block(blk, case.reference(name), name)
    if name == "tie":
        pairs, below, earlier, later = case.tie_facts()
        kept = set(blk.edge_ids.tolist())
        assert below == c.fanout - 1 and earlier in kept and later not in kept


def test_two_hops_equal_the_reference():
    import pygat_amd as pg
    t = case.TWO_HOP
    blocks = pg.sample_blocks(graph(t["graph"]), torch.as_tensor(case.two_hop_seeds()).to(DEV), list(t["fanouts"]), seed=seed_of(t["seed"]))
    refs = case.two_hop_reference()
    assert len(blocks) == len(refs) == 2
    for k, (blk, ref) in enumerate(zip(blocks, refs)):
        same_block(blk, ref, f"two-hop block {k}")
    assert torch.equal(blocks[0].dst_nodes, blocks[1].src_nodes)


# ------------------------------------------------------------------------------------------------------------------- 2. determinism
def test_one_seed_one_block_and_hops_differ():
    import pygat_amd as pg
    g = graph("cora")
    dst = torch.as_tensor(case.case("cora-300-f3").dst).to(DEV)
    seed = seed_of(17)
    a, b = pg.sample_neighbors(g, dst, 3, seed=seed), pg.sample_neighbors(g, dst, 3, seed=seed)
    for x, y in ((a.pattern.rowptr, b.pattern.rowptr), (a.pattern.col, b.pattern.col), (a.pattern.edge_rc, b.pattern.edge_rc),
                 (a.edge_ids, b.edge_ids), (a.src_nodes, b.src_nodes)):
        assert torch.equal(x, y)
    other = pg.sample_neighbors(g, dst, 3, seed=seed, hop=1)
    assert torch.equal(other.pattern.rowptr, a.pattern.rowptr) and not torch.equal(other.edge_ids, a.edge_ids)
    # a seed drawn from a generator: the same generator state gives the same block
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    c = pg.sample_neighbors(g, dst, 3, generator=gen)
    gen.manual_seed(5)
    d = pg.sample_neighbors(g, dst, 3, generator=gen)
    assert torch.equal(c.edge_ids, d.edge_ids) and not torch.equal(c.edge_ids, a.edge_ids)


# --------------------------------------------------------------------------------------------------------------------- 3. refusals
def test_refusals_from_the_device_flags():
    import pygat_amd as pg
    g = graph("cora")
    N = g.n
    seed = seed_of(1)
    with pytest.raises(ValueError, match="an id repeats in dst"):
        pg.sample_neighbors(g, torch.tensor([5, 9, 5], device=DEV), 3, seed=seed)
    for bad in (N, N + 12345, -1, 2 ** 40):                   # handled as an empty row on the device, never used as an index
        with pytest.raises(ValueError, match=rf"an id in dst lies outside the graph's nodes \[0, {N}\)"):
            pg.sample_neighbors(g, torch.tensor([3, bad, 8], device=DEV), 3, seed=seed)
    torch.cuda.synchronize()
    dst = torch.tensor([3, 4, 8], device=DEV)
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            pg.sample_neighbors(g, dst, 3, seed=seed)
    torch.cuda.synchronize()
    ok = pg.sample_neighbors(g, dst, 3, seed=seed)               # and the next call is served
    assert ok.n_dst == 3 and ok.nnz >= 3


# ------------------------------------------------------------------------------------------------- 4. the full-rows pass-through
def test_whole_rows_of_every_node_give_the_graph_back():
    import pygat_amd as pg
    g = graph("cora")
    N = g.n
    blk = pg.sample_neighbors(g, torch.arange(N, device=DEV), None, seed=seed_of(2))
    full = g.edge_pattern()
    assert blk.n_src == N and torch.equal(blk.src_nodes, torch.arange(N, device=DEV)) and blk.nnz == g.nnz
    assert torch.equal(blk.pattern.rowptr, full.rowptr) and torch.equal(blk.pattern.col, full.col)
    assert torch.equal(blk.pattern.edge_rc, full.edge_rc) and torch.equal(blk.edge_ids, torch.arange(g.nnz, device=DEV))
    gen = torch.Generator().manual_seed(3)
    x, a = torch.randn(N, 4, 16, generator=gen).to(DEV), torch.randn(4, 16, generator=gen).to(DEV)
    assert torch.equal(pg.gatv2_attention(blk.pattern, x, x, a), pg.gatv2_attention(full, x, x, a))


# ------------------------------------------------------------------------------------------- 5., 6. blocks go through the pattern ops
@pytest.fixture(scope="module")
def sampled():
    """One sampled Cora block (fanout 5, 64 destinations), the same block through EdgePattern.from_indices of the reference's
    indices, and tables for it."""
    import pygat_amd as pg
    c = case.case("cora-64-f5")
    ref = case.reference(c.name)
    blk = pg.sample_neighbors(graph("cora"), torch.as_tensor(c.dst).to(DEV), c.fanout, seed=seed_of(c.seed), hop=c.hop)
    via = pg.EdgePattern.from_indices(torch.as_tensor(ref.edge_rc.T.copy()).to(DEV), (ref.n_dst, ref.n_src))
    gen = torch.Generator().manual_seed(8)
    H, F = 4, 16
    t = dict(x_dst=torch.randn(ref.n_dst, H, F, generator=gen), x_src=torch.randn(ref.n_src, H, F, generator=gen),
             v=torch.randn(ref.n_src, H, F, generator=gen), a=torch.randn(H, F, generator=gen), s_dst=torch.randn(ref.n_dst, H, generator=gen),
             s_src=torch.randn(ref.n_src, H, generator=gen), G=torch.randn(ref.n_dst, H, F, generator=gen),
             e_full=torch.randn(graph("cora").nnz, H, F, generator=gen))
    return blk, via, ref, {k: v.to(DEV) for k, v in t.items()}


def _run(op, pattern, leaves, G):
    leaves = [t.clone().requires_grad_(True) for t in leaves]
    out = op(pattern, *leaves)
    return [out.detach()] + list(torch.autograd.grad(out, leaves, G))


@pytest.mark.parametrize("op", ["gatv2_attention", "additive_attention", "dot_attention"])
def test_a_sampled_block_through_the_pattern_ops(sampled, op):
    import pygat_amd as pg
    blk, via, ref, t = sampled
    leaves = {"gatv2_attention": [t["x_dst"], t["x_src"], t["a"], t["v"]], "additive_attention": [t["s_dst"], t["s_src"], t["v"]],
              "dot_attention": [t["x_dst"], t["x_src"], t["v"]]}[op]
    got, want = _run(getattr(pg, op), blk.pattern, leaves, t["G"]), _run(getattr(pg, op), via, leaves, t["G"])
    assert blk.pattern.has_transpose, "the backward built the lazy transpose"
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), (op, k)
    assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in got)


def test_edge_ids_gather_the_per_edge_inputs(sampled):
    import pygat_amd as pg
    blk, via, ref, t = sampled
    ids = torch.as_tensor(ref.edge_ids).to(DEV)
    op = lambda pattern, x_dst, x_src, a, e: pg.gatv2_attention_edge(pattern, x_dst, x_src, a, e)  # noqa: E731
    got = _run(op, blk.pattern, [t["x_dst"], t["x_src"], t["a"], t["e_full"][blk.edge_ids]], t["G"])
    want = _run(op, via, [t["x_dst"], t["x_src"], t["a"], t["e_full"][ids]], t["G"])
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), k
    plain = pg.gatv2_attention(blk.pattern, t["x_dst"], t["x_src"], t["a"])
    assert not torch.equal(got[0], plain), "e enters the score"
