"""pygat_amd.sample_neighbors_weighted / sample_blocks_weighted on the GPU against the fp64 restatement
(tests/sampler_weighted_ref.py), entry for entry, on the seeded cases of tests/sample_weighted_case.py (whose gaps at the cut make the
fp32 answer unique); determinism; the inclusion frequencies of successive sampling against their exact values (which does not go
through the restatement); the bad-weight flag; a weighted block through gatv2_attention; the footprints of the new kernels."""
import ctypes as C

import pytest
import torch

import sample_case as base
import sample_weighted_case as case
from test_gpu_sample import DEV, graph, same_block, seed_of

pytestmark = pytest.mark.gpu
NEW_KERNELS = ("k22_count_weighted", "k22_list_weighted", "k22_count_long_weighted", "k22_entries_weighted", "k22_select_wave_weighted",
               "k22_select_block_weighted")
_weights = {}


def weights(name, kind="rand"):
    if (name, kind) not in _weights:
        _weights[name, kind] = torch.as_tensor(case.weights(name, kind).copy()).to(DEV)
    return _weights[name, kind]


# ------------------------------------------------------------------------------------------------------ 1. equality with the reference
@pytest.mark.parametrize("dtype", [torch.int64, torch.int32])
@pytest.mark.parametrize("name", case.case_names())
def test_block_equals_the_reference(name, dtype):
    import pygat_amd as pg
    c = case.case(name)
    dst = torch.as_tensor(c.dst).to(DEV).to(dtype)
    blk = pg.sample_neighbors_weighted(graph(c.graph), dst, c.fanout, weights(c.graph, c.weights), seed=seed_of(c.seed), hop=c.hop)
    same_block(blk, case.reference(name)[0], name)


# ------------------------------------------------------------------------------------------------------------------- 2. two hops
def test_two_hops_equal_the_reference():
    import pygat_amd as pg
    t = case.TWO_HOP
    blocks = pg.sample_blocks_weighted(graph(t["graph"]), torch.as_tensor(case.two_hop_seeds()).to(DEV), list(t["fanouts"]),
                                       weights(t["graph"], t["weights"]), seed=seed_of(t["seed"]))
    refs, _ = case.two_hop_reference()
    assert len(blocks) == len(refs) == 2
    for k, (blk, ref) in enumerate(zip(blocks, refs)):
        same_block(blk, ref, f"two-hop block {k}")
    assert torch.equal(blocks[0].dst_nodes, blocks[1].src_nodes)


# ------------------------------------------------------------------------------------------------------------------- 3. determinism
def test_one_seed_one_block_and_hops_differ():
    import pygat_amd as pg
    g, w = graph("cora"), weights("cora")
    dst = torch.as_tensor(case.case("cora-300-f3").dst).to(DEV)
    seed = seed_of(17)
    a, b = pg.sample_neighbors_weighted(g, dst, 3, w, seed=seed), pg.sample_neighbors_weighted(g, dst, 3, w, seed=seed)
    for x, y in ((a.pattern.rowptr, b.pattern.rowptr), (a.pattern.col, b.pattern.col), (a.pattern.edge_rc, b.pattern.edge_rc),
                 (a.edge_ids, b.edge_ids), (a.src_nodes, b.src_nodes)):
        assert torch.equal(x, y)
    other = pg.sample_neighbors_weighted(g, dst, 3, w, seed=seed, hop=1)
    assert torch.equal(other.pattern.rowptr, a.pattern.rowptr) and not torch.equal(other.edge_ids, a.edge_ids)
    # the weights enter the key: other weights, another sample; and it is not the unweighted sample
    assert not torch.equal(pg.sample_neighbors_weighted(g, dst, 3, weights("cora", "selfloop"), seed=seed).edge_ids, a.edge_ids)
    assert not torch.equal(pg.sample_neighbors(g, dst, 3, seed=seed).edge_ids, a.edge_ids)


# --------------------------------------------------------------------------------------------------------- 4. inclusion frequencies
def test_inclusion_frequencies_are_those_of_successive_sampling():
    """512 rows with the weights (1, 2, 3, 0, 4, 6) at hops 0-7 of seed 2024: 4096 row draws per fanout.  Every entry's frequency
    within 5 binomial standard deviations of the exact probability of successive sampling, by enumeration
    (sample_weighted_case.inclusion_probabilities); the entry of weight 0 never.  Nothing here reads the restatement's clocks: a key
    that is wrong in the kernels and in the restatement alike fails here."""
    import pygat_amd as pg
    rowptr, col = case.freq_graph()
    g = pg.CSRGraph(torch.as_tensor(rowptr).to(DEV), torch.as_tensor(col).to(DEV))
    w = torch.as_tensor(case.freq_weights()).to(DEV)
    dst, seed = torch.arange(case.FREQ_ROWS, device=DEV), seed_of(case.FREQ_SEED)
    for fanout in case.FREQ_FANOUTS:
        counts = torch.zeros(6, dtype=torch.int64, device=DEV)
        for hop in case.FREQ_HOPS:
            blk = pg.sample_neighbors_weighted(g, dst, fanout, w, seed=seed, hop=hop)
            assert blk.nnz == fanout * case.FREQ_ROWS
            counts += torch.bincount(blk.edge_ids % 6, minlength=6)
        case.check_frequencies(counts.cpu().numpy(), fanout)


# ------------------------------------------------------------------------------------------------------------ 5., 6. the bad weights
@pytest.mark.parametrize("row", [0, 21], ids=["short-row", "long-row"])
def test_bad_weights_raise_only_where_they_are_sampled(row):
    import pygat_amd as pg
    g = graph("lengths")
    rowptr, _ = base.graphs()["lengths"]
    seed = seed_of(1)
    inside = torch.tensor([3, row, 8], device=DEV)
    outside = torch.tensor([r for r in range(len(base.LENGTHS)) if r != row], device=DEV)
    good = weights("lengths")
    for bad in (-1.0, float("nan"), float("-inf")):
        w = good.clone()
        w[int(rowptr[row + 1]) - 2] = bad
        for fanout in (3, None):
            with pytest.raises(ValueError, match="sample_neighbors_weighted: edge_weight is negative or NaN at an entry of a sampled row"):
                pg.sample_neighbors_weighted(g, inside, fanout, w, seed=seed)
        with pytest.raises(ValueError, match="sample_neighbors_weighted: edge_weight is negative or NaN"):
            pg.sample_blocks_weighted(g, inside, [3], w, seed=seed)
        # the same weights, rows that do not hold the entry: served, and equal to the block of the good weights
        ok = pg.sample_neighbors_weighted(g, outside, 7, w, seed=seed)
        assert torch.equal(ok.edge_ids, pg.sample_neighbors_weighted(g, outside, 7, good, seed=seed).edge_ids)
    ok = pg.sample_neighbors_weighted(g, inside, 3, good, seed=seed)               # and the next call is served
    assert ok.n_dst == 3 and ok.nnz == 9


def test_refusals_that_need_the_device():
    import pygat_amd as pg
    g, w = graph("cora"), weights("cora")
    dst = torch.tensor([3, 4, 8], device=DEV)
    with pytest.raises(ValueError, match="sample_neighbors_weighted: edge_weight lives on cpu, the graph on cuda:0"):
        pg.sample_neighbors_weighted(g, dst, 3, w.cpu())
    with pytest.raises(ValueError, match="sample_blocks_weighted: edge_weight lives on cpu"):
        pg.sample_blocks_weighted(g, dst, [3], w.cpu())
    with pytest.raises(ValueError, match="an id repeats in dst"):
        pg.sample_neighbors_weighted(g, torch.tensor([5, 9, 5], device=DEV), 3, w)
    with pytest.raises(ValueError, match=r"an id in dst lies outside the graph's nodes"):
        pg.sample_neighbors_weighted(g, torch.tensor([3, g.n, 8], device=DEV), 3, w)
    seed = seed_of(1)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="capture"):
        with torch.cuda.graph(torch.cuda.CUDAGraph()):
            pg.sample_neighbors_weighted(g, dst, 3, w, seed=seed)
    torch.cuda.synchronize()
    assert pg.sample_neighbors_weighted(g, dst, 3, w, seed=seed).n_dst == 3


# ------------------------------------------------------------------------------------------------ 7. a weighted block goes through K21
def test_a_weighted_block_through_gatv2_attention():
    import pygat_amd as pg
    c = case.case("cora-selfloop-f5")
    ref, _ = case.reference(c.name)
    blk = pg.sample_neighbors_weighted(graph("cora"), torch.as_tensor(c.dst).to(DEV), c.fanout, weights("cora", "selfloop"),
                                       seed=seed_of(c.seed), hop=c.hop)
    via = pg.EdgePattern.from_indices(torch.as_tensor(ref.edge_rc.T.copy()).to(DEV), (ref.n_dst, ref.n_src))
    gen = torch.Generator().manual_seed(8)
    H, F = 4, 16
    x_dst, x_src, a, G = (torch.randn(*s, generator=gen).to(DEV) for s in ((ref.n_dst, H, F), (ref.n_src, H, F), (H, F), (ref.n_dst, H, F)))

    def run(pattern):
        leaves = [t.clone().requires_grad_(True) for t in (x_dst, x_src, a)]
        out = pg.gatv2_attention(pattern, *leaves)
        return [out.detach()] + list(torch.autograd.grad(out, leaves, G))
    got, want = run(blk.pattern), run(via)
    for k, (x, y) in enumerate(zip(got, want)):
        assert torch.equal(x, y), k
    assert all(bool(torch.isfinite(x).all()) and float(x.abs().max()) > 0 for x in got)
    # the self loop of every row is in the block: the row attends to itself, as the reference's +I makes it
    rows, cols = blk.pattern.edge_rc[:, 0], blk.pattern.edge_rc[:, 1]
    assert int((rows == cols).sum()) == blk.n_dst


# ------------------------------------------------------------------------------------------------------------------- 8. footprints
@pytest.mark.parametrize("name", NEW_KERNELS)
def test_no_new_kernel_uses_scratch(name):
    from pygat_amd import _lib
    torch.cuda.init()
    regs, scratch = C.c_int(-1), C.c_int(-1)
    _lib.check(_lib.lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)), name)
    assert scratch.value == 0 and 0 < regs.value <= 128, (name, regs.value, scratch.value)
