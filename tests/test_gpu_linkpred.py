"""pygat_amd.find_edges / negative_edges / link_batch on the GPU against the NumPy restatement (tests/linkpred_ref.py), integer for
integer, on the seeded cases of tests/linkpred_case.py; the refusals; the batch's blocks against sample_blocks_weighted called by hand;
one link-prediction training step end to end.  Every comparison of integers is exact; the one tolerance, of the scores, is
tests/parity.py's."""
import ctypes as C

import numpy as np
import pytest
import torch

import linkpred_case as case
import linkpred_ref as R
import parity

pytestmark = pytest.mark.gpu
DEV = "cuda"
_graphs = {}


def graph(name):
    import pygat_amd as pg
    if name not in _graphs:
        rowptr, col = case.graphs()[name]
        _graphs[name] = pg.CSRGraph(torch.as_tensor(rowptr).to(DEV), torch.as_tensor(col).to(DEV), validate=name not in case.UNVALIDATED)
    return _graphs[name]


def seed_of(value):
    return torch.tensor([value], dtype=torch.int64, device=DEV)


def dev(a, int32=False):
    t = torch.as_tensor(np.ascontiguousarray(a)).to(DEV)
    return t.to(torch.int32) if int32 else t


def same(got, want, what):
    assert got.is_cuda and got.dtype == torch.int64 and got.is_contiguous() and tuple(got.shape) == want.shape, (what, tuple(got.shape))
    assert np.array_equal(got.cpu().numpy(), want), what


# ------------------------------------------------------------------------------------------------------ 1. equality with the reference
@pytest.mark.parametrize("name", case.FIND_NAMES)
def test_find_edges_equals_the_reference(name):
    import pygat_amd as pg
    c = case.find_case(name)
    g = graph(c.graph)
    i32 = name in case.FIND_INT32_CASES
    row, col = dev(c.row, i32), dev(c.col, i32)
    pos = pg.find_edges(g, row, col) if name != "cora-random-64" else g.find_edges(row, col)
    want = case.find_reference(name)
    same(pos, want, name)
    assert torch.equal(g.has_edges(row, col), pos >= 0) and g.has_edges(row, col).dtype == torch.bool
    if name == "cora-own-pairs":
        assert torch.equal(pos, torch.arange(g.nnz, device=DEV))
    if name == "cora-swapped-pairs":
        assert g.symmetric and torch.equal(pos, g.perm_f.long())


@pytest.mark.parametrize("name", case.DRAW_NAMES)
def test_negative_edges_equal_the_reference(name):
    import pygat_amd as pg
    c = case.draw_case(name)
    g = graph(c.graph)
    src = dev(c.src, name in case.DRAW_INT32_CASES)
    neg = pg.negative_edges(g, src, c.num_neg, seed=seed_of(c.seed), hop=c.hop, exclude_self=c.exclude_self, allow_full=True)
    want, full = case.draw_reference(name)
    same(neg, want, name)
    if not full:                                         # without a full row allow_full changes nothing
        again = pg.negative_edges(g, src, c.num_neg, seed=seed_of(c.seed), hop=c.hop, exclude_self=c.exclude_self)
        assert torch.equal(again, neg)
        drawn = g.find_edges(src.long().repeat_interleave(c.num_neg), neg.flatten())
        assert bool((drawn == -1).all()), "no draw is an entry"


def test_one_seed_one_set_of_draws_and_hops_differ():
    import pygat_amd as pg
    g = graph("cora")
    src = dev(case.draw_case("cora-1000-neg5").src)
    seed = seed_of(17)
    a, b = pg.negative_edges(g, src, 5, seed=seed), pg.negative_edges(g, src, 5, seed=seed)
    assert torch.equal(a, b)
    other = pg.negative_edges(g, src, 5, seed=seed, hop=1)
    assert other.shape == a.shape and not torch.equal(other, a)
    assert torch.equal(pg.negative_edges(g, src[:10], 5, seed=seed), a[:10]), "a draw depends on its flat index and its row alone"
    gen = torch.Generator(device=DEV)
    gen.manual_seed(5)
    c = pg.negative_edges(g, src, 5, generator=gen)
    gen.manual_seed(5)
    d = pg.negative_edges(g, src, 5, generator=gen)
    assert torch.equal(c, d) and not torch.equal(c, a)


def test_reverse_edge_ids():
    g = graph("cora")
    rev = g.reverse_edge_ids()
    assert g.symmetric and rev.dtype == torch.int64 and g.reverse_edge_ids() is rev, "cached"
    rc = g.fwd.edge_rc
    assert torch.equal(rev, g.perm_f.long()) and torch.equal(rev, g.find_edges(rc[:, 1], rc[:, 0]))
    a = graph("lengths")
    rowptr, col = case.graphs()["lengths"]
    row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    want = R.find_edges_ref(rowptr, col, col, row_of)
    assert not a.symmetric and (want < 0).sum() > 0 and (want >= 0).sum() > 0
    same(a.reverse_edge_ids(), want, "lengths")
    assert a.reverse_edge_ids() is a.reverse_edge_ids()


# --------------------------------------------------------------------------------------------------------------------- 2. refusals
def test_refusals_from_the_device_flags():
    import pygat_amd as pg
    g = graph("cora")
    N = g.n
    ok = torch.tensor([3, 4, 8], device=DEV)
    for bad in (N, -1, 2 ** 40):                           # found on the device, never used as an index
        ids = torch.tensor([3, bad, 8], device=DEV)
        for row, col in ((ids, ok), (ok, ids)):
            with pytest.raises(ValueError, match=rf"find_edges: an id in row or col lies outside the graph's nodes \[0, {N}\)"):
                pg.find_edges(g, row, col)
        with pytest.raises(ValueError, match=rf"negative_edges: an id in src lies outside the graph's nodes \[0, {N}\)"):
            pg.negative_edges(g, ids, 4, seed=seed_of(1))
        with pytest.raises(ValueError, match=rf"negative_edges: an id in src lies outside the graph's nodes \[0, {N}\)"):
            pg.negative_edges(g, ids, 4, seed=seed_of(1), allow_full=True)
        assert bool((pg.find_edges(g, ok, ok) >= 0).all()), "the next call is served (Cora holds self loops)"
    s7 = graph("small7")
    full = "negative_edges: a node in src has no candidate: every one of the 7 nodes is a column of its row"
    with pytest.raises(ValueError, match=full + " or the node itself"):
        pg.negative_edges(s7, torch.tensor([3, 1], device=DEV), 2, seed=seed_of(1))
    with pytest.raises(ValueError, match=full + r" \(allow_full"):
        pg.negative_edges(s7, torch.tensor([0], device=DEV), 2, seed=seed_of(1), exclude_self=False)
    assert pg.negative_edges(s7, torch.tensor([1], device=DEV), 3, seed=seed_of(1), exclude_self=False).tolist() == [[1, 1, 1]]
    assert pg.negative_edges(s7, torch.tensor([3, 1], device=DEV), 2, seed=seed_of(1), allow_full=True)[1].tolist() == [-1, -1]
    with pytest.raises(ValueError, match=rf"link_batch: an id in edge_ids lies outside the graph's entries \[0, {g.nnz}\)"):
        pg.link_batch(g, torch.tensor([5, g.nnz], device=DEV), 2, [3])
    with pytest.raises(ValueError, match="link_batch: an id in edge_ids lies outside"):
        pg.link_batch(g, torch.tensor([-1, 5], device=DEV), 2, [3])


def test_refused_during_stream_capture():
    import pygat_amd as pg
    g = graph("cora")
    g.reverse_edge_ids()
    torch.cuda.synchronize()
    ids, seed = torch.tensor([3, 4, 8], device=DEV), seed_of(1)          # (nothing is allocated inside the capture)
    for call in (lambda: pg.find_edges(g, ids, ids), lambda: pg.negative_edges(g, ids, 4, seed=seed),
                 lambda: pg.link_batch(g, ids, 2, [3], seed=seed)):
        with pytest.raises(ValueError, match="capture"):
            with torch.cuda.graph(torch.cuda.CUDAGraph()):
                call()
        torch.cuda.synchronize()
    assert pg.find_edges(g, ids, ids).shape == (3,) and pg.negative_edges(g, ids, 4, seed=seed).shape == (3, 4)


def test_the_kernels_use_no_scratch():
    from pygat_amd import _lib
    for name in ("k24_find", "k24_draw"):
        regs, scratch = C.c_int(0), C.c_int(-1)
        _lib.check(_lib.lib.pygat_kernel_footprint(name.encode(), C.byref(regs), C.byref(scratch)), name)
        assert scratch.value == 0 and 0 < regs.value <= 64, (name, regs.value, scratch.value)


# ------------------------------------------------------------------------------------------------------------------ 3. link_batch
@pytest.fixture(scope="module")
def cora_link():
    g = graph("cora")
    return g, dev(case.link_edge_ids()), case.LINK["num_neg"], seed_of(case.LINK["seed"])


def test_the_batch_bookkeeping_equals_the_reference(cora_link):
    import pygat_amd as pg
    from pygat_amd import linkpred
    g, edge_ids, K, seed = cora_link
    B = edge_ids.numel()
    for exclude in ("none", "positive", "reverse"):
        ref = case.link_reference(exclude)
        batch = pg.link_batch(g, edge_ids, K, [5], seed=seed, exclude=exclude)
        assert isinstance(batch, pg.LinkBatch) and len(batch.blocks) == 1
        for name in ("seeds", "pos_src", "pos_dst", "neg_dst"):
            same(getattr(batch, name), getattr(ref, name), (exclude, name))
        assert np.array_equal(batch.seeds[batch.pos_src].cpu().numpy(), ref.u) and np.array_equal(batch.seeds[batch.pos_dst].cpu().numpy(), ref.v)
        assert np.array_equal(batch.seeds[batch.neg_dst].cpu().numpy(), ref.neg)
        assert torch.equal(batch.seeds[batch.neg_dst], pg.negative_edges(g, dev(ref.u), K, seed=seed))
        n = ref.seeds.size
        assert batch.pairs.shape == (n, n) and batch.pairs.nnz == B + B * K
        assert np.array_equal(batch.pairs.edge_rc.cpu().numpy(), np.stack([ref.pair_rows, ref.pair_cols], 1))
        assert batch.labels.dtype == torch.float32 and np.array_equal(batch.labels.cpu().numpy(), ref.labels)
        assert torch.equal(batch.blocks[-1].dst_nodes, batch.seeds)
        excluded = linkpred._excluded(g, edge_ids, exclude)
        got = np.zeros(0, dtype=np.int64) if excluded is None else np.unique(excluded.cpu().numpy())
        assert np.array_equal(got, ref.excluded), exclude
    again = pg.link_batch(g, edge_ids.to(torch.int32), K, [5], seed=seed)
    assert torch.equal(again.blocks[0].edge_ids, batch.blocks[0].edge_ids) and torch.equal(again.neg_dst, batch.neg_dst), "the same bits"


def test_the_blocks_leave_the_positives_out(cora_link):
    import pygat_amd as pg
    g, edge_ids, K, seed = cora_link
    rev = g.reverse_edge_ids()[edge_ids]
    assert bool((rev >= 0).all()) and not bool(torch.isin(rev, edge_ids).any())
    present = {}
    for exclude in ("none", "positive", "reverse"):
        blk = pg.link_batch(g, edge_ids, K, [None], seed=seed, exclude=exclude).blocks[0]
        present[exclude] = (torch.isin(edge_ids, blk.edge_ids), torch.isin(rev, blk.edge_ids), blk.nnz)
    assert bool(present["none"][0].all()) and bool(present["none"][1].all()), "whole rows hold the positives and their reverses"
    assert not bool(present["positive"][0].any()) and bool(present["positive"][1].all())
    assert not bool(present["reverse"][0].any()) and not bool(present["reverse"][1].any())
    n_pos = int(torch.unique(edge_ids).numel())
    assert present["positive"][2] == present["none"][2] - n_pos and present["reverse"][2] == present["none"][2] - 2 * n_pos
    assert bool((g._link_w == 1).all()) and g._link_w.shape == (g.nnz,)


def test_the_blocks_equal_the_weighted_sampler_called_by_hand(cora_link):
    import pygat_amd as pg
    g, edge_ids, K, seed = cora_link
    ref = case.link_reference("reverse")
    batch = pg.link_batch(g, edge_ids, K, [5, 5], seed=seed)
    w = torch.ones(g.nnz, device=DEV)
    w[dev(ref.excluded)] = 0.0
    by_hand = pg.sample_blocks_weighted(g, dev(ref.seeds), [5, 5], w, seed=seed)
    assert len(batch.blocks) == len(by_hand) == 2
    for a, b in zip(batch.blocks, by_hand):
        assert (a.n_dst, a.n_src, a.nnz) == (b.n_dst, b.n_src, b.nnz)
        for name in ("src_nodes", "dst_nodes", "edge_ids"):
            assert torch.equal(getattr(a, name), getattr(b, name)), name
        for name in ("rowptr", "col", "edge_rc"):
            assert torch.equal(getattr(a.pattern, name), getattr(b.pattern, name)), name
        assert not bool(torch.isin(a.edge_ids, dev(ref.excluded)).any())
    assert bool((g._link_w == 1).all())
    # a caller's weights replace the ones: they are copied, the copy is zeroed, the caller's tensor stays
    mine = torch.rand(g.nnz, generator=torch.Generator().manual_seed(1)).to(DEV) + 0.5
    keep = mine.clone()
    got = pg.link_batch(g, edge_ids, K, [5, 5], seed=seed, edge_weight=mine)
    w2 = mine.clone()
    w2[dev(ref.excluded)] = 0.0
    want = pg.sample_blocks_weighted(g, dev(ref.seeds), [5, 5], w2, seed=seed)
    assert torch.equal(mine, keep) and all(torch.equal(a.edge_ids, b.edge_ids) for a, b in zip(got.blocks, want))
    assert not torch.equal(got.blocks[0].edge_ids, batch.blocks[0].edge_ids)


def test_the_weights_are_ones_again_after_a_call_that_raised(cora_link, monkeypatch):
    import pygat_amd as pg
    from pygat_amd import linkpred
    g, edge_ids, K, seed = cora_link
    pg.link_batch(g, edge_ids, K, [5], seed=seed)
    seen = {}

    def failing(graph_, seeds, fanouts, w, seed=None):
        seen["zeros"] = int((w == 0).sum())
        raise RuntimeError("the sampler failed")
    monkeypatch.setattr(linkpred, "sample_blocks_weighted", failing)
    with pytest.raises(RuntimeError, match="the sampler failed"):
        pg.link_batch(g, edge_ids, K, [5], seed=seed)
    assert seen["zeros"] == case.link_reference("reverse").excluded.size and bool((g._link_w == 1).all())


def test_one_training_step(cora_link):
    import pygat_amd as pg
    g, edge_ids, K, seed = cora_link
    B = edge_ids.numel()
    batch = pg.link_batch(g, edge_ids, K, [5, 5], seed=seed)
    H, F, Fin = 4, 8, 32
    gen = torch.Generator().manual_seed(24)
    x = torch.randn(g.n, Fin, generator=gen).to(DEV)
    params = {"W1": torch.randn(Fin, H * F, generator=gen) * 0.2, "a1": torch.randn(H, F, generator=gen) * 0.3,
              "W2": torch.randn(H * F, H * F, generator=gen) * 0.2, "a2": torch.randn(H, F, generator=gen) * 0.3}
    params = {k: v.to(DEV).requires_grad_(True) for k, v in params.items()}
    h = x[batch.blocks[0].src_nodes]
    for t, blk in enumerate(batch.blocks):
        z = (h @ params[f"W{t + 1}"]).view(-1, H, F)
        h = pg.gatv2_attention(blk.pattern, z[:blk.n_dst], z, params[f"a{t + 1}"]).reshape(blk.n_dst, H * F)
        if t == 0:
            h = torch.nn.functional.elu(h)
    assert h.shape == (batch.seeds.numel(), H * F)
    score = pg.edge_dot(batch.pairs, h, h)
    assert score.shape == batch.labels.shape == (B + B * K,)
    loss = torch.nn.functional.binary_cross_entropy_with_logits(score, batch.labels)
    loss.backward()
    assert bool(torch.isfinite(loss.detach())) and float(loss.detach()) > 0
    for name, p in params.items():
        assert p.grad is not None and bool(torch.isfinite(p.grad).all()) and float(p.grad.abs().max()) > 0, name
    h64 = h.detach().double().cpu()
    rows = torch.cat([batch.pos_src, batch.pos_src.repeat_interleave(K)]).cpu()
    cols = torch.cat([batch.pos_dst, batch.neg_dst.flatten()]).cpu()
    want = (h64[rows] * h64[cols]).sum(-1)
    own = (h64.float()[rows] * h64.float()[cols]).sum(-1)
    parity.close_fwd(score, want, "the scores", own)
