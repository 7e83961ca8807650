"""The fp64 restatement of the neighbour sampler weighted by edge (tests/sampler_weighted_ref.py) on the seeded cases of
tests/sample_weighted_case.py: the gap condition that makes every case's answer unique in fp32, the invariants of a block, nesting
over fanouts, the zero and +inf rules, and the inclusion frequencies of successive sampling.  No GPU, no torch."""
import numpy as np
import pytest

import sample_case as base
import sample_weighted_case as case
import sampler_ref as R
import sampler_weighted_ref as W


def check_block(blk, rowptr, col, dst, fanout, w):
    dst = np.asarray(dst, dtype=np.int64)
    assert blk.n_dst == dst.size and blk.rowptr.shape == (dst.size + 1,) and blk.rowptr[0] == 0 and blk.rowptr[-1] == blk.nnz
    lens = np.diff(blk.rowptr)
    positive = np.array([(w[rowptr[i]:rowptr[i + 1]] > 0).sum() for i in dst])
    assert np.array_equal(lens, positive if fanout is None else np.minimum(positive, fanout))
    assert (w[blk.edge_ids] > 0).all(), "an entry of weight 0 is never kept"
    assert blk.col.shape == (blk.nnz,) and (blk.col >= 0).all() and (blk.col < blk.n_src).all()
    assert blk.src_nodes.shape == (blk.n_src,) and np.array_equal(blk.src_nodes[:blk.n_dst], dst)
    assert np.unique(blk.src_nodes).size == blk.n_src and (np.diff(blk.src_nodes[blk.n_dst:]) > 0).all()
    assert np.array_equal(col[blk.edge_ids], blk.src_nodes[blk.col])
    row_of = np.repeat(np.arange(dst.size), lens)
    assert np.array_equal(blk.edge_rc[:, 0], row_of) and np.array_equal(blk.edge_rc[:, 1], blk.col)
    assert (blk.edge_ids >= rowptr[dst][row_of]).all() and (blk.edge_ids < rowptr[dst + 1][row_of]).all()
    inside = np.ones(blk.nnz, dtype=bool)
    inside[blk.rowptr[:-1][lens > 0]] = False
    assert (np.diff(blk.edge_ids)[inside[1:]] > 0).all(), "edge_ids ascend inside a row"
    # every +inf entry of a row is kept, up to the fanout, the first by position
    for r, i in enumerate(dst):
        inf = rowptr[i] + np.nonzero(np.isinf(w[rowptr[i]:rowptr[i + 1]]))[0]
        kept = blk.edge_ids[blk.rowptr[r]:blk.rowptr[r + 1]]
        assert set(inf[:fanout].tolist()) <= set(kept.tolist())
        if fanout is not None and inf.size >= fanout:
            assert np.array_equal(kept, inf[:fanout])


@pytest.mark.parametrize("name", case.case_names())
def test_gap_condition_and_invariants_on_every_case(name):
    c = case.case(name)
    rowptr, col = base.graphs()[c.graph]
    blk, gaps = case.reference(name)
    cut = ~np.isnan(gaps)
    print(f"{name}: {int(cut.sum())} rows cut, smallest gap {gaps[cut].min() if cut.any() else None}")
    assert (gaps[cut] >= case.MIN_GAP).all(), (name, gaps[cut].min())
    assert cut.any() or c.fanout is None
    check_block(blk, rowptr, col, c.dst, c.fanout, case.weights(c.graph, c.weights))


def test_two_hop_blocks_chain_and_keep_the_gap():
    rowptr, col = base.graphs()["cora"]
    (outer, inner), gaps = case.two_hop_reference()
    w = case.weights("cora", case.TWO_HOP["weights"])
    for g in gaps:
        assert np.nanmin(g) >= case.MIN_GAP
    check_block(inner, rowptr, col, case.two_hop_seeds(), case.TWO_HOP["fanouts"][-1], w)
    check_block(outer, rowptr, col, inner.src_nodes, case.TWO_HOP["fanouts"][0], w)
    assert np.array_equal(outer.dst_nodes, inner.src_nodes) and outer.n_dst == inner.n_src


def test_the_cases_cover_what_they_are_meant_to():
    rowptr, col = base.graphs()["lengths"]
    w = case.weights("lengths", "exact")
    positive = {r: int((w[rowptr[r]:rowptr[r + 1]] > 0).sum()) for r in case.EXACT_ROWS}
    assert positive == case.EXACT_ROWS and {case.EXACT_FANOUT - 1, case.EXACT_FANOUT, case.EXACT_FANOUT + 1} == set(positive.values())
    q = {r: base.quads(int(rowptr[r]), int(rowptr[r + 1])) for r in case.EXACT_ROWS}
    for want in (4, 5, 6):                       # each count on a row of the wave and on a row of the work-group
        assert any(positive[r] == want and q[r] <= base.WAVE_QUADS for r in q)
        assert any(positive[r] == want and q[r] > base.WAVE_QUADS for r in q)
    for r in case.EXACT_ROWS:
        assert (w[rowptr[r]:rowptr[r + 1]] == 0).sum() >= 8 and w[rowptr[r]] > 0 and w[rowptr[r + 1] - 1] > 0
    w = case.weights("lengths")
    share = (w == 0).mean()
    assert 0.13 < share < 0.17 and w[w > 0].min() >= 0.05 and w.max() <= 4.0 and w.dtype == np.float32
    # the +inf cases: a self loop per Cora row; more +inf entries than the fanout in row 0 of the relabel graph, as many in row 5
    rp, col = base.graphs()["cora"]
    w = case.weights("cora", "selfloop")
    assert all(np.isinf(w[rp[i]:rp[i + 1]]).sum() == 1 for i in range(rp.size - 1))
    rp, col = base.graphs()["relabel"]
    w = case.weights("relabel", "inftie")
    assert np.isinf(w[rp[0]:rp[1]]).sum() == 3 and np.isinf(w[rp[5]:rp[6]]).sum() == 2 and case.case("relabel-inftie-f2").fanout == 2
    blk, gaps = case.reference("relabel-inftie-f2")
    assert np.isinf(gaps[1]) and blk.edge_ids[2:4].tolist() == [rp[0], rp[0] + 2], "cut between two clocks of 0: by position"


def test_the_clock_is_the_exponential_of_the_key():
    p = np.arange(64)
    w = np.full(64, 2.0, dtype=np.float32)
    k = R.keys(9, 1, p).astype(np.float64)
    assert np.allclose(W.clocks(9, 1, p, w), -np.log(1 - (k + 0.5) / 2 ** 32) / 2, rtol=1e-12)
    w[3] = np.inf
    assert W.clocks(9, 1, p, w)[3] == 0
    # unit weights order a row as the unweighted sampler does: the clock is monotone in the key
    kept, gap = W.kept_positions(37, 57, 10, 5, 0, np.ones(100, dtype=np.float32))
    assert np.array_equal(kept, R.kept_positions(37, 57, 10, 5, 0)) and gap > 0


def test_nesting_over_fanouts():
    rowptr, col = base.graphs()["lengths"]
    dst = np.arange(len(base.LENGTHS))
    w = case.weights("lengths")
    nested = [set(W.sample_neighbors_weighted_ref(rowptr, col, dst, f, w, 99)[0].edge_ids.tolist()) for f in (7, 60, 200, 256, None)]
    assert all(a < b for a, b in zip(nested[:-1], nested[1:]))
    assert nested[-1] == set(np.nonzero(w[:rowptr[len(base.LENGTHS)]] > 0)[0].tolist()), "None keeps every entry of positive weight"
    small, large = case.reference("cora-selfloop-f3")[0], case.reference("cora-selfloop-f5")[0]
    assert small.nnz < large.nnz and set(small.edge_ids.tolist()) <= set(large.edge_ids.tolist())


@pytest.mark.parametrize("bad", [-1.0, -0.001, float("nan"), float("-inf")])
def test_a_bad_weight_is_refused_in_a_sampled_row_only(bad):
    rowptr, col = base.graphs()["relabel"]
    w = case.weights("relabel").copy()
    w[rowptr[2] + 1] = bad
    with pytest.raises(ValueError, match="negative or NaN"):
        W.sample_neighbors_weighted_ref(rowptr, col, [0, 2], 2, w, 3)
    W.sample_neighbors_weighted_ref(rowptr, col, [0, 1, 4], 2, w, 3)


def test_inclusion_frequencies_of_the_reference():
    """Successive sampling: 4096 row draws per fanout, every frequency within 5 binomial standard deviations of the exact probability
    (the seeds are fixed, so the outcome is a fact)."""
    rowptr, col = case.freq_graph()
    w = case.freq_weights()
    dst = np.arange(case.FREQ_ROWS)
    assert np.allclose(case.inclusion_probabilities((1, 1, 1, 1), 2), 0.5)
    assert np.allclose(case.inclusion_probabilities((1, 3), 1), (0.25, 0.75))
    for fanout in case.FREQ_FANOUTS:
        counts = np.zeros(6, dtype=np.int64)
        for hop in case.FREQ_HOPS:
            blk, _ = W.sample_neighbors_weighted_ref(rowptr, col, dst, fanout, w, case.FREQ_SEED, hop)
            counts += np.bincount(blk.edge_ids % 6, minlength=6)
        case.check_frequencies(counts, fanout)
