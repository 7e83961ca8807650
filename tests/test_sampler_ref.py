"""The NumPy restatement of the neighbour sampler (tests/sampler_ref.py) keeps the invariants of a block on every seeded case of
tests/sample_case.py, nests over fanouts, and draws every subset of a row equally often.  No GPU, no torch."""
import numpy as np
import pytest

import sample_case as case
import sampler_ref as R


def check_block(blk, rowptr, col, dst, fanout):
    dst = np.asarray(dst, dtype=np.int64)
    assert blk.n_dst == dst.size and blk.rowptr.shape == (dst.size + 1,) and blk.rowptr[0] == 0 and blk.rowptr[-1] == blk.nnz
    lens = np.diff(blk.rowptr)
    assert (lens >= 0).all(), "rowptr is monotone"
    deg = rowptr[dst + 1] - rowptr[dst]
    assert np.array_equal(lens, deg if fanout is None else np.minimum(deg, fanout))
    assert blk.col.shape == (blk.nnz,) and (blk.col >= 0).all() and (blk.col < blk.n_src).all()
    assert blk.src_nodes.shape == (blk.n_src,) and np.array_equal(blk.src_nodes[:blk.n_dst], dst)
    assert np.unique(blk.src_nodes).size == blk.n_src, "src_nodes are distinct"
    assert (np.diff(blk.src_nodes[blk.n_dst:]) > 0).all(), "the tail ascends"
    assert np.array_equal(col[blk.edge_ids], blk.src_nodes[blk.col])
    row_of = np.repeat(np.arange(dst.size), lens)
    assert np.array_equal(blk.edge_rc[:, 0], row_of) and np.array_equal(blk.edge_rc[:, 1], blk.col)
    assert (blk.edge_ids >= rowptr[dst][row_of]).all() and (blk.edge_ids < rowptr[dst + 1][row_of]).all()
    inside = np.ones(blk.nnz, dtype=bool)
    inside[blk.rowptr[:-1][lens > 0]] = False
    assert (np.diff(blk.edge_ids)[inside[1:]] > 0).all(), "edge_ids ascend inside a row"
    used = np.zeros(blk.n_src, dtype=bool)
    used[blk.col] = True
    assert used[blk.n_dst:].all(), "every source after dst is some entry's column"


@pytest.mark.parametrize("name", case.case_names())
def test_invariants_on_every_case(name):
    c = case.case(name)
    rowptr, col = case.graphs()[c.graph]
    check_block(case.reference(name), rowptr, col, c.dst, c.fanout)


def test_two_hop_blocks_chain():
    rowptr, col = case.graphs()["cora"]
    outer, inner = case.two_hop_reference()
    seeds = case.two_hop_seeds()
    check_block(inner, rowptr, col, seeds, case.TWO_HOP["fanouts"][-1])
    check_block(outer, rowptr, col, inner.src_nodes, case.TWO_HOP["fanouts"][0])
    assert np.array_equal(outer.dst_nodes, inner.src_nodes) and outer.n_dst == inner.n_src
    # the hop word separates the draws: hop 1 of the seeds' own rows is not hop 0 at the same fanout
    again = R.sample_neighbors_ref(rowptr, col, seeds, 3, case.TWO_HOP["seed"], hop=1)
    assert not np.array_equal(again.edge_ids, inner.edge_ids)


def test_the_cases_cover_what_they_are_meant_to():
    g = case.graphs()
    rowptr, _ = g["lengths"]
    b, e = rowptr[:len(case.LENGTHS)], rowptr[1:len(case.LENGTHS) + 1]
    q = np.array([case.quads(int(x), int(y)) for x, y in zip(b, e)])
    lens = e - b
    assert tuple(lens) == case.LENGTHS
    for fanout in (7, 60, 200):
        assert {fanout - 1, fanout, fanout + 1, 2 * fanout} <= set(lens.tolist())
    assert {63, 64, 65, 255, 256, 257} <= set(lens.tolist())
    assert sorted(q[lens == 256].tolist()) == [64, 65], "a 256-entry row on either side of the path boundary"
    assert q[lens == 253][0] == 64 and q[lens == 257][0] == 65 and q[lens <= 253].max() <= 64
    assert lens.max() >= 2 * 257 and lens.max() > 2 * 1024, "a long row of several emit rounds"
    names = case.case_names()
    assert sum(n.startswith("cora-") for n in names) == 12 and "tie" in names
    # (d) each relabel branch, in the reference's block of the descending case
    blk = case.reference("relabel-descending-fNone")
    rp, col = g["relabel"]
    dst = case.case("relabel-descending-fNone").dst
    gcol = col[blk.edge_ids]
    assert np.isin(gcol, dst).any() and (~np.isin(gcol, dst)).any(), "a neighbour that is a dst node, and one that is not"
    assert 3 in dst and 3 not in gcol, "a dst node that is nobody's neighbour"
    assert (gcol == 5).sum() == 3, "one neighbour kept by several rows"
    assert (np.diff(dst) < 0).all() and not (np.diff(case.case("relabel-shuffled-f2").dst) > 0).all()


def test_the_tie_case_is_a_tie():
    """Row 0 of the tie graph at seed 0, hop 0: five pairs of equal keys, the lowest with exactly 20607 keys below it, so that fanout
    20608 keeps the earlier position of that pair and not the later.  If the key layout changes, this fails instead of passing
    vacuously."""
    pairs, below, earlier, later = case.tie_facts()
    assert pairs == 5 and below == case.TIE_FANOUT - 1 == 20607 and earlier < later
    blk = case.reference("tie")
    assert blk.nnz == case.TIE_FANOUT
    kept = set(blk.edge_ids.tolist())
    assert earlier in kept and later not in kept
    k = R.keys(0, 0, blk.edge_ids)
    assert k.max() == R.keys(0, 0, [later])[0] and (k == k.max()).sum() == 1


def test_keys_follow_the_layout():
    from philox_ref import philox4x32_10
    seed = (5 << 32) | 9
    w = philox4x32_10(np.array([[3, 2, 4, 0]]), (9, 5))[0]
    assert np.array_equal(R.keys(seed, 2, [12, 13, 14, 15]), w)
    assert not np.array_equal(R.keys(seed, 2, [12, 13, 14, 15]), R.keys(seed, 3, [12, 13, 14, 15]))
    assert R.STREAM_SAMPLE == 4
    from pygat_amd.dropout import STREAM_SAMPLE, STREAM_X, STREAM_WH, STREAM_ATT
    assert STREAM_SAMPLE == 4 and STREAM_SAMPLE not in (STREAM_X, STREAM_WH, STREAM_ATT)


def test_nesting_over_fanouts():
    rowptr, col = case.graphs()["cora"]
    dst = case.case("cora-300-f5").dst
    small = R.sample_neighbors_ref(rowptr, col, dst, 3, 77)
    large = R.sample_neighbors_ref(rowptr, col, dst, 5, 77)
    assert small.nnz < large.nnz and set(small.edge_ids.tolist()) <= set(large.edge_ids.tolist())
    rowptr, col = case.graphs()["lengths"]
    dst = np.arange(len(case.LENGTHS))
    nested = [set(R.sample_neighbors_ref(rowptr, col, dst, f, 99).edge_ids.tolist()) for f in (7, 60, 200, None)]
    assert all(a < b for a, b in zip(nested[:-1], nested[1:]))


def test_every_entry_of_a_row_is_kept_equally_often():
    """A 20-entry row at fanout 10 over the seeds 0 .. 1999: every entry is kept in 45 % to 55 % of the draws (p = 0.5 and n = 2000
    give sd = 1.1 %: the band is 4.5 sd; the seeds are fixed, so the outcome is a fact)."""
    counts = np.zeros(20, dtype=np.int64)
    for seed in range(2000):
        kept = R.kept_positions(37, 57, 10, seed, 0)
        assert kept.size == 10
        counts[kept - 37] += 1
    assert counts.sum() == 20000 and counts.min() >= 900 and counts.max() <= 1100, counts
