"""tests/linkpred_ref.py against restatements that share nothing with it: the sorted list of allowed ids for the rank formula, the
rows by hand, membership for the draws, the counts for their uniformity.  No torch, no GPU."""
import itertools

import numpy as np

import linkpred_case as case
import linkpred_ref as R


def _allowed(N, cols, u, exclude_self):
    bad = set(int(c) for c in cols) | ({u} if exclude_self else set())
    return [x for x in range(N) if x not in bad]


def _check_rank(N, cols, u, exclude_self):
    allowed = _allowed(N, cols, u, exclude_self)
    got = [R.nth_non_neighbour(cols, u, N, r, exclude_self) for r in range(len(allowed))]
    assert got == allowed, (N, list(cols), u, exclude_self, got, allowed)


def test_the_rank_formula_equals_brute_force():
    """Every (N <= 8, subset, u, r, exclude_self): 2^N subsets each; beyond that, 150 seeded subsets per N up to 12 and 40 per N up
    to 40, with 3 seeded u each."""
    for N in range(1, 9):
        for k in range(N + 1):
            for cols in itertools.combinations(range(N), k):
                for u in range(N):
                    for ex in (True, False):
                        _check_rank(N, np.asarray(cols, dtype=np.int64), u, ex)
    rng = np.random.default_rng(0)
    for N in list(range(9, 13)) * 150 + list(range(13, 41)) * 40:
        cols = np.nonzero(rng.random(N) < rng.random())[0]
        for u in rng.integers(0, N, size=3):
            _check_rank(N, cols, int(u), bool(rng.integers(0, 2)))


def test_the_small_cases_by_hand():
    rowptr, col = case.graphs()["small7"]
    row = lambda u: col[rowptr[u]:rowptr[u + 1]]  # noqa: E731
    want = {2: [0, 1, 3, 4, 5, 6], 3: [1, 2, 4, 5], 4: [0, 1, 2, 3, 5, 6], 5: [6], 6: [0]}
    for u, ids in want.items():
        assert [R.nth_non_neighbour(row(u), u, 7, r, True) for r in range(len(ids))] == ids, u
    assert R.nth_non_neighbour(row(1), 1, 7, 0, False) == 1 and R.nth_non_neighbour(row(4), 4, 7, 4, False) == 4
    assert [R.nth_non_neighbour(row(3), 3, 7, r, False) for r in range(5)] == [1, 2, 3, 4, 5]
    for u in (0, 1):
        assert R.forbidden(row(u), u, True).size == 7, "no candidate"
    neg, full = case.draw_reference("small7-neg64")
    assert full and np.all(neg[0] == -1) and np.all(neg[1] == -1) and np.all(neg[2:] >= 0)
    for u, ids in want.items():
        assert sorted(set(neg[u].tolist())) == ids, ("64 draws meet every r", u)
    neg, full = case.draw_reference("small7-with-self-neg64")
    assert full and np.all(neg[0] == -1) and np.all(neg[1] == 1) and sorted(set(neg[2].tolist())) == [0, 1, 3, 4, 5, 6]
    assert sorted(set(neg[3].tolist())) == [1, 2, 3, 4, 5]
    neg, full = case.draw_reference("tie-row0")
    assert full and np.all(neg[[0, 2]] == -1) and np.all(neg[[1, 3, 4]] >= 0)
    # find_edges: the 49 pairs of small7 against its rows
    pos = case.find_reference("small7-all-49").reshape(7, 7)
    for u in range(7):
        assert np.array_equal(np.nonzero(pos[u] >= 0)[0], row(u)) and np.array_equal(pos[u][pos[u] >= 0], np.arange(rowptr[u], rowptr[u + 1]))
    rp, cc = case.graphs()["cora"]
    assert np.array_equal(case.find_reference("cora-own-pairs"), np.arange(cc.size))
    swapped = case.find_reference("cora-swapped-pairs")
    assert np.all(swapped >= 0) and np.array_equal(swapped[swapped], np.arange(cc.size)), "Cora is symmetric: an involution"
    assert (case.find_reference("cora-random-1000") >= 0).sum() < 20, "mostly absent"
    for name in ("lengths-long-rows", "tie-long-row"):
        p = case.find_reference(name)
        assert (p >= 0).sum() >= p.size // 3 and (p < 0).sum() > 0, name


def test_every_draw_is_a_non_neighbour():
    for name in case.DRAW_NAMES:
        c = case.draw_case(name)
        rowptr, col = case.graphs()[c.graph]
        neg, full = case.draw_reference(name)
        assert neg.shape == (c.src.size, c.num_neg) and neg.dtype == np.int64 and neg.max() < rowptr.size - 1 and neg.min() >= -1
        assert full == (c.graph in ("small7", "tie")), name
        u = np.repeat(c.src, c.num_neg)
        v = neg.reshape(-1)
        drawn = v >= 0
        assert np.all(R.find_edges_ref(rowptr, col, u[drawn], v[drawn]) == -1), name
        if c.exclude_self:
            assert np.all(v[drawn] != u[drawn]), name
        rows_without = ~drawn.reshape(neg.shape).any(1)
        assert np.array_equal(rows_without, ~drawn.reshape(neg.shape).all(1)), "a row draws everywhere or nowhere"
    rep = case.draw_reference("cora-repeated-src")[0]
    assert not np.array_equal(rep[0], rep[1]), "repeats of one source draw their own words"
    a = case.draw_case("cora-hop3-big-seed")
    other = R.negative_edges_ref(*case.graphs()["cora"], a.src, a.num_neg, a.seed, 0, True)[0]
    assert not np.array_equal(other, case.draw_reference("cora-hop3-big-seed")[0]), "the hop is a word of the counter"


def test_the_draw_is_uniform():
    """A row with m = 7 candidates, 70 000 draws of seed 1: every count within 5 sigma of 10 000, sigma = sqrt(10 000 * 6 / 7) = 92.6
    (the largest deviation of these keys is 84).  A layout that reuses a word, or a rank that favours a border, fails this."""
    N, u, cols = 12, 3, np.array([0, 2, 5, 9])
    rowptr = np.array([0, 0, 0, 0, 4] + [4] * 8)
    neg, full = R.negative_edges_ref(rowptr, cols, np.array([u]), 70000, 1, 0, True)
    ids, counts = np.unique(neg, return_counts=True)
    assert not full and ids.tolist() == [1, 4, 6, 7, 8, 10, 11]
    sigma = np.sqrt(10000 * 6 / 7)
    dev = np.abs(counts - 10000).max()
    print("largest deviation", dev, "sigma", sigma)
    assert dev <= 5 * sigma, counts


def test_the_stream_is_free():
    assert R.STREAM_NEG == 6
    from pygat_amd import dropout
    streams = {k: v for k, v in vars(dropout).items() if k.startswith("STREAM_")}
    assert streams["STREAM_NEG"] == 6 and len(streams) >= 6
    assert [k for k, v in streams.items() if v == 6] == ["STREAM_NEG"], "stream 6 is used by nothing else"


def test_the_literal_names_are_the_cases():
    assert list(case.DRAW_NAMES) == case.draw_case_names() and list(case.FIND_NAMES) == case.find_case_names()
    assert set(case.DRAW_INT32_CASES) <= set(case.DRAW_NAMES) and set(case.FIND_INT32_CASES) <= set(case.FIND_NAMES)


def test_the_batch_bookkeeping():
    rowptr, col = case.graphs()["cora"]
    ids = case.link_edge_ids()
    B, K = case.LINK["B"], case.LINK["num_neg"]
    assert ids.size == B and np.unique(ids).size == B - 2
    none, pos, rev = (case.link_reference(e) for e in ("none", "positive", "reverse"))
    b = rev
    assert np.array_equal(b.seeds[b.pos_src], b.u) and np.array_equal(b.seeds[b.pos_dst], b.v) and np.array_equal(b.seeds[b.neg_dst], b.neg)
    assert np.all(np.diff(b.seeds) > 0) and np.all(b.u != b.v) and np.array_equal(col[ids], b.v)
    assert none.excluded.size == 0 and np.array_equal(pos.excluded, np.unique(ids)) and rev.excluded.size == 2 * (B - 2)
    mirror = np.setdiff1d(rev.excluded, pos.excluded)
    row_of = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    assert sorted(zip(row_of[mirror], col[mirror])) == sorted(set(zip(b.v, b.u)))
    assert b.pair_rows.shape == b.pair_cols.shape == b.labels.shape == (B + B * K,)
    assert np.array_equal(b.pair_rows[B:].reshape(B, K), np.repeat(b.pos_src[:, None], K, 1)) and b.labels.sum() == B
