"""tests/subgraph_ref.py against restatements that share nothing with it: the dense A[S][:, S] for the induced subgraph, the
neighbour lists and the pick frequencies for the walk.  No torch, no GPU."""
import numpy as np

import subgraph_case as case
import subgraph_ref as R


def _dense(rowptr, col):
    n = rowptr.size - 1
    A = np.zeros((n, n), dtype=bool)
    A[np.repeat(np.arange(n), np.diff(rowptr)), col] = True
    return A


def test_induced_subgraph_equals_the_dense_restatement_on_cora():
    rowptr, col = case.graphs()["cora"]
    ids, _ = case.cora_set()
    sub = R.induced_subgraph_ref(rowptr, col, ids)
    S = np.unique(ids)
    D = _dense(rowptr, col)[np.ix_(S, S)]
    r, c = np.nonzero(D)                                   # row-major: rows ascending, columns ascending inside a row
    assert sub.n == S.size == 300 and np.array_equal(sub.nodes, S) and sub.nnz == r.size > 300
    assert np.array_equal(sub.edge_rc, np.stack([r, c], 1)) and np.array_equal(sub.col, c)
    assert np.array_equal(sub.rowptr, np.concatenate([[0], np.cumsum(np.bincount(r, minlength=S.size))]))
    assert np.array_equal(np.diff(sub.edge_ids) > 0, np.ones(sub.nnz - 1, dtype=bool)), "positions strictly increasing"
    row_of_pos = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    assert np.array_equal(row_of_pos[sub.edge_ids], S[r]) and np.array_equal(col[sub.edge_ids], S[c])
    assert np.array_equal(sub.nodes[sub.index], ids) and sub.n_empty_rows == 0


def test_only_the_set_counts():
    rowptr, col = case.graphs()["cora"]
    ids, more = case.cora_set()
    assert more.size == 350 and np.unique(more).size == 300 and not np.array_equal(more[:300], ids)
    a, b = R.induced_subgraph_ref(rowptr, col, ids), R.induced_subgraph_ref(rowptr, col, more)
    for name in ("rowptr", "col", "edge_rc", "edge_ids", "nodes"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert b.index.shape == (350,) and np.array_equal(b.nodes[b.index], more)


def test_the_small_cases_by_hand():
    rowptr, col = case.graphs()["relabel"]
    for nodes in ([0, 1], [1, 0], [0, 1, 0]):
        sub = R.induced_subgraph_ref(rowptr, col, np.array(nodes))
        assert sub.rowptr.tolist() == [0, 2, 4] and sub.col.tolist() == [0, 1, 0, 1] and sub.edge_ids.tolist() == [0, 1, 4, 5]
        assert sub.nodes.tolist() == [0, 1] and sub.index.tolist() == nodes
    sub = R.induced_subgraph_ref(rowptr, col, np.array([0, 2, 4, 5]))          # rows 0, 2 and 4 share the neighbour 5
    assert sub.rowptr.tolist() == [0, 2, 4, 6, 7] and sub.col.tolist() == [0, 3, 1, 3, 2, 3, 3]
    lone = R.induced_subgraph_ref(*case.graphs()[case.NO_ENTRY[0]], case.NO_ENTRY[1])
    assert lone.nnz == 0 and lone.n_empty_rows == 1
    for name in ("lengths-long-alone", "lengths-long-and-half"):
        assert case.reference(name).n_empty_rows > 0, "the lengths graph leaves sub-rows empty"
    tie = case.reference("tie-even")
    assert tie.nnz == 65536 + 65535 and tie.rowptr[1] == 65536


def test_every_step_lands_on_a_neighbour():
    for name in ("cora-1000-len9", "cora-hop3-big-seed", "hole"):
        c = case.walk_case(name)
        rowptr, col = case.graphs()[c.graph]
        walks = case.walk_reference(name)
        assert walks.shape == (c.start.size, c.length + 1) and np.array_equal(walks[:, 0], c.start)
        A = _dense(rowptr, col)
        stays = np.diff(rowptr) == 0
        for t in range(1, c.length + 1):
            prev, cur = walks[:, t - 1], walks[:, t]
            assert np.all(np.where(stays[prev], cur == prev, A[prev, cur])), (name, t)
    hole = case.walk_reference("hole")
    assert np.all(hole[hole[:, 0] == 2] == 2) and (hole[:, -1] == 2).sum() > 20, "the row without entries keeps its walkers"


def test_the_pick_is_uniform_and_steps_and_walkers_draw_their_own_words():
    """30 000 walkers on a node of degree 3 at seed 0, hop 0: each neighbour's share at steps 1, 4 and 5 is within 0.01 of 1/3 (the
    largest deviation of these keys is 0.0022).  A counter layout that reuses one word for all steps or all walkers fails this."""
    n_walk, d = 30000, 3
    for t in (1, 4, 5):
        pick = (R.step_keys(0, 0, n_walk, t).astype(np.uint64) * np.uint64(d)) >> np.uint64(32)
        share = np.bincount(pick.astype(np.int64), minlength=d) / n_walk
        assert share.size == d and np.all(np.abs(share - 1 / 3) < 0.01), (t, share)
    # the same through random_walk_ref on the complete graph of four nodes: every node has degree 3 at every step
    col = np.array([1, 2, 3, 0, 2, 3, 0, 1, 3, 0, 1, 2])
    rowptr = np.arange(0, 13, 3)
    walks = R.random_walk_ref(rowptr, col, np.zeros(n_walk, dtype=np.int64), 5, 0, 0)
    picks = []
    for t in (1, 4, 5):
        prev, cur = walks[:, t - 1], walks[:, t]
        pick = cur - (cur > prev)                           # the place of cur in the row of prev (the row skips prev itself)
        assert np.array_equal(col[rowptr[prev] + pick], cur)
        share = np.bincount(pick, minlength=d) / n_walk
        assert np.all(np.abs(share - 1 / 3) < 0.01), (t, share)
        picks.append(pick)
    assert not np.array_equal(picks[0], picks[1]) and not np.array_equal(picks[1], picks[2])


def test_the_literal_names_are_the_cases():
    assert list(case.SUB_NAMES) == case.case_names() and list(case.WALK_NAMES) == case.walk_case_names()


def test_the_stream_is_free():
    assert R.STREAM_WALK == 5
    from pygat_amd.dropout import STREAM_WALK, STREAM_SAMPLE, STREAM_X, STREAM_WH, STREAM_ATT
    assert STREAM_WALK == 5 and STREAM_WALK not in (STREAM_SAMPLE, STREAM_X, STREAM_WH, STREAM_ATT)
