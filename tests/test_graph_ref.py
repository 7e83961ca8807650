"""CPU rehearsal of tests/graph_ref.py on the graphs of tests/test_gpu_graph_structures.py: the reference agrees with
hand-worked examples and with itself (brute-force cut list = closed form), and the graphs have what makes the GPU tests
meaningful -- wide chains, both branches of the snapping rule, a self-loop-only tail -- so none of them passes vacuously.
Prints the cut-row and tail statistics of every graph once."""
import numpy as np
import pytest

import graph_ref as R
from graph_cases import SLOT_EDGES, graph

MAIN = ("ladder", "hub", "tail", "cora")


def _stats(name, ts):
    rowptr, _ = graph(name)
    sb = R.slot_borders(rowptr, ts)
    pieces = sorted(t[2] for t in R.cut_rows(rowptr, sb))
    return dict(cut=len(pieces), wide=sum(p > 32 for p in pieces), longest=pieces[-1] if pieces else 0,
                snapped=int((sb != R.uniform_borders(rowptr[-1], ts)).sum()))


# ------------------------------------------------------------------ the reference on hand-worked examples
def test_dense_pattern_by_hand():
    inf, nan = np.inf, np.nan
    a = np.array([[1.0, -1.0, -0.0, nan], [inf, -inf, 1e-40, -1e-40], [0.0, 0.0, 0.0, 0.0], [0.0, 0.0, 0.0, 2.0]], dtype=np.float32)
    rp, col = R.dense_pattern(a, "nonzero")
    assert rp.tolist() == [0, 3, 7, 7, 8] and col.tolist() == [0, 1, 3, 0, 1, 2, 3, 3]
    rp, col = R.dense_pattern(a, "positive")
    assert rp.tolist() == [0, 1, 3, 3, 4] and col.tolist() == [0, 0, 2, 3]
    rp, col = R.dense_pattern(np.array([[1e-60, 0.0], [0.0, -1e-60]]), "nonzero")     # float64: no entry of it is 0
    assert rp.tolist() == [0, 1, 2] and col.tolist() == [0, 1]


def test_slots_by_hand():
    """rows 0: {0,1,2}  1: {0,1}  2: {0,2}  3: {3}, 4-edge slots: border 1 (edge 4) falls inside row 1, whose end 5 is one edge
    away -> snapped to 5; uniform borders cut row 1 in two."""
    rowptr, col = graph("shared_slot")
    assert R.edge_pairs(rowptr, col).tolist() == [[0, 0], [0, 1], [0, 2], [1, 0], [1, 1], [2, 0], [2, 2], [3, 3]]
    sb = R.slot_borders(rowptr, 4)
    assert sb.tolist() == [0, 5, 8]
    assert R.slot_meta(rowptr, 4, sb).tolist() == [[0, 5, 0, 0], [5, 8, 2, 0]]
    assert R.slot_meta(rowptr, 4, None).tolist() == [[0, 4, 0, 2], [4, 8, 1, 1]]
    assert R.cut_rows(rowptr, sb) == set()
    assert R.cut_rows(rowptr, R.uniform_borders(8, 4)) == {(0, 1, 2)} == R.cut_rows_closed_form(rowptr, R.uniform_borders(8, 4))
    # a row of 11 edges at 4-edge slots, ending at nnz: borders 4 and 8 fall inside it, its end is nnz -> never snapped to
    rp = np.array([0, 1, 12])
    sb = R.slot_borders(rp, 4)
    assert sb.tolist() == [0, 4, 8, 12]
    assert R.slot_meta(rp, 4, sb)[:, 3].tolist() == [2, 3, 1]
    assert R.cut_rows(rp, sb) == {(0, 1, 3)} == R.cut_rows_closed_form(rp, sb)
    # the end is ts / 2 = 2 edges away: not "fewer than"; one edge away: snapped
    assert R.slot_borders(np.array([0, 2, 6, 9]), 4).tolist() == [0, 4, 8, 9]
    assert R.slot_borders(np.array([0, 2, 5, 9]), 4).tolist() == [0, 5, 8, 9]


def test_mirror_transpose_degree_order_by_hand():
    rowptr, col = np.array([0, 2, 3, 5]), np.array([0, 2, 1, 0, 1])          # (2, 1) has no mirror
    perm, asym, empty = R.mirror_perm(rowptr, col)
    assert perm.tolist() == [0, 3, 2, 1, 4] and asym and not empty
    rp_t, col_t, perm_t, perm_f = R.transpose(rowptr, col)
    assert rp_t.tolist() == [0, 2, 4, 5] and col_t.tolist() == [0, 2, 1, 2, 0]
    assert perm_t.tolist() == [0, 3, 2, 4, 1] and perm_f.tolist() == [0, 4, 2, 1, 3]
    assert R.mirror_perm(np.array([0, 1, 1]), np.array([0]))[2]
    to_user, to_int, rp2, c2 = R.degree_order(rowptr, col)                   # degrees 2, 1, 2: stable -> nodes 0, 2, 1
    assert to_user.tolist() == [0, 2, 1] and to_int.tolist() == [0, 2, 1]
    assert rp2.tolist() == [0, 2, 4, 5] and c2.tolist() == [0, 1, 0, 2, 2]


# ------------------------------------------------------------------ the graphs
def test_stated_statistics(capsys):
    with capsys.disabled():
        print()
        for name in MAIN:
            rowptr, col = graph(name)
            deg = np.diff(rowptr)
            print(f"{name}: n {len(rowptr) - 1}, {len(col)} edges, degree {deg.min()}..{deg.max()}, {int((deg == 1).sum())} rows of degree 1")
            for ts in SLOT_EDGES:
                s = _stats(name, ts)
                _, _, rp2, c2 = R.degree_order(rowptr, col)
                print(f"  {ts:2d}-edge slots: {s['cut']} cut rows, {s['wide']} over 32 pieces, longest chain {s['longest']}, "
                      f"{s['snapped']} snapped borders, tail {R.self_loop_tail(rp2, c2, ts)}")
    rowptr, col = graph("ladder")
    assert (len(rowptr) - 1, len(col)) == (360, 6086)
    assert _stats("ladder", 4) == dict(cut=360, wide=8, longest=45, snapped=68)
    s = _stats("ladder", 64)
    assert (s["cut"], s["wide"]) == (13, 0)
    rowptr, col = graph("hub")
    assert (len(rowptr) - 1, len(col)) == (1001, 7387) and (len(rowptr) - 1) % 4 == 1
    s = _stats("hub", 4)
    assert (s["cut"], s["wide"], s["longest"]) == (862, 1, 176)
    s = _stats("hub", 8)
    assert (s["wide"], s["longest"]) == (1, 89)
    rowptr, col = graph("tail")
    deg = np.diff(rowptr)
    lone = np.nonzero(deg == 1)[0]
    assert len(lone) == 327 and np.array_equal(col[rowptr[lone]], lone)


@pytest.mark.parametrize("ts", SLOT_EDGES)
@pytest.mark.parametrize("name", MAIN)
def test_slot_preconditions(name, ts):
    rowptr, _ = graph(name)
    nnz = int(rowptr[-1])
    sb = R.slot_borders(rowptr, ts)
    uni = R.uniform_borders(nnz, ts)
    row_of = R.edge_rows(rowptr)
    inside = np.array([rowptr[row_of[p]] != p for p in uni[:-1]])
    moved = sb[:-1] != uni[:-1]
    assert (moved & inside).any() and (~moved & inside).any()        # both branches of the snapping rule
    assert not (moved & ~inside).any()
    size = np.diff(sb)
    assert size.min() > 0 and 2 * size.max() < 3 * ts
    assert sb[0] == 0 and sb[-1] == nnz
    brute = R.cut_rows(rowptr, sb)
    assert brute == R.cut_rows_closed_form(rowptr, sb)
    # the records and the cut list tell one story: a slot's last row continues exactly where a chain passes its end
    meta = R.slot_meta(rowptr, ts, sb)
    passes = np.zeros(len(meta), dtype=int)
    for owner, _, pieces in brute:
        passes[owner:owner + pieces - 1] += 1
    assert np.array_equal(passes, (meta[:, 3] >> 1) & 1)
    assert np.array_equal((meta[1:, 3] & 1), (meta[:-1, 3] >> 1) & 1) and meta[0, 3] & 1 == 0
    # uniform slots: same story with the uniform borders
    metau = R.slot_meta(rowptr, ts, None)
    assert np.array_equal(metau[:, :2], np.stack([uni[:-1], uni[1:]], 1))
    assert int(((metau[:, 3] >> 1) & 1).sum()) == sum(p - 1 for _, _, p in R.cut_rows(rowptr, uni))


@pytest.mark.parametrize("name", ["ladder", "hub", "hub_minus_edge", "asym65"])
def test_mirror_and_transpose_preconditions(name):
    rowptr, col = graph(name)
    perm, asym, empty = R.mirror_perm(rowptr, col)
    rp_t, col_t, perm_t, perm_f = R.transpose(rowptr, col)
    ar = np.arange(len(col))
    assert not empty
    assert np.array_equal(perm_f[perm_t], ar) and np.array_equal(perm_t[perm_f], ar)
    rc = R.edge_pairs(rowptr, col)
    assert np.array_equal(R.edge_pairs(rp_t, col_t), rc[perm_t][:, ::-1])
    if name in ("ladder", "hub"):
        assert not asym and np.array_equal(perm[perm], ar)
        assert np.array_equal(rp_t, rowptr) and np.array_equal(col_t, col) and np.array_equal(perm_t, perm)
    else:
        assert asym and not np.array_equal(rp_t, rowptr)
    if name == "hub_minus_edge":
        assert len(col) == len(graph("hub")[1]) - 1 and int((perm == ar).sum()) == 1001 + 1     # the self loops and (j, 7)


def test_tail_preconditions():
    rowptr, col = graph("tail")
    to_user, to_int, rp2, c2 = R.degree_order(rowptr, col)
    assert np.array_equal(to_int[to_user], np.arange(1000))
    deg2 = np.diff(rp2)
    assert (np.diff(deg2) <= 0).all()
    n1 = int((deg2 > 1).sum())
    assert n1 == 1000 - 327
    seen = set()
    for ts in SLOT_EDGES:
        t = R.self_loop_tail(rp2, c2, ts)
        assert t is not None
        row_first, first_slot = t
        assert n1 <= row_first and 2 * (row_first - n1) < 3 * ts
        assert rp2[row_first] == R.slot_borders(rp2, ts)[first_slot]
        seen.add(row_first > n1)
    assert seen == {True, False}          # a tail that begins at the first self-loop-only row, and one that begins later
    for name in ("ladder", "hub", "identity64", "shared_slot"):
        rp, c = graph(name)
        _, _, rp2, c2 = R.degree_order(rp, c)
        if name == "shared_slot":
            assert np.array_equal(rp2, rp) and np.array_equal(c2, c)
        for ts in SLOT_EDGES:
            assert R.self_loop_tail(rp2, c2, ts) is None, (name, ts)
    assert int((np.diff(graph("ladder")[0]) == 1).sum()) == 0
    assert int((np.diff(graph("hub")[0]) == 1).sum()) == 1        # a lone degree-1 row that begins no slot of its own


def test_wide_split_preconditions():
    """A row of exactly 32 pieces (not wide) beside one of 33 (wide): the cases on the two sides of `pieces > 32`."""
    rowptr, _ = graph("pieces32")
    cut = R.cut_rows(rowptr, R.slot_borders(rowptr, 4))
    assert cut == {(0, 0, 32), (32, 1, 33)} == R.cut_rows_closed_form(rowptr, R.slot_borders(rowptr, 4))
    assert R.cut_list_order(cut) == [(32, 1, 33), (0, 0, 32)]


def test_row_chunk_preconditions():
    """500 chunks are more than the ladder graph has row-starting slots (it has 360 rows), so some targets share a border;
    and the identity pattern has no cut row at any slot length."""
    rowptr, _ = graph("ladder")
    for ts in SLOT_EDGES:
        sb = R.slot_borders(rowptr, ts)
        starts = np.isin(sb[:-1], rowptr[:-1])
        assert 7 <= int(starts.sum()) < 500
    for ts in SLOT_EDGES:
        assert R.cut_rows(graph("identity64")[0], R.slot_borders(graph("identity64")[0], ts)) == set()
