"""Plain NumPy reference of the integer structures every attention kernel trusts: the CSR of a dense adjacency, the (row, col)
edge pairs, the mirror permutation, the transpose, the row-snapped slot borders, the 16-byte slot records, the cut-row list,
the degree order and the self-loop-only tail.  No torch, no GPU; loops where a loop is the clearest statement.  Written from
the documented meaning of each structure (pygat_amd/graph.py's docstrings, csrc/k0_graph.hip's comments), not from their code:
tests/test_graph_ref.py rehearses it on the CPU, tests/test_gpu_graph_structures.py compares the GPU structures with it bit
for bit.

A pattern is (rowptr [n + 1], col [nnz]) with the columns of a row ascending.  Edge k is the k-th entry of `col`; a slot is
a range of consecutive edges [sb[s], sb[s + 1])."""
import numpy as np


def dense_pattern(adj, mode="nonzero"):
    """(rowptr, col) of `adj != 0` ("nonzero") or `adj > 0` ("positive"), row-major.  Comparisons are IEEE ones in adj's own
    dtype: -0.0 is no entry, a subnormal is one, NaN is one under "nonzero" and none under "positive"."""
    adj = np.asarray(adj)
    assert adj.ndim == 2 and adj.shape[0] == adj.shape[1] and mode in ("nonzero", "positive")
    rowptr, col = [0], []
    for i in range(adj.shape[0]):
        for j in range(adj.shape[1]):
            v = adj[i, j]
            if (v > 0) if mode == "positive" else (v != 0):
                col.append(j)
        rowptr.append(len(col))
    return np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)


def edge_rows(rowptr):
    """Row of every edge."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    out = np.empty(int(rowptr[-1]), dtype=np.int64)
    for r in range(len(rowptr) - 1):
        out[rowptr[r]:rowptr[r + 1]] = r
    return out


def edge_pairs(rowptr, col):
    """[nnz, 2]: (row, col) of every edge."""
    return np.stack([edge_rows(rowptr), np.asarray(col, dtype=np.int64)], 1)


def mirror_perm(rowptr, col):
    """-> (perm, asymmetric, empty_row): perm[k] = position of edge (j, i) for edge k = (i, j); where (j, i) is no edge,
    perm[k] = k and `asymmetric` is set.  `empty_row`: some row has no edge."""
    rc = edge_pairs(rowptr, col)
    where = {(int(i), int(j)): k for k, (i, j) in enumerate(rc)}
    perm = np.arange(len(rc), dtype=np.int64)
    asym = False
    for k, (i, j) in enumerate(rc):
        m = where.get((int(j), int(i)))
        if m is None:
            asym = True
        else:
            perm[k] = m
    return perm, asym, bool((np.diff(np.asarray(rowptr, dtype=np.int64)) == 0).any())


def transpose(rowptr, col):
    """-> (rowptr_t, col_t, perm_t, perm_f): the pattern of the transpose (row j of it lists the i with an edge (i, j),
    ascending); perm_t[q] = forward position of transposed entry q, perm_f its inverse."""
    n = len(rowptr) - 1
    rc = edge_pairs(rowptr, col)
    into = [[] for _ in range(n)]
    for k, (i, j) in enumerate(rc):          # k ascending = i ascending inside every column list
        into[j].append(k)
    rowptr_t, col_t, perm_t = [0], [], []
    for j in range(n):
        for k in into[j]:
            col_t.append(rc[k, 0])
            perm_t.append(k)
        rowptr_t.append(len(col_t))
    perm_t = np.asarray(perm_t, dtype=np.int64)
    perm_f = np.empty_like(perm_t)
    for q, k in enumerate(perm_t):
        perm_f[k] = q
    return np.asarray(rowptr_t, dtype=np.int64), np.asarray(col_t, dtype=np.int64), perm_t, perm_f


def n_slots(nnz, ts):
    return -(-int(nnz) // ts)


def slot_borders(rowptr, ts):
    """[nslots + 1] row-snapped borders: border k is k * ts, moved to the end of the row it falls inside (not: begins) when
    that end is fewer than ts / 2 edges away and is not nnz; sb[nslots] = nnz."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nnz = int(rowptr[-1])
    row_of = edge_rows(rowptr)
    sb = []
    for k in range(n_slots(nnz, ts)):
        pos = k * ts
        r = row_of[pos]
        if rowptr[r] != pos:
            end = int(rowptr[r + 1])
            if 2 * (end - pos) < ts and end != nnz:
                pos = end
        sb.append(pos)
    sb.append(nnz)
    return np.asarray(sb, dtype=np.int64)


def uniform_borders(nnz, ts):
    return np.asarray([min(k * ts, int(nnz)) for k in range(n_slots(nnz, ts) + 1)], dtype=np.int64)


def slot_meta(rowptr, ts, sb=None):
    """[nslots, 4]: (first edge, end edge, first row, flags) of every slot; sb = None: uniform slots of ts edges.
    flags bit 0: the slot's first row began in an earlier slot; bit 1: its last row continues in a later one."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    nnz = int(rowptr[-1])
    if sb is None:
        sb = uniform_borders(nnz, ts)
    row_of = edge_rows(rowptr)
    out = []
    for s in range(n_slots(nnz, ts)):
        e0, e1 = int(sb[s]), int(sb[s + 1])
        rf, rl = row_of[e0], row_of[e1 - 1]
        out.append((e0, e1, rf, (1 if rowptr[rf] < e0 else 0) | (2 if rowptr[rl + 1] > e1 else 0)))
    return np.asarray(out, dtype=np.int64).reshape(-1, 4)


def edge_slots(sb):
    """Slot of every edge."""
    out = np.empty(int(sb[-1]), dtype=np.int64)
    for s in range(len(sb) - 1):
        out[sb[s]:sb[s + 1]] = s
    return out


def cut_rows(rowptr, sb):
    """Brute force: the set of (owner slot, row, pieces) of every row whose edges lie in more than one slot; the owner is the
    slot of its first edge, `pieces` the number of slots it touches."""
    rowptr = np.asarray(rowptr, dtype=np.int64)
    slot_of = edge_slots(sb)
    out = set()
    for r in range(len(rowptr) - 1):
        touched = sorted(set(slot_of[rowptr[r]:rowptr[r + 1]].tolist()))
        if len(touched) > 1:
            out.add((touched[0], r, len(touched)))
    return out


def cut_rows_closed_form(rowptr, sb):
    """The same set from the slot ends: the last row of slot k is cut and owned by k when it ends beyond the slot
    (row_end > e1) and begins inside it (rowptr[r] >= e0); pieces from a search of its last edge among the borders."""
    rowptr, sb = np.asarray(rowptr, dtype=np.int64), np.asarray(sb, dtype=np.int64)
    row_of = edge_rows(rowptr)
    out = set()
    for k in range(len(sb) - 1):
        e0, e1 = sb[k], sb[k + 1]
        r = row_of[e1 - 1]
        if rowptr[r + 1] > e1 and rowptr[r] >= e0:
            k_end = int(np.searchsorted(sb, rowptr[r + 1] - 1, side="right")) - 1
            out.add((k, int(r), k_end - k + 1))
    return out


def cut_list_order(cut):
    """The order the cut list is kept in: pieces descending, owner slot ascending inside a piece count."""
    return sorted(cut, key=lambda t: (-t[2], t[0]))


def degree_order(rowptr, col):
    """-> (to_user, to_internal, rowptr2, col2): nodes renumbered by descending degree, the old order kept inside a degree;
    internal node p is node to_user[p]; the columns of every renumbered row ascending again."""
    rowptr, col = np.asarray(rowptr, dtype=np.int64), np.asarray(col, dtype=np.int64)
    n = len(rowptr) - 1
    deg = np.diff(rowptr)
    to_user = np.asarray(sorted(range(n), key=lambda u: -deg[u]), dtype=np.int64)       # sorted() is stable
    to_internal = np.empty(n, dtype=np.int64)
    for p, u in enumerate(to_user):
        to_internal[u] = p
    rowptr2, col2 = [0], []
    for u in to_user:
        col2.extend(sorted(to_internal[col[rowptr[u]:rowptr[u + 1]]].tolist()))
        rowptr2.append(len(col2))
    return to_user, to_internal, np.asarray(rowptr2, dtype=np.int64), np.asarray(col2, dtype=np.int64)


def self_loop_tail(rowptr2, col2, ts):
    """For a degree-ordered pattern: (row_first, first_slot) -- rows [row_first, n) hold only their self loop and fill exactly
    the slots [first_slot, nslots) -- or None: no row of degree 1, a degree-1 row that is not a self loop, no slot that holds
    such rows alone (the tail begins no slot of its own), or no slot in front of them (an empty prefix)."""
    rowptr2, col2 = np.asarray(rowptr2, dtype=np.int64), np.asarray(col2, dtype=np.int64)
    n = len(rowptr2) - 1
    deg = np.diff(rowptr2)
    n1 = int((deg > 1).sum())                 # descending degree: rows [n1, n) are the candidates
    if n1 == n:
        return None
    for r in range(n1, n):
        if deg[r] != 1 or col2[rowptr2[r]] != r:
            return None
    sb = slot_borders(rowptr2, ts)
    row_of, slot_of = edge_rows(rowptr2), edge_slots(sb)
    pure = [s for s in range(len(sb) - 1) if row_of[slot_of == s].min() >= n1]       # slots of candidate rows only
    if not pure or pure[0] == 0:
        return None
    first_slot = pure[0]
    assert pure == list(range(first_slot, len(sb) - 1))
    return int(row_of[sb[first_slot]]), first_slot
