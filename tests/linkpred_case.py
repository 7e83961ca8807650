"""The seeded cases of find_edges and negative_edges, shared by tests/test_linkpred_ref.py (CPU) and tests/test_gpu_linkpred.py: the
smallest inputs at which each path of csrc/k24_linkpred.hip can go wrong.  A draw case is (name, graph, src, num_neg, seed, hop,
exclude_self); a find case is (name, graph, row, col); the expected result is linkpred_ref's, computed once per case (draw_reference(),
find_reference()).  Every draw case is run with allow_full=True: small7 and tie hold rows without a candidate, whose draws are -1.

The graphs are subgraph_case's plus small7 (a CSRGraph only with validate=False: row 4 is empty), whose seven rows are the borders of
the rank search:
    0  {0..6}            a full row: -1
    1  {0,2,3,4,5,6}     the only candidate is the node itself: full under exclude_self, the single answer 1 without it
    2  {2}               a self loop alone
    3  {0,6}             both borders taken, the node itself absent and merged in
    4  {}                an empty row
    5  {0,1,2,3,4}       the node itself merged in at the end, the only candidate is 6
    6  {1..6}            the only candidate is 0
A draw spends one Philox word of a call that serves four consecutive flat draws: num_neg = 1, 4, 5 and 64 end before, at and after a
call's border, and 64 draws of a row with at most 6 candidates meet every r.  The "lengths" graph has rows of 6 .. 65, 199 .. 257 and
2500 entries (the searches' depths 3 .. 12), the "tie" graph a row of 2^17 (17 steps of the search for the node itself, then full).
"""
import functools
from collections import namedtuple

import numpy as np

import linkpred_ref as R
import sample_case
import subgraph_case

DrawCase = namedtuple("DrawCase", "name graph src num_neg seed hop exclude_self")
FindCase = namedtuple("FindCase", "name graph row col")
BIG_SEED = (1 << 62) - 3
SMALL7 = ([0, 1, 2, 3, 4, 5, 6], [0, 2, 3, 4, 5, 6], [2], [0, 6], [], [0, 1, 2, 3, 4], [1, 2, 3, 4, 5, 6])
N_LONG = len(sample_case.LENGTHS)


def _small7_graph():
    rowptr = np.zeros(8, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(x) for x in SMALL7])
    return rowptr, np.concatenate([np.asarray(x, dtype=np.int64) for x in SMALL7])


@functools.lru_cache(maxsize=None)
def graphs():
    return dict(subgraph_case.graphs(), small7=_small7_graph())


UNVALIDATED = ("small7", "hole")          # graphs with a row without entries: a CSRGraph only with validate=False


@functools.lru_cache(maxsize=None)
def draw_cases():
    g = graphs()
    n_cora = g["cora"][0].size - 1
    rng = np.random.default_rng(24)
    out = []
    for num_neg in (1, 4, 5, 64):
        out.append(DrawCase(f"small7-neg{num_neg}", "small7", np.arange(7), num_neg, 11 + num_neg, 0, True))
    out.append(DrawCase("small7-with-self-neg64", "small7", np.arange(7), 64, 3, 0, False))
    for n_src in (1, 64, 1000):
        for num_neg in (1, 5):
            out.append(DrawCase(f"cora-{n_src}-neg{num_neg}", "cora", rng.integers(0, n_cora, size=n_src), num_neg, 100 + n_src + num_neg, 0,
                                True))
    out.append(DrawCase("lengths-every-row", "lengths", np.arange(g["lengths"][0].size - 1), 3, 5, 0, True))
    out.append(DrawCase("lengths-with-self", "lengths", np.arange(N_LONG), 5, 6, 1, False))
    out.append(DrawCase("tie-row0", "tie", np.array([0, 5, 0, 70000, sample_case.TIE_N - 1]), 5, 0, 0, True))
    out.append(DrawCase("cora-hop3-big-seed", "cora", rng.integers(0, n_cora, size=500), 5, BIG_SEED, 3, True))
    out.append(DrawCase("cora-repeated-src", "cora", np.repeat(rng.integers(0, n_cora, size=8), 40), 3, 9, 0, True))
    return tuple(out)


DRAW_INT32_CASES = ("cora-64-neg5", "small7-neg5")
DRAW_NAMES = ("small7-neg1", "small7-neg4", "small7-neg5", "small7-neg64", "small7-with-self-neg64", "cora-1-neg1", "cora-1-neg5",
              "cora-64-neg1", "cora-64-neg5", "cora-1000-neg1", "cora-1000-neg5", "lengths-every-row", "lengths-with-self", "tie-row0",
              "cora-hop3-big-seed", "cora-repeated-src")


def _row_of(rowptr):
    return np.repeat(np.arange(rowptr.size - 1, dtype=np.int64), np.diff(rowptr))


def _long_row_pairs(rowptr, col, rows):
    """For every row of `rows`: its first, last and middle column, and the ids one below and one above each (inside [0, N))."""
    N = rowptr.size - 1
    r_out, c_out = [], []
    for r in rows:
        b, e = rowptr[r], rowptr[r + 1]
        for c in (col[b], col[e - 1], col[(b + e) // 2]):
            for q in (c - 1, c, c + 1):
                if 0 <= q < N:
                    r_out.append(r)
                    c_out.append(q)
    return np.asarray(r_out, dtype=np.int64), np.asarray(c_out, dtype=np.int64)


@functools.lru_cache(maxsize=None)
def find_cases():
    g = graphs()
    rowptr, col = g["cora"]
    n_cora = rowptr.size - 1
    rng = np.random.default_rng(42)
    out = [FindCase("cora-own-pairs", "cora", _row_of(rowptr), col), FindCase("cora-swapped-pairs", "cora", col, _row_of(rowptr))]
    for n in (1, 64, 1000):
        out.append(FindCase(f"cora-random-{n}", "cora", rng.integers(0, n_cora, size=n), rng.integers(0, n_cora, size=n)))
    ii, jj = np.meshgrid(np.arange(7), np.arange(7), indexing="ij")
    out.append(FindCase("small7-all-49", "small7", ii.reshape(-1), jj.reshape(-1)))
    out.append(FindCase("lengths-long-rows", "lengths", *_long_row_pairs(*g["lengths"], np.arange(N_LONG))))
    out.append(FindCase("tie-long-row", "tie", *_long_row_pairs(*g["tie"], [0, 1, sample_case.TIE_N - 1])))
    return tuple(out)


FIND_INT32_CASES = ("cora-random-64", "small7-all-49")
FIND_NAMES = ("cora-own-pairs", "cora-swapped-pairs", "cora-random-1", "cora-random-64", "cora-random-1000", "small7-all-49",
              "lengths-long-rows", "tie-long-row")


def draw_case_names():
    return [c.name for c in draw_cases()]


def find_case_names():
    return [c.name for c in find_cases()]


def draw_case(name):
    return next(c for c in draw_cases() if c.name == name)


def find_case(name):
    return next(c for c in find_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def draw_reference(name):
    """-> (neg [n_src, num_neg], full)"""
    c = draw_case(name)
    rowptr, col = graphs()[c.graph]
    return R.negative_edges_ref(rowptr, col, c.src, c.num_neg, c.seed, c.hop, c.exclude_self)


@functools.lru_cache(maxsize=None)
def find_reference(name):
    c = find_case(name)
    rowptr, col = graphs()[c.graph]
    return R.find_edges_ref(rowptr, col, c.row, c.col)


# link_batch on Cora: 64 positive edges that are no self loops, two of them repeated
LINK = dict(graph="cora", B=64, num_neg=5, seed=2024)


@functools.lru_cache(maxsize=None)
def link_edge_ids():
    rowptr, col = graphs()["cora"]
    off = np.nonzero(_row_of(rowptr) != col)[0]
    ids = np.random.default_rng(64).permutation(off)[:LINK["B"]]
    ids[-2:] = ids[:2]
    return ids


@functools.lru_cache(maxsize=None)
def link_reference(exclude):
    rowptr, col = graphs()["cora"]
    return R.link_batch_ref(rowptr, col, link_edge_ids(), LINK["num_neg"], LINK["seed"], exclude)
