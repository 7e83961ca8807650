"""The seeded cases of the neighbour sampler, shared by tests/test_sampler_ref.py (CPU) and tests/test_gpu_sample.py: the smallest
inputs at which each path of csrc/k22_sample.hip can go wrong.  A case is (graph name, dst, fanout, seed, hop); its expected block is
sampler_ref.sample_neighbors_ref, computed once per case (reference()).

The select kernels change path where a row's positions span more than 64 Philox calls (WAVE_QUADS): at most 253 entries at any
alignment, 256 when the row starts at a multiple of 4.  The emit loop of a work-group takes 1024 positions per round.
"""
import functools
import os
from collections import namedtuple

import numpy as np

import sampler_ref as R

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
WAVE_QUADS = 64
Case = namedtuple("Case", "name graph dst fanout seed hop")

# (b), (c): row lengths around the fanouts used on this graph (7, 60, 200) and around the path boundary; the 2-entry row aligns the
# first 256-entry row to a Philox call (64 calls: the wave), the second one starts off a multiple of 4 (65 calls: the work-group)
LENGTHS = (6, 7, 8, 14, 59, 60, 61, 120, 63, 64, 65, 199, 200, 201, 400, 255, 2, 256, 257, 256, 253, 2500)
LENGTHS_N = 3000
TIE_N, TIE_FANOUT = 1 << 17, 20608


def quads(b, e):
    return ((e - 1) >> 2) - (b >> 2) + 1


def _lengths_graph():
    rng = np.random.default_rng(22)
    lens = list(LENGTHS) + [1] * (LENGTHS_N - len(LENGTHS))
    rowptr = np.zeros(LENGTHS_N + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(lens)
    col = np.concatenate([np.sort(rng.choice(LENGTHS_N, size=d, replace=False)) for d in lens])
    return rowptr, col.astype(np.int64)


def _relabel_graph():
    """Rows 0, 2 and 4 share the neighbour 5; 0 and 1 are each other's neighbours; node 3 is in nobody's row (its own included)."""
    rows = {0: [0, 1, 5, 7], 1: [0, 1, 2], 2: [2, 5, 9], 3: [8], 4: [4, 5, 10, 11], 5: [5, 11]}
    n = 12
    lists = [rows.get(i, [i]) for i in range(n)]
    rowptr = np.zeros(n + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(x) for x in lists])
    return rowptr, np.concatenate(lists).astype(np.int64)


def _tie_graph():
    """Row 0 holds all 2^17 columns at positions 0 .. 2^17 - 1; every other row only its self loop."""
    n = TIE_N
    rowptr = np.concatenate([[0], n + np.arange(n, dtype=np.int64)])
    col = np.concatenate([np.arange(n, dtype=np.int64), np.arange(1, n, dtype=np.int64)])
    return rowptr, col


@functools.lru_cache(maxsize=None)
def graphs():
    z = np.load(os.path.join(GOLDEN, "cora_csr.npz"), allow_pickle=False)
    return {"cora": (z["rowptr"].astype(np.int64), z["col"].astype(np.int64)), "lengths": _lengths_graph(), "relabel": _relabel_graph(),
            "tie": _tie_graph()}


@functools.lru_cache(maxsize=None)
def cases():
    g = graphs()
    out = []
    n_cora = g["cora"][0].size - 1
    perm = np.random.default_rng(7).permutation(n_cora)
    for n_dst in (1, 64, 300):                                                   # (a)
        for fanout in (1, 3, 5, None):
            out.append(Case(f"cora-{n_dst}-f{fanout}", "cora", perm[:n_dst], fanout, 1234 + n_dst, 0))
    rows = np.arange(len(LENGTHS))
    for fanout in (7, 60, 200, 256, None):                                       # (b), (c)
        out.append(Case(f"lengths-f{fanout}", "lengths", rows, fanout, 99, 0))
    out.append(Case("lengths-f7-hop3-reversed", "lengths", rows[::-1].copy(), 7, 99, 3))
    out.append(Case("lengths-long-f1000", "lengths", np.array([len(LENGTHS) - 1, 2999, 0]), 1000, 5, 1))
    out.append(Case("lengths-big-seed", "lengths", rows, 60, (1 << 62) - 3, 2 ** 32 - 1))
    for name, dst in (("ascending", [0, 1, 2, 3, 4]), ("descending", [4, 3, 2, 1, 0]), ("shuffled", [2, 0, 4, 1, 3]), ("lone", [3]),
                      ("pair", [5, 0])):                                         # (d)
        for fanout in (2, None):
            out.append(Case(f"relabel-{name}-f{fanout}", "relabel", np.array(dst), fanout, 3, 0))
    out.append(Case("tie", "tie", np.array([0]), TIE_FANOUT, 0, 0))             # (e)
    return tuple(out)


def case_names():
    return [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    rowptr, col = graphs()[c.graph]
    return R.sample_neighbors_ref(rowptr, col, c.dst, c.fanout, c.seed, c.hop)


# (f)
TWO_HOP = dict(graph="cora", fanouts=(5, 3), seed=4321, n_seeds=64)


def two_hop_seeds():
    n = graphs()["cora"][0].size - 1
    return np.random.default_rng(11).permutation(n)[:TWO_HOP["n_seeds"]]


@functools.lru_cache(maxsize=None)
def two_hop_reference():
    rowptr, col = graphs()["cora"]
    return R.sample_blocks_ref(rowptr, col, two_hop_seeds(), list(TWO_HOP["fanouts"]), TWO_HOP["seed"])


@functools.lru_cache(maxsize=None)
def tie_facts():
    """Re-derived from sampler_ref.keys: the pairs of equal keys of row 0 of the tie graph at seed 0, hop 0, and where the lowest pair
    stands.  -> (number of pairs, keys below the lowest pair, earlier position, later position)."""
    k = R.keys(0, 0, np.arange(TIE_N))
    order = np.lexsort((np.arange(TIE_N), k))
    ks = k[order]
    same = np.nonzero(ks[1:] == ks[:-1])[0]
    first = int(same[0])
    assert ks[first] != ks[first + 2], "a pair, not a triple"
    return int(same.size), first, int(order[first]), int(order[first + 1])
