"""The seeded cases of induced_subgraph and random_walk, shared by tests/test_subgraph_ref.py (CPU) and tests/test_gpu_subgraph.py: the
smallest inputs at which each path of csrc/k23_subgraph.hip can go wrong.  A subgraph case is (name, graph, nodes); a walk case is
(name, graph, start, length, seed, hop); the expected result is subgraph_ref's, computed once per case (reference(), walk_reference()).

The count and fill kernels change path by the row's length in the GRAPH: at most 64 entries go to a thread (THREAD_ROW), at most 256 to
a wave in rounds of 64 (WAVE_ROW), longer rows to a work-group in rounds of 1024 positions (BLOCK_ROUND).  sample_case's "lengths"
graph has rows of 6 .. 65, 199 .. 257 and 2500 entries (one below, at and one above both borders; 2500 = two whole rounds and a part)
and one random column in every other row, so it is asymmetric and sub-rows come out empty; its "tie" graph has a row of 2^17 = 128
whole rounds.  The walk draws one Philox call per four steps: lengths 1, 4, 5 and 9 end before, at and after a call's border (t = 3
| 4, t = 7 | 8).
"""
import functools
from collections import namedtuple

import numpy as np

import sample_case
import subgraph_ref as R

THREAD_ROW, WAVE_ROW, BLOCK_ROUND = 64, 256, 1024
SubCase = namedtuple("SubCase", "name graph nodes")
WalkCase = namedtuple("WalkCase", "name graph start length seed hop")
BIG_SEED = (1 << 62) - 3
N_LONG = len(sample_case.LENGTHS)          # the rows of the "lengths" graph that are longer than one entry


def _hole_graph():
    """Five nodes; row 2 holds no entry (a CSRGraph only with validate=False): a walker that starts there, or arrives, stays."""
    lists = [[0, 1, 2], [0, 1], [], [2, 3], [2, 4]]
    rowptr = np.zeros(6, dtype=np.int64)
    rowptr[1:] = np.cumsum([len(x) for x in lists])
    return rowptr, np.concatenate([np.asarray(x, dtype=np.int64) for x in lists])


@functools.lru_cache(maxsize=None)
def graphs():
    return dict(sample_case.graphs(), hole=_hole_graph())


def cora_set():
    """300 seeded ids of Cora in shuffled order, and the same with 50 of them repeated and shuffled again."""
    n = graphs()["cora"][0].size - 1
    rng = np.random.default_rng(23)
    ids = rng.permutation(n)[:300]
    more = np.concatenate([ids, rng.choice(ids, size=50, replace=False)])
    return ids, rng.permutation(more)


@functools.lru_cache(maxsize=None)
def cases():
    g = graphs()
    out = []
    n_cora = g["cora"][0].size - 1
    perm = np.random.default_rng(7).permutation(n_cora)
    for n_in in (1, 64, 300, n_cora):
        out.append(SubCase(f"cora-{n_in}", "cora", perm[:n_in]))
    out.append(SubCase("cora-300-plus-50-repeats", "cora", cora_set()[1]))
    out.append(SubCase("cora-whole-range", "cora", np.arange(n_cora)))
    n_len = g["lengths"][0].size - 1
    rest = np.arange(N_LONG, n_len)
    half = np.random.default_rng(5).permutation(rest)[:rest.size // 2]
    out.append(SubCase("lengths-all", "lengths", np.arange(n_len)))
    out.append(SubCase("lengths-long-and-half", "lengths", np.concatenate([half, np.arange(N_LONG)])))
    out.append(SubCase("lengths-long-alone", "lengths", np.arange(N_LONG)))
    for name, nodes in (("01", [0, 1]), ("10", [1, 0]), ("010", [0, 1, 0]), ("0245", [0, 2, 4, 5])):
        out.append(SubCase(f"relabel-{name}", "relabel", np.array(nodes)))
    out.append(SubCase("tie-even", "tie", np.arange(0, sample_case.TIE_N, 2)))
    return tuple(out)


INT32_CASES = ("cora-64", "relabel-0245")         # the cases the GPU test passes as int32
NO_ENTRY = ("relabel", np.array([3]))             # row 3 of the relabel graph holds only column 8: a ValueError


# the names as literals: a test module parametrises over them without building a case while tests are collected
SUB_NAMES = ("cora-1", "cora-64", "cora-300", "cora-2708", "cora-300-plus-50-repeats", "cora-whole-range", "lengths-all",
             "lengths-long-and-half", "lengths-long-alone", "relabel-01", "relabel-10", "relabel-010", "relabel-0245", "tie-even")
WALK_NAMES = tuple(f"cora-{n}-len{t}" for n in (1, 64, 1000) for t in (1, 4, 5, 9)) + (
    "cora-hop3-big-seed", "cora-repeated-starts", "tie-4096-at-0", "hole")


def case_names():
    return [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    c = case(name)
    rowptr, col = graphs()[c.graph]
    return R.induced_subgraph_ref(rowptr, col, c.nodes)


@functools.lru_cache(maxsize=None)
def walk_cases():
    g = graphs()
    n_cora = g["cora"][0].size - 1
    rng = np.random.default_rng(31)
    out = []
    for n_walk in (1, 64, 1000):
        for length in (1, 4, 5, 9):
            out.append(WalkCase(f"cora-{n_walk}-len{length}", "cora", rng.integers(0, n_cora, size=n_walk), length, 77 + n_walk + length, 0))
    out.append(WalkCase("cora-hop3-big-seed", "cora", rng.integers(0, n_cora, size=500), 9, BIG_SEED, 3))
    out.append(WalkCase("cora-repeated-starts", "cora", np.repeat(rng.integers(0, n_cora, size=8), 40), 5, 9, 0))
    out.append(WalkCase("tie-4096-at-0", "tie", np.zeros(4096, dtype=np.int64), 2, 0, 0))
    out.append(WalkCase("hole", "hole", np.tile(np.arange(5), 20), 6, 4, 1))
    return tuple(out)


WALK_INT32_CASES = ("cora-64-len5", "cora-hop3-big-seed")


def walk_case_names():
    return [c.name for c in walk_cases()]


def walk_case(name):
    return next(c for c in walk_cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def walk_reference(name):
    c = walk_case(name)
    rowptr, col = graphs()[c.graph]
    return R.random_walk_ref(rowptr, col, c.start, c.length, c.seed, c.hop)
