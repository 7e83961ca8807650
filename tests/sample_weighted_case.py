"""The seeded cases of the neighbour sampler weighted by edge, shared by tests/test_sampler_weighted_ref.py (CPU) and
tests/test_gpu_sample_weighted.py, on the graphs of sample_case.graphs().  A case is (name, graph, weights, dst, fanout, seed, hop);
its expected block is sampler_weighted_ref.sample_neighbors_weighted_ref in fp64, computed once per case (reference()).

The kernels order fp32 clocks, the reference fp64 ones.  A case belongs here only if, IN THE REFERENCE ALONE, every row's relative
gap between the last clock kept and the first one dropped is at least MIN_GAP = 1e-4: some 200 x the error of two fp32 clocks (a few
ulps of 6e-8 each), so the set the kernels keep is determined and must equal the reference's entry for entry.
tests/test_sampler_weighted_ref.py asserts the condition for every case; a case that falls below it gets another seed, never another
bound.

Weights ("rand"): default_rng(5).uniform(0.05, 4.0) as float32, 15 % of the entries set to 0.  The other weight tables start from it:
  selfloop   +inf on every entry (i, i) of Cora: the always-keep rule, one per row
  inftie     relabel graph: +inf on three of the four entries of row 0 and on both of row 5 -- more than fanout 2 / as many as it
  exact      lengths graph, fanout 5: rows of every kind (one thread, one wave, one work-group) whose positive entries number exactly
             4, 5 and 6 with zeros in between them
"""
import functools
from collections import namedtuple

import numpy as np

import sample_case as base
import sampler_weighted_ref as W

MIN_GAP = 1e-4
EXACT_FANOUT = 5
# lengths graph: row -> number of positive entries, spread evenly over the row (the rest are zeros).  Rows 3-5 are short (14, 59, 60
# entries) and 17 is the 256-entry row one wave still takes; 14, 18, 19 and 21 go to a work-group (400, 257, 256 off a multiple of 4,
# and 2500 entries)
EXACT_ROWS = {3: 5, 4: 6, 5: 4, 7: 6, 17: 4, 14: 6, 18: 5, 19: 4, 21: 5}
Case = namedtuple("Case", "name graph weights dst fanout seed hop")


@functools.lru_cache(maxsize=None)
def weights(graph, kind="rand"):
    """float32 [nnz], read-only."""
    rowptr, col = base.graphs()[graph]
    rng = np.random.default_rng(5)
    w = rng.uniform(0.05, 4.0, col.size).astype(np.float32)
    w[rng.random(col.size) < 0.15] = 0
    if kind == "selfloop":
        row = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
        w[row == col] = np.inf
    elif kind == "inftie":
        assert graph == "relabel"
        w[rowptr[0]:rowptr[0] + 4] = (np.inf, 1.5, np.inf, np.inf)
        w[rowptr[5]:rowptr[5] + 2] = np.inf
    elif kind == "exact":
        assert graph == "lengths"
        for r, positive in EXACT_ROWS.items():
            b, e = int(rowptr[r]), int(rowptr[r + 1])
            keep = b + (np.arange(positive) * (e - b - 1)) // (positive - 1)          # first and last entry, the others between
            row = np.zeros(e - b, dtype=np.float32)
            row[keep - b] = rng.uniform(0.05, 4.0, positive)
            w[b:e] = row
    elif kind != "rand":
        raise KeyError(kind)
    w.setflags(write=False)
    return w


@functools.lru_cache(maxsize=None)
def cases():
    g = base.graphs()
    out = []
    rows = np.arange(len(base.LENGTHS))
    for fanout in (7, 60, 200, 256, None):
        out.append(Case(f"lengths-f{fanout}", "lengths", "rand", rows, fanout, 99, 0))
    out.append(Case("lengths-f7-hop3-reversed", "lengths", "rand", rows[::-1].copy(), 7, 99, 3))
    out.append(Case("lengths-big-seed", "lengths", "rand", rows, 60, (1 << 62) - 3, 2 ** 32 - 1))
    out.append(Case("lengths-exact-f5", "lengths", "exact", rows, EXACT_FANOUT, 99, 0))
    perm = np.random.default_rng(7).permutation(g["cora"][0].size - 1)
    for fanout in (1, 3, 5):
        out.append(Case(f"cora-300-f{fanout}", "cora", "rand", perm[:300], fanout, 1534, 0))
        out.append(Case(f"cora-selfloop-f{fanout}", "cora", "selfloop", perm[:300], fanout, 1534, 0))
    for name, dst in (("ascending", [0, 1, 2, 3, 4]), ("shuffled", [2, 0, 4, 1, 3]), ("pair", [5, 0])):
        for fanout in (2, None):
            out.append(Case(f"relabel-{name}-f{fanout}", "relabel", "rand", np.array(dst), fanout, 3, 0))
    out.append(Case("relabel-inftie-f2", "relabel", "inftie", np.array([5, 0, 4]), 2, 3, 0))
    return tuple(out)


def case_names():
    return [c.name for c in cases()]


def case(name):
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def reference(name):
    """-> (Block, gaps)"""
    c = case(name)
    rowptr, col = base.graphs()[c.graph]
    return W.sample_neighbors_weighted_ref(rowptr, col, c.dst, c.fanout, weights(c.graph, c.weights), c.seed, c.hop)


TWO_HOP = dict(graph="cora", weights="selfloop", fanouts=(5, 3), seed=4321, n_seeds=64)


def two_hop_seeds():
    n = base.graphs()["cora"][0].size - 1
    return np.random.default_rng(11).permutation(n)[:TWO_HOP["n_seeds"]]


@functools.lru_cache(maxsize=None)
def two_hop_reference():
    """-> (blocks, gaps), outermost hop first"""
    rowptr, col = base.graphs()["cora"]
    return W.sample_blocks_weighted_ref(rowptr, col, two_hop_seeds(), list(TWO_HOP["fanouts"]), weights("cora", TWO_HOP["weights"]),
                                        TWO_HOP["seed"])


# ---- the inclusion-frequency experiment: FREQ_ROWS rows of six entries, every row with the weights FREQ_WEIGHTS, drawn at the hops
# FREQ_HOPS of one seed -- FREQ_ROWS * len(FREQ_HOPS) row draws per fanout.  Nothing here goes through sampler_weighted_ref's clocks.
FREQ_WEIGHTS = (1.0, 2.0, 3.0, 0.0, 4.0, 6.0)
FREQ_ROWS, FREQ_HOPS, FREQ_SEED, FREQ_FANOUTS, FREQ_SIGMAS = 512, tuple(range(8)), 2024, (1, 2, 3), 5.0


def freq_graph():
    """Node r's row: the six columns (r + d) mod FREQ_ROWS, d in (0, 1, 2, 3, 5, 8), ascending."""
    cols = np.sort((np.arange(FREQ_ROWS)[:, None] + np.array([0, 1, 2, 3, 5, 8])[None, :]) % FREQ_ROWS, axis=1)
    return np.arange(FREQ_ROWS + 1, dtype=np.int64) * 6, cols.reshape(-1).astype(np.int64)


def freq_weights():
    return np.tile(np.array(FREQ_WEIGHTS, dtype=np.float32), FREQ_ROWS)


def inclusion_probabilities(w, fanout):
    """Exact probability that successive sampling without replacement (draw entry i with probability w_i over the sum of what is
    left, `fanout` times) includes each entry, by enumeration of the ordered draws.  Finite weights; 0 is never drawn."""
    w = np.asarray(w, dtype=np.float64)
    prob = np.zeros(w.size)

    def walk(left, chosen, p):
        if len(chosen) == fanout or not left:
            for i in chosen:
                prob[i] += p
            return
        total = sum(w[i] for i in left)
        for i in left:
            walk([j for j in left if j != i], chosen + [i], p * w[i] / total)
    walk([i for i in range(w.size) if w[i] > 0], [], 1.0)
    return prob


def check_frequencies(counts, fanout):
    """counts [6]: how often each entry was kept in FREQ_ROWS * len(FREQ_HOPS) row draws at `fanout`.  Every frequency within
    FREQ_SIGMAS binomial standard deviations of the exact probability; the zero-weight entry never.  -> the largest |z|."""
    n = FREQ_ROWS * len(FREQ_HOPS)
    p = inclusion_probabilities(FREQ_WEIGHTS, fanout)
    assert abs(p.sum() - fanout) < 1e-12 and p[3] == 0
    counts = np.asarray(counts, dtype=np.float64)
    assert counts.sum() == n * fanout and counts[3] == 0, counts
    pos = p > 0
    z = (counts[pos] - n * p[pos]) / np.sqrt(n * p[pos] * (1 - p[pos]))
    print(f"fanout {fanout}: frequencies {counts / n}, exact {p}, z {z}")
    assert np.abs(z).max() <= FREQ_SIGMAS, (fanout, z)
    return float(np.abs(z).max())
