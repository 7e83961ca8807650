"""The seeded graphs, entry lists and level parameters that the tests of the pattern ops (spmm, edge_softmax, edge_dot and the attention
ops on K19, K20 and K21) and of the levels' attention coefficients share.  CPU only: nothing here imports pygat_amd or touches a
device, so the case modules and the CPU-only *_abi.py tests build their cases from it without loading a GPU test module."""
import numpy as np
import torch

from spmm_case import coo_of

SLOPE = 0.2
SHAPES = [(1, 7), (8, 8), (8, 16), (4, 64), (4, 256), (16, 64)]       # (H, F') of the levels' lane shapes
SID = ["x".join(map(str, s)) for s in SHAPES]
COMPOSE_SEED = 816      # _params seed of the composition case: no logit of its fp64 run lies in the LeakyReLU kink band


def _hub_graph(N=700, seed=3):
    from oracle import gat_oracle as O
    return O.random_symmetric_csr(N, 8, seed, hub=(5, N - 1))


def _asym_graph(N=500, seed=4):
    """Directed edges, a self loop on every other node only, some rows of one edge whose node is gathered elsewhere."""
    rng = np.random.default_rng(seed)
    r = rng.integers(0, N, 6 * N); c = rng.integers(0, N, 6 * N)
    r = np.concatenate([r, np.arange(0, N, 2), np.arange(N)]); c = np.concatenate([c, np.arange(0, N, 2), (np.arange(N) * 7 + 1) % N])
    key = np.unique(r.astype(np.int64) * N + c)
    rr, cc = key // N, key % N
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=N))]).astype(np.int32)
    return rowptr, cc.astype(np.int32)


def _params(N, Fin, H, Fo, seed, v2=False):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Fin, generator=g).float()
    W = (torch.randn(H, (2 if v2 else 1) * Fin, Fo, generator=g) * (1.414 * (2.0 / (Fin + Fo)) ** 0.5)).float()
    a = (torch.randn(H, Fo if v2 else 2 * Fo, generator=g) * 0.5).float()
    S = (torch.randn(H, Fin, Fo, generator=g) * 0.1).float()
    return x, W, a, S


def _coo(csr):
    """(rowptr, col) -> (row, col, N), the entries in CSR order."""
    return coo_of(*csr) + (len(csr[0]) - 1,)


def _rect_coo(seed=12):
    """(300, 500): every third row and every fourth column without entries; unsorted, no repeats."""
    rng = np.random.default_rng(seed)
    rows, cols = np.setdiff1d(np.arange(300), np.arange(0, 300, 3)), np.setdiff1d(np.arange(500), np.arange(0, 500, 4))
    key = np.unique(rng.choice(rows, 4000).astype(np.int64) * 500 + rng.choice(cols, 4000))
    key = key[rng.permutation(len(key))]
    return torch.as_tensor(key // 500), torch.as_tensor(key % 500)


def _repeat_coo(seed=13):
    """The asymmetric pattern, 5 % of its entries duplicated, shuffled -> (row, col, N, [(k, k')] positions of repeated pairs)."""
    row, col, N = _coo(_asym_graph())
    rng = np.random.default_rng(seed)
    E = row.numel()
    dup = rng.choice(E, E // 20, replace=False)
    order = rng.permutation(E + len(dup))
    src = np.concatenate([np.arange(E), dup])[order]              # original entry of every new position
    pos, pairs = {}, []
    for k, s in enumerate(src):
        s = int(s)
        if s in pos:
            pairs.append((pos[s], k))
        pos[s] = k
    assert len(pairs) == len(dup)
    return row[src], col[src], N, torch.as_tensor(pairs)
