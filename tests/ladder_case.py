"""The cut-row "ladder" graph: imported by tests/test_gpu_parity.py (v1 level) and tests/test_gpu_gatv2_sweep.py (GATv2 level)."""
import numpy as np


def _ladder_graph(N=360, seed=5):
    """Symmetric pattern + self loops whose degrees run from 3 to ~180: with 4-edge slots the cut-row list holds chains of 2 ...
    40+ pieces -- packed entries (several rows per wave of the list-driven fix-ups), every remainder of the last wave, and
    `wide` entries (more than 32 pieces: a whole work-group each)."""
    rng = np.random.default_rng(seed)
    r, c = [], []
    for i in range(N):
        d = 170 if i % 45 == 0 else (40 if i % 45 == 7 else 1 + (i * 7) % 6)   # forward neighbours, symmetrised below
        nb = (i + 1 + rng.choice(N - 1, size=d, replace=False)) % N
        r.append(np.full(d, i)); c.append(nb)
    r = np.concatenate(r); c = np.concatenate(c)
    rr = np.concatenate([r, c, np.arange(N)]); cc = np.concatenate([c, r, np.arange(N)])
    key = np.unique(rr.astype(np.int64) * N + cc)
    rr = (key // N).astype(np.int32); cc = (key % N).astype(np.int32)
    rowptr = np.zeros(N + 1, dtype=np.int64); np.add.at(rowptr, rr + 1, 1)
    return np.cumsum(rowptr).astype(np.int32), cc
