"""The two passes of csrc/k14_alpha_grad.hip at full size: the config 5 graph (pygat_amd.rmat, the generator bench.py uses:
2^20 nodes, 10.7 M edges, rows up to 26 779 edges, 55 % of one), H = 8, F' = 16, seeded tables and a seeded A = dL/d alpha.

Autograd in fp64 over 10.7 M edges x 8 heads is too heavy for a test, so ops.alpha_grad_scores (just the row and the column pass)
is compared with the formulas themselves, formed in numpy head by head (one [E] column at a time keeps fp64 below 1 GB), once in
fp64 and once in fp32:
    c_i = sum_k alpha_ik A_ik,  dz_ij = l_ij alpha_ij (A_ij - c_i),  ds'_i = sum_j dz_ij,  dt'_j = sum_i dz_ij
and ds', dt' are priced by the rule of parity.close_grad, max(1e-5, 4 x |fp32 - fp64|).  Near-kink edges (|z| <= 4e-6 (|s_i| +
|t_j|), the full-size band of parity.close_fullsize_grads) are not dropped from either side: what a branch flip can move,
|alpha_ij (A_ij - c_i)| (1 - slope), is added to the tolerance of the two nodes such an edge touches, and the fp64 run may have at
most parity.KINK_MAX such (edge, head) pairs -- a condition on the input, checked on the CPU for the seed below."""
import numpy as np
import pytest
import torch

import parity

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SLOPE, TAU, SEED = 0.2, 4e-6, 1


def tables(rowptr, col, H, seed):
    """Seeded node tables s, t [N, H] and A [E, H] (float32), and the forward's m, Z formed from them in fp32."""
    rng = np.random.default_rng(seed)
    N, E = len(rowptr) - 1, len(col)
    s = rng.standard_normal((N, H)).astype(np.float32)
    t = rng.standard_normal((N, H)).astype(np.float32)
    A = rng.standard_normal((E, H)).astype(np.float32)
    src = np.repeat(np.arange(N), np.diff(rowptr))
    starts = rowptr[:-1].astype(np.int64)
    m, Z = np.empty((N, H), np.float32), np.empty((N, H), np.float32)
    for h in range(H):
        z = s[src, h] + t[col, h]
        e = np.where(z > 0, z, np.float32(SLOPE) * z)
        m[:, h] = np.maximum.reduceat(e, starts)
        Z[:, h] = np.add.reduceat(np.exp(e - m[src, h]), starts)
    return s, t, A, m, Z, src


def formulas(rowptr, col, src, s, t, A, dtype):
    """-> ds', dt' [N, H], the flip bound per node [N, H] x 2 (rows, columns) and the number of near-kink pairs."""
    N, H = s.shape
    starts = rowptr[:-1].astype(np.int64)
    single = (np.diff(rowptr) == 1)[src]
    ds, dt = np.zeros((N, H), dtype), np.zeros((N, H), dtype)
    kb_s, kb_t, near = np.zeros((N, H)), np.zeros((N, H)), 0
    sl = dtype(SLOPE)
    for h in range(H):
        si, tj = s[src, h].astype(dtype), t[col, h].astype(dtype)
        z = si + tj
        e = np.where(z > 0, z, sl * z)
        m = np.maximum.reduceat(e, starts)
        p = np.exp(e - m[src])
        al = p / np.add.reduceat(p, starts)[src]
        a = A[:, h].astype(dtype)
        c = np.add.reduceat(al * a, starts)
        dz = np.where(z > 0, dtype(1), sl) * al * (a - c[src])
        dz[single] = 0                                     # alpha = 1, a constant
        ds[:, h] = np.add.reduceat(dz, starts)
        dt[:, h] = np.bincount(col, weights=dz, minlength=N)
        k = np.nonzero((np.abs(z) <= TAU * (np.abs(si) + np.abs(tj))))[0]
        near += k.size
        move = np.abs(al[k] * (a[k] - c[src[k]])) * (1 - SLOPE)
        np.add.at(kb_s[:, h], src[k], move)
        np.add.at(kb_t[:, h], col[k], move)
    return ds, dt, kb_s, kb_t, near


def _price(got, r64, r32, kb, what):
    own = float(np.maximum(np.abs(r32.astype(np.float64) - r64) - kb, 0).max())
    tol = max(parity.ATOL, 4.0 * own)
    err = np.abs(got.astype(np.float64) - r64)
    worst = float(np.maximum(err - kb, 0).max())
    print(f"{what}: max err beyond the flip bound {worst:.3e}, tolerance {tol:.3e} (fp32 formulas' own error {own:.3e})")
    assert np.isfinite(got).all() and worst <= tol, (what, worst, tol)


def test_fullsize_config5_scores():
    import pygat_amd as pg
    from pygat_amd import ops
    from pygat_amd.rmat import rmat_csr_numpy
    H, Fo = 8, 16
    rowptr, col = rmat_csr_numpy(20, 5_000_000, seed=1)
    assert (np.diff(rowptr) > 0).all()
    col64 = col.astype(np.int64)
    s, t, A, m, Z, src = tables(rowptr, col64, H, SEED)
    d64 = formulas(rowptr, col64, src, s, t, A, np.float64)
    assert d64[4] <= parity.KINK_MAX, f"{d64[4]} near-kink (edge, head) pairs: choose another seed"
    d32 = formulas(rowptr, col64, src, s, t, A, np.float32)
    graph = pg.CSRGraph(torch.from_numpy(rowptr).to(DEV), torch.from_numpy(col).to(DEV))
    dev = lambda v: torch.from_numpy(v).to(DEV)     # noqa: E731
    runs = [ops.alpha_grad_scores(graph, dev(s), dev(t), dev(m), dev(Z), dev(A), SLOPE, Fo) for _ in range(2)]
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])       # fixed summation order
    _price(runs[0][0].cpu().numpy(), d64[0], d32[0], d64[2], "ds'")
    _price(runs[0][1].cpu().numpy(), d64[1], d32[1], d64[3], "dt'")
