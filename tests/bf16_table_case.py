"""Inputs and ground truth of the tests of the bf16 feature table (gat_level(..., table_dtype=torch.bfloat16),
csrc/k16_bf16_forward.hip).  Imported by tests/test_gpu_bf16_table.py.

The contract: the bf16 level is exactly the fp32 level applied to the table Whq = Q(x W), Q = round to nearest even from fp32 to
bf16.  To price the kernel against that statement with the ONE rule of tests/parity.py, the kernel's table and the table formed
here must agree bit for bit, whatever order the projection sums in: the inputs make x W exact in fp32 --
    x integer-valued in [-2, 2],  W = k / 64 with integer k in [-64, 64]  (W_skip likewise),  a = 0.5 N(0, 1) (arbitrary)
-- every product is a multiple of 1/64 below 2^2, every partial sum a multiple of 1/64 below 2^24 / 64.  Both are also exact in
bf16 (8 significant bits), so the split-bf16 product mode of the projection is exact on them too.
The reference level is alpha_grad_case.level_ref fed x' = [Whq of all heads | x] with 0/1 selector matrices as W and [0; W_skip]
as S: x' W'_h = Whq_h and x' S'_h = x W_skip_h exactly, in float64 and in float32 -- "the fp32 level on Whq".
`table` asserts that the case can tell a kernel that never rounds, or rounds ties the wrong way, from a correct one: at least 15 %
of the non-zero table entries change when rounded, at least 5 % of all entries are exact ties (low 16 bits == 0x8000)."""
import numpy as np
import torch

import parity
from alpha_grad_case import level_ref

SLOPE = 0.2


def exact_inputs(N, Fin, H, Fo, seed):
    """-> x [N, Fin], W [H, Fin, F'], a [H, 2F'], W_skip [H, Fin, F'], all float32."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (N, Fin), generator=g).float()
    W = torch.randint(-64, 65, (H, Fin, Fo), generator=g).float() / 64
    S = torch.randint(-64, 65, (H, Fin, Fo), generator=g).float() / 64
    a = (torch.randn(H, 2 * Fo, generator=g) * 0.5).float()
    return x, W, a, S


def table(x, W, check_stats=True):
    """Whq [H, N, F'] as float32 (bf16 values) = Q(x W), formed in float64 and rounded once to fp32 (exact) and once to bf16."""
    wh64 = torch.einsum("nk,hkf->hnf", x.double(), W.double())
    wh32 = wh64.float()
    assert torch.equal(wh32.double(), wh64), "the projection is not exact in fp32: the inputs are not the exact-input case"
    assert torch.equal(torch.einsum("nk,hkf->hnf", x, W), wh32) and \
        torch.equal(torch.einsum("nk,hkf->hnf", x.flip(1), W.flip(1)), wh32), "fp32 sums of the projection depend on their order"
    whq = wh32.bfloat16().float()
    if check_stats:
        nz = wh32 != 0
        rounded = float((whq != wh32)[nz].float().mean())
        ties = float(((wh32.view(torch.int32) & 0xFFFF) == 0x8000).float().mean())
        assert rounded >= 0.15, f"only {rounded:.1%} of the non-zero table entries are rounded: the case cannot see a missing rounding"
        assert ties >= 0.05, f"only {ties:.1%} of the table entries are exact ties: the case cannot see a wrong tie rule"
    return whq


def _restated(x, W, S):
    """x' = [Whq of all heads | x], selectors W' [H, H F' + Fin, F'], S' = [0; W_skip] (or None)."""
    H, Fin, Fo = W.shape
    whq = table(x, W)
    xp = torch.cat([whq[h] for h in range(H)] + [x], 1)
    Wp = torch.zeros(H, H * Fo + Fin, Fo)
    for h in range(H):
        Wp[h, h * Fo:(h + 1) * Fo] = torch.eye(Fo)
    Sp = None if S is None else torch.cat([torch.zeros(H, H * Fo, Fo), S], 1)
    return xp, Wp, Sp


def kink_count(x, rowptr, col, W, a, tau=parity.KINK_TAU):
    """(edge, head) pairs of the fp64 run on Whq whose logit lies in the rounding band of the LeakyReLU kink (alpha_grad_case)."""
    xp, Wp, _ = _restated(x, W, None)
    with torch.no_grad():
        _, _, z, sc = level_ref(xp.double(), rowptr, col, Wp.double(), a.double(), None, SLOPE, True, want_z=True)
    return int(((z.abs() <= tau * sc) & (sc > 0)).sum())


def case(N, Fin, H, Fo, rowptr, col, seed):
    """Exact inputs of the first seed in seed, seed + 1000, ... on whose fp64 run no logit lies in the kink band (the treatment
    of tests/test_gpu_edge_logit.py: parity.close_fwd knows no branch flips, so the cases carry none)."""
    for k in range(32):
        x, W, a, S = exact_inputs(N, Fin, H, Fo, seed + 1000 * k)
        if kink_count(x, rowptr, col, W, a) == 0:
            return x, W, a, S
    raise AssertionError("no seed without a near-kink logit")


def reference(x, rowptr, col, W, a, S, concat):
    """-> (out64, out32): the fp32 level applied to Whq, evaluated in float64 (ground truth) and in float32 (its own precision)."""
    xp, Wp, Sp = _restated(x, W, S)
    with torch.no_grad():
        o64 = level_ref(xp.double(), rowptr, col, Wp.double(), a.double(), None if Sp is None else Sp.double(), SLOPE, concat)[0]
        o32 = level_ref(xp, rowptr, col, Wp, a, Sp, SLOPE, concat)[0]
    return o64, o32


def hub_graph(N=300, seed=3, hub_deg=200, lonely=12):
    """Symmetric pattern with self loops, one hub row of ~hub_deg edges (cut into 2 .. > 32 pieces, by the slot length) and
    `lonely` nodes that keep nothing but their self loop (rows of exactly one edge)."""
    rng = np.random.default_rng(seed)
    M = N - lonely                                    # the last `lonely` nodes take part in no edge
    r = rng.integers(0, M, 2 * M); c = rng.integers(0, M, 2 * M)
    nb = rng.choice(M, size=hub_deg, replace=False)
    r = np.concatenate([r, np.full(hub_deg, 5)]); c = np.concatenate([c, nb])
    rr = np.concatenate([r, c, np.arange(N)]); cc = np.concatenate([c, r, np.arange(N)])
    key = np.unique(rr.astype(np.int64) * N + cc)
    rr, cc = key // N, (key % N).astype(np.int32)
    rowptr = np.concatenate([[0], np.cumsum(np.bincount(rr, minlength=N))]).astype(np.int32)
    deg = np.diff(rowptr)
    assert int((deg == 1).sum()) >= lonely and deg.max() >= hub_deg and ((deg > 4) & (deg <= 8)).any()
    return rowptr, cc
