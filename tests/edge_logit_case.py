"""Ground truth of the tests of the per-edge logit term (gat_level(..., edge_logit=u), csrc/k15_edge_logit.hip): a restatement of
alpha_grad_case.level_ref with z = s[src] + t[col] + u[:, h] in front of the LeakyReLU, for all heads of a level, plus the
near-kink census of its logits.  Runs in any dtype on the CPU through torch autograd, with u as a leaf.  Imported by
tests/test_gpu_edge_logit.py."""
import numpy as np
import torch
import torch.nn.functional as F

import parity
from alpha_grad_case import src_of


def level_ref(x, rowptr, col, W, a, S, slope, concat, u, want_z=False):
    """x [N, Fin], W [H, Fin, F'], a [H, 2F'], S [H, Fin, F'] | None, u [E, H] -> (out, alpha [E, H]).
    want_z: also (z [E, H], |s_i| + |t_j| + |u_ij| [E, H]) of the logits in front of the LeakyReLU."""
    N = x.shape[0]
    src, col = src_of(rowptr), torch.as_tensor(np.asarray(col), dtype=torch.int64)
    H, _, Fo = W.shape
    outs, alphas, zs, scales = [], [], [], []
    for h in range(H):
        Wh = x @ W[h]
        ah = a[h].reshape(-1)
        s, t = Wh @ ah[:Fo], Wh @ ah[Fo:]
        z = s[src] + t[col] + u[:, h]
        e = torch.where(z > 0, z, slope * z)
        m = torch.full((N,), -float("inf"), dtype=x.dtype).scatter_reduce(0, src, e.detach(), "amax", include_self=True)
        p = torch.exp(e - m[src])
        Z = torch.zeros(N, dtype=x.dtype).index_add(0, src, p)
        alpha = p / Z[src]
        hp = torch.zeros(N, Fo, dtype=x.dtype).index_add(0, src, alpha[:, None] * Wh[col])
        if S is not None:
            hp = hp + x @ S[h]
        outs.append(F.elu(hp) if concat else hp)
        alphas.append(alpha)
        zs.append(z.detach())
        scales.append((s[src].abs() + t[col].abs() + u[:, h].abs()).detach())
    out = torch.cat(outs, 1) if concat else torch.mean(torch.stack(outs, 1), 1)
    al = torch.stack(alphas, 1)
    return (out, al, torch.stack(zs, 1), torch.stack(scales, 1)) if want_z else (out, al)


def kink_count(x, rowptr, col, W, a, u, slope=0.2, tau=parity.KINK_TAU):
    """(edge, head) pairs of the fp64 run with a logit inside the rounding band of the LeakyReLU kink,
    |z| <= tau (|s_i| + |t_j| + |u_ij|).  A logit whose three terms are all exactly 0 is 0 in every precision: not counted."""
    with torch.no_grad():
        _, _, z, sc = level_ref(x.double(), rowptr, col, W.double(), a.double(), None, slope, True, u.double(), want_z=True)
    return int(((z.abs() <= tau * sc) & (sc > 0)).sum())


def edge_logits(E, H, seed, scale=0.5):
    """u ~ scale * N(0, 1), seeded, float32 [E, H]."""
    return (scale * torch.randn(E, H, generator=torch.Generator().manual_seed(seed))).float()
