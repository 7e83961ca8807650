"""Ground truth of the tests of differentiable attention coefficients (return_attention="grad", csrc/k14_alpha_grad.hip):
a restatement of oracle.sparse_head_forward (reference layers.py:125-173) that returns (out, alpha) with alpha kept in the
autograd graph, for all heads of a level, plus the near-kink census of its logits.  Imported by tests/test_gpu_attention_grad.py."""
import numpy as np
import torch
import torch.nn.functional as F

import parity


def src_of(rowptr):
    rp = torch.as_tensor(np.asarray(rowptr), dtype=torch.int64)
    return torch.repeat_interleave(torch.arange(rp.numel() - 1), rp[1:] - rp[:-1])


def level_ref(x, rowptr, col, W, a, S, slope, concat, mask_x=None, mask_wh=None, mask_att=None, want_z=False):
    """x [N, Fin], W [H, Fin, F'], a [H, 2F'], S [H, Fin, F'] | None -> (out, alpha [E, H]); masks as dropout.draw_masks gives
    them (x [H, N, Fin], wh [H, N, F'], att [E, H]).  alpha is taken before the attention mask (layers.py:150-153).
    want_z: also (z [E, H], |s_i| + |t_j| [E, H]) of the logits in front of the LeakyReLU."""
    N = x.shape[0]
    src, col = src_of(rowptr), torch.as_tensor(np.asarray(col), dtype=torch.int64)
    H, _, Fo = W.shape
    outs, alphas, zs, scales = [], [], [], []
    for h in range(H):
        xh = x if mask_x is None else x * mask_x[h].to(x.dtype)
        Wh = xh @ W[h]
        if mask_wh is not None:
            Wh = Wh * mask_wh[h].to(x.dtype)
        ah = a[h].reshape(-1)
        s, t = Wh @ ah[:Fo], Wh @ ah[Fo:]
        z = s[src] + t[col]
        e = torch.where(z > 0, z, slope * z)
        m = torch.full((N,), -float("inf"), dtype=x.dtype).scatter_reduce(0, src, e.detach(), "amax", include_self=True)
        p = torch.exp(e - m[src])
        Z = torch.zeros(N, dtype=x.dtype).index_add(0, src, p)
        alpha = p / Z[src]
        w = alpha if mask_att is None else alpha * mask_att[:, h].to(x.dtype)
        hp = torch.zeros(N, Fo, dtype=x.dtype).index_add(0, src, w[:, None] * Wh[col])
        if S is not None:
            hp = hp + xh @ S[h]
        outs.append(F.elu(hp) if concat else hp)
        alphas.append(alpha)
        zs.append(z.detach())
        scales.append((s[src].abs() + t[col].abs()).detach())
    out = torch.cat(outs, 1) if concat else torch.mean(torch.stack(outs, 1), 1)
    al = torch.stack(alphas, 1)
    return (out, al, torch.stack(zs, 1), torch.stack(scales, 1)) if want_z else (out, al)


def kink_count(x, rowptr, col, W, a, slope=0.2, mask_x=None, mask_wh=None, tau=parity.KINK_TAU):
    """(edge, head) pairs of the fp64 run with a logit inside the rounding band of the LeakyReLU kink, |z| <= tau (|s_i| + |t_j|).
    A logit with s_i = t_j = 0 EXACTLY (train-mode dropout that masked both Wh rows entirely: 0.6^8 of the nodes at p = 0.6,
    F' = 8) is not counted: it is 0 in every precision, no rounding decides its branch, and z > 0 is false for all of them."""
    with torch.no_grad():
        _, _, z, sc = level_ref(x.double(), rowptr, col, W.double(), a.double(), None, slope, True, mask_x, mask_wh, want_z=True)
    return int(((z.abs() <= tau * sc) & (sc > 0)).sum())
