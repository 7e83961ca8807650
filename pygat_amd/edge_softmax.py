"""The softmax of per-entry logits over the entries of every row (or column) of a sparse pattern, as an op of its own on the K18
kernels (csrc/k18_edge_softmax.hip): what the reference's layers.py:145-150,160 computes with attention dropout off.

  alpha[k, h] = exp(logits[k, h] - m[i, h]) / sum over the entries k' of group i of exp(logits[k', h] - m[i, h]),  m = the group's maximum

    pattern = graph.edge_pattern()                       # or EdgePattern.from_indices(indices [2, E], (n_rows, n_cols))
    alpha = edge_softmax(pattern, my_logits)             # [E] or [E, H], the caller's entry order, as spmm's values
    y = spmm(pattern, alpha, table.view(N, H, F))

The group of entry k = (i, j) is its row i (by="row") or its column j (by="col", on pattern.transposed()).  Differentiable in the
logits: dlogits = alpha (G - c), c = the group's sum of alpha G; the backward keeps alpha and nothing else per entry.  fp32, no float
atomics, a fixed summation order: two runs give the same bits.  Nothing is read back to the host.  There is no CPU path and no
fallback to torch.
"""
from __future__ import annotations

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check
from ._pattern_ops import EdgePattern, MAX_HEADS, _ptr, _require_float32_grad, _require_pattern, _require_rows, _require_tensor, _stream


def _grouping(pattern: EdgePattern, by: str):
    """-> (groups, rowptr, perm, side): the CSR of the grouping side and the half of edge_rc that names an entry's group."""
    if by == "row":
        return pattern.n_rows, pattern.rowptr, pattern.perm, 0
    rowptr_t, _, perm_t = pattern.transposed()
    return pattern.n_cols, rowptr_t, perm_t, 1


def _heads(pattern, logits: torch.Tensor, by) -> int:
    """-> H of a call, after every refusal."""
    _require_pattern("edge_softmax", pattern)
    if by not in ("row", "col"):
        raise ValueError(f"pygat_amd edge_softmax: by must be \"row\" or \"col\", not {by!r}")
    _require_tensor("edge_softmax", pattern, "logits", logits)
    if logits.dim() not in (1, 2):
        raise ValueError(f"pygat_amd edge_softmax: logits [E] or [E, H] expected, got {tuple(logits.shape)}")
    _require_rows("edge_softmax", (("logits", logits, pattern.nnz, "entries"),))
    H = 1 if logits.dim() == 1 else int(logits.shape[1])
    if not (1 <= H <= MAX_HEADS):
        raise ValueError(f"pygat_amd edge_softmax: H = {H} heads: the limits are 1 <= H <= {MAX_HEADS}")
    return H


def _workspace(nnz: int, H: int, device) -> torch.Tensor:
    return torch.empty(_lib.edge_softmax_workspace_bytes(nnz, H), dtype=torch.uint8, device=device)


def _forward(pattern: EdgePattern, logits: torch.Tensor, by: str) -> torch.Tensor:
    H = _heads(pattern, logits, by)
    x = logits.detach().contiguous()
    alpha = torch.empty_like(x)
    if pattern.nnz == 0:
        return alpha
    n, rowptr, perm, side = _grouping(pattern, by)
    with torch.cuda.device(x.device):
        m, Z = torch.empty(n, H, dtype=torch.float32, device=x.device), torch.empty(n, H, dtype=torch.float32, device=x.device)
        ws = _workspace(pattern.nnz, H, x.device)
        check(lib.pygat_edge_softmax_rows(n, pattern.nnz, _ptr(rowptr), _ptr(perm), H, _ptr(x), _ptr(m), _ptr(Z), _ptr(ws), _stream()),
              "edge_softmax_rows")
        check(lib.pygat_edge_softmax_apply(pattern.nnz, _ptr(pattern.edge_rc), side, H, _ptr(x), _ptr(m), _ptr(Z), _ptr(alpha),
                                           _stream()), "edge_softmax_apply")
    return alpha


def _backward(pattern: EdgePattern, alpha: torch.Tensor, by: str, G: torch.Tensor) -> torch.Tensor:
    _require_float32_grad("edge_softmax", G)
    G = G.contiguous()
    dl = torch.empty_like(alpha)
    if pattern.nnz == 0:
        return dl
    H = 1 if alpha.dim() == 1 else int(alpha.shape[1])
    n, rowptr, perm, side = _grouping(pattern, by)
    with torch.cuda.device(alpha.device):
        c = torch.empty(n, H, dtype=torch.float32, device=alpha.device)
        ws = _workspace(pattern.nnz, H, alpha.device)
        check(lib.pygat_edge_softmax_grad_rows(n, pattern.nnz, _ptr(rowptr), _ptr(perm), H, _ptr(alpha), _ptr(G), _ptr(c), _ptr(ws),
                                               _stream()), "edge_softmax_grad_rows")
        check(lib.pygat_edge_softmax_grad_apply(pattern.nnz, _ptr(pattern.edge_rc), side, H, _ptr(alpha), _ptr(G), _ptr(c), _ptr(dl),
                                                _stream()), "edge_softmax_grad_apply")
    return dl


class _EdgeSoftmaxFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, logits, by):
        alpha = _forward(pattern, logits, by)
        ctx.pattern, ctx.by = pattern, by
        ctx.save_for_backward(alpha)
        return alpha

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        (alpha,) = ctx.saved_tensors
        return None, _backward(ctx.pattern, alpha, ctx.by, G), None


def edge_softmax(pattern: EdgePattern, logits: torch.Tensor, by: str = "row") -> torch.Tensor:
    """alpha like logits ([E] or [E, H], 1 <= H <= 64, float32 on the pattern's device, the caller's entry order): the softmax of the
    logits over the entries of every row (by="row") or column (by="col") of the pattern, per head.  Differentiable in logits."""
    return _EdgeSoftmaxFn.apply(pattern, logits, by)
