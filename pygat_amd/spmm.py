"""The reference's sparse-region SpMM (SpecialSpmmFunction / SpecialSpmm, layers.py:70-95) as an op of its own, on the K17 kernels
(csrc/k17_spmm.hip).

  out[i, h, :] = sum over the entries k = (i, j) of the pattern of  values[k, h] * b[j, h, :]

    pattern = graph.edge_pattern()                       # or EdgePattern.from_indices(indices [2, E], (n_rows, n_cols))
    y = spmm(pattern, alpha, table.view(N, H, F))        # alpha [E, H] of gat_level(..., return_attention="grad") plugs in unchanged
    h_prime = SpecialSpmm()(edge, edge_e, torch.Size([N, N]), h)      # the reference's call, unchanged

Gradients flow to `values` (an edge-parallel SDDMM, O(E F): the reference forms a dense N x N product, layers.py:85) and to `b` (the
same SpMM on the transposed pattern).  fp32, no float atomics, a fixed summation order: two runs give the same bits.  There is no
CPU path and no fallback to torch.sparse.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check
from ._pattern_ops import (EdgePattern, MAX_HEADS, MAX_ROW_FLOATS, _csr_of, _ptr, _require_float32_grad,    # noqa: F401
                           _require_row_floats, _require_rows, _require_tensor, _stream)     # (the pattern's home was this module)

PATTERN_CACHE_SIZE = 8     # patterns SpecialSpmm keeps (the reference passes the same `edge` tensor to every head and every step)


def _shapes(pattern: EdgePattern, values: torch.Tensor, b: torch.Tensor):
    """-> (H, F) of a call, after every refusal."""
    for name, t in (("values", values), ("b", b)):
        _require_tensor("spmm", pattern, name, t)
    if values.dim() == 1 and b.dim() == 2:
        H, F = 1, int(b.shape[1])
    elif values.dim() == 2 and b.dim() == 3 and values.shape[1] == b.shape[1]:
        H, F = int(b.shape[1]), int(b.shape[2])
    else:
        raise ValueError(f"pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values "
                         f"{tuple(values.shape)} and b {tuple(b.shape)}")
    _require_rows("spmm", (("values", values, pattern.nnz, "entries"), ("b", b, pattern.n_cols, "columns")))
    _require_row_floats("spmm", H, F)
    return H, F


def _launch_spmm(n_rows, nnz, rowptr, col, perm, H, F, val, table):
    """out [n_rows, H * F] = the pattern (rowptr, col, perm) with values val [nnz, H] times table [*, H * F]."""
    out = torch.empty(n_rows, H * F, dtype=torch.float32, device=table.device)
    with torch.cuda.device(table.device):
        ws = torch.empty(_lib.spmm_workspace_bytes(nnz, H, F), dtype=torch.uint8, device=table.device)
        check(lib.pygat_spmm_forward(n_rows, nnz, _ptr(rowptr), _ptr(col), _ptr(perm), H, F, _ptr(val), _ptr(table), H * F,
                                     _ptr(out), H * F, _ptr(ws), _stream()), "spmm_forward")
    return out


def _forward(pattern: EdgePattern, values: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    H, F = _shapes(pattern, values, b)
    out = _launch_spmm(pattern.n_rows, pattern.nnz, pattern.rowptr, pattern.col, pattern.perm, H, F, values.detach().contiguous(),
                       b.detach().contiguous())
    return out.view((pattern.n_rows,) + tuple(b.shape[1:]))


def _backward(pattern: EdgePattern, values: torch.Tensor, b: torch.Tensor, G: torch.Tensor, need_values: bool, need_b: bool):
    """Only the launches asked for: the SDDMM for dvalues, the transposed pattern and its SpMM for db."""
    values_shape, b_shape = values.shape, b.shape
    H, F = (1, int(b.shape[1])) if b.dim() == 2 else (int(b.shape[1]), int(b.shape[2]))
    val, table = values.detach().contiguous(), b.detach().contiguous()
    _require_float32_grad("spmm", G)
    G = G.contiguous().view(pattern.n_rows, H * F)
    dval = db = None
    if need_values:
        dval = torch.empty(pattern.nnz, H, dtype=torch.float32, device=G.device)
        with torch.cuda.device(G.device):
            check(lib.pygat_spmm_grad_values(pattern.nnz, _ptr(pattern.edge_rc), H, F, _ptr(G), H * F, _ptr(table), H * F, _ptr(dval),
                                             _stream()), "spmm_grad_values")
        dval = dval.view(values_shape)
    if need_b:
        rowptr_t, row_t, perm_t = pattern.transposed()
        db = _launch_spmm(pattern.n_cols, pattern.nnz, rowptr_t, row_t, perm_t, H, F, val, G).view(b_shape)
    return dval, db


class _SpmmFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, values, b):
        out = _forward(pattern, values, b)
        ctx.pattern = pattern
        ctx.save_for_backward(values, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        dval, db = _backward(ctx.pattern, *ctx.saved_tensors, G, ctx.needs_input_grad[1], ctx.needs_input_grad[2])
        return None, dval, db


def spmm(pattern: EdgePattern, values: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """out [N, F] (values [E], b [M, F]) or out [N, H, F] (values [E, H], b [M, H, F]): out[i] = sum over the entries k = (i, j) of
    values[k] * b[j], per head.  Differentiable in values and b.  float32 GPU tensors; H <= 64 and H * F <= 1024."""
    return _SpmmFn.apply(pattern, values, b)


# ---------------------------------------------------------------------------------------------------------------------------------
# The reference's names and signature.  The pattern of an index tensor is built once and kept: the key is the tensor's storage,
# offset, strides, shape and version counter, and the entry holds the tensor, so its memory cannot be handed to other indices while
# the entry lives.
# ---------------------------------------------------------------------------------------------------------------------------------
_patterns: "OrderedDict[tuple, Tuple[torch.Tensor, EdgePattern]]" = OrderedDict()


def clear_pattern_cache() -> None:
    """Forget the patterns SpecialSpmm built (and release the index tensors they hold)."""
    _patterns.clear()


def _cached_pattern(indices: torch.Tensor, shape) -> EdgePattern:
    if not isinstance(indices, torch.Tensor) or not indices.is_cuda:
        raise ValueError("pygat_amd spmm: indices must be a tensor on the GPU (there is no CPU path)")
    if len(shape) != 2:
        raise ValueError("pygat_amd spmm: shape (n_rows, n_cols) expected")
    key = (indices.untyped_storage().data_ptr(), indices.storage_offset(), tuple(indices.stride()), tuple(indices.shape),
           indices.dtype, str(indices.device), indices._version, int(shape[0]), int(shape[1]))
    hit = _patterns.get(key)
    if hit is not None:
        _patterns.move_to_end(key)
        return hit[1]
    pattern = EdgePattern.from_indices(indices, shape)
    _patterns[key] = (indices, pattern)
    while len(_patterns) > PATTERN_CACHE_SIZE:
        _patterns.popitem(last=False)
    return pattern


class SpecialSpmmFunction(torch.autograd.Function):
    """layers.py:70-84: apply(indices [2, E], values [E], shape, b [M, F]) -> sparse(indices, values, shape) @ b, with gradients
    for values and b only."""

    @staticmethod
    def forward(ctx, indices, values, shape, b):
        if getattr(indices, "requires_grad", False):
            raise ValueError("pygat_amd spmm: indices must not require a gradient")
        if isinstance(values, torch.Tensor) and isinstance(b, torch.Tensor) and (values.dim() != 1 or b.dim() != 2):
            raise ValueError(f"pygat_amd spmm: SpecialSpmm takes values [E] and b [M, F]; got values {tuple(values.shape)} and b "
                             f"{tuple(b.shape)} (spmm takes heads)")
        pattern = _cached_pattern(indices, shape)
        out = _forward(pattern, values, b)
        ctx.pattern = pattern
        ctx.save_for_backward(values, b)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_output):
        dval, db = _backward(ctx.pattern, *ctx.saved_tensors, grad_output, ctx.needs_input_grad[1], ctx.needs_input_grad[3])
        return None, dval, None, db


class SpecialSpmm(torch.nn.Module):
    """layers.py:93-95."""

    def forward(self, indices, values, shape, b):
        return SpecialSpmmFunction.apply(indices, values, shape, b)
