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
from typing import Optional, Tuple

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check

MAX_ROW_FLOATS = 1024      # H * F of one call (csrc/k17_spmm.hip)
MAX_HEADS = 64
PATTERN_CACHE_SIZE = 8     # patterns SpecialSpmm keeps (the reference passes the same `edge` tensor to every head and every step)


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _csr_of(key: torch.Tensor, other: torch.Tensor, n: int):
    """Entries sorted by `key`, stable: -> (rowptr [n + 1], the other index in that order, perm = the caller's entry index of every
    sorted position), all int32.  No host read."""
    order = torch.sort(key, stable=True).indices
    rowptr = torch.searchsorted(key[order].contiguous(), torch.arange(n + 1, device=key.device, dtype=key.dtype))
    return rowptr.to(torch.int32), other[order].to(torch.int32).contiguous(), order.to(torch.int32).contiguous()


class EdgePattern:
    """A device-resident COO entry list (row, col) of a sparse (n_rows, n_cols) matrix, which may be rectangular, as the K17
    kernels read it: the entries in the caller's order (edge_rc), the CSR by rows (rowptr, col, perm) and -- built the first time a
    gradient with respect to b is asked for -- the CSR by columns (rowptr_t, row_t, perm_t).  Entries may be unsorted and may
    repeat; repeats are separate entries and add, as torch.sparse_coo_tensor's do.  Sorting is stable, so the entries of a row (of
    a column) are added in the caller's order."""

    def __init__(self, shape, edge_rc, rowptr, col, perm, transposed=None):
        self.shape = (int(shape[0]), int(shape[1]))
        self.n_rows, self.n_cols = self.shape
        self.edge_rc, self.rowptr, self.col, self.perm = edge_rc, rowptr, col, perm
        self._t = transposed                                  # (rowptr_t, row_t, perm_t) or None: not built yet
        self.nnz = int(edge_rc.shape[0])
        self.device = edge_rc.device

    @staticmethod
    def from_indices(indices: torch.Tensor, shape) -> "EdgePattern":
        """indices [2, E] (row 0 = the row, row 1 = the column of every entry, any integer dtype), shape = (n_rows, n_cols).
        The indices are range-checked on the device, once, here: a violation is a ValueError."""
        if not isinstance(indices, torch.Tensor) or indices.dim() != 2 or indices.shape[0] != 2:
            raise ValueError("pygat_amd spmm: indices [2, E] expected")
        if not indices.is_cuda:
            raise ValueError("pygat_amd spmm: indices must live on the GPU (there is no CPU path)")
        if indices.dtype.is_floating_point or indices.dtype in (torch.bool, torch.complex64, torch.complex128):
            raise ValueError(f"pygat_amd spmm: integer indices expected, not {indices.dtype}")
        if len(shape) != 2:
            raise ValueError("pygat_amd spmm: shape (n_rows, n_cols) expected")
        n_rows, n_cols, E = int(shape[0]), int(shape[1]), int(indices.shape[1])
        if not (0 < n_rows < 2 ** 31 and 0 < n_cols < 2 ** 31 and E < 2 ** 31):
            raise ValueError(f"pygat_amd spmm: n_rows={n_rows}, n_cols={n_cols} must lie in [1, 2^31) and nnz={E} below 2^31")
        if torch.cuda.is_current_stream_capturing():
            raise ValueError("pygat_amd spmm: a pattern cannot be built during stream capture (its index check reads a flag back); "
                             "build it -- or call SpecialSpmm once with these indices -- before the capture")
        with torch.cuda.device(indices.device):
            row, col = indices[0].long(), indices[1].long()
            if E and bool(((row < 0) | (row >= n_rows) | (col < 0) | (col >= n_cols)).any()):
                raise ValueError(f"pygat_amd spmm: an index lies outside the shape ({n_rows}, {n_cols})")
            edge_rc = torch.stack([row, col], 1).to(torch.int32).contiguous()
            rowptr, c, perm = _csr_of(row, col, n_rows)
        return EdgePattern((n_rows, n_cols), edge_rc, rowptr, c, perm)

    @property
    def has_transpose(self) -> bool:
        return self._t is not None

    def transposed(self) -> Tuple[torch.Tensor, torch.Tensor, Optional[torch.Tensor]]:
        """(rowptr_t [n_cols + 1], row_t [E], perm_t [E]): the CSR by columns, built on first use."""
        if self._t is None:
            with torch.cuda.device(self.device):
                self._t = _csr_of(self.edge_rc[:, 1].long(), self.edge_rc[:, 0].long(), self.n_cols)
        return self._t


def _shapes(pattern: EdgePattern, values: torch.Tensor, b: torch.Tensor):
    """-> (H, F) of a call, after every refusal."""
    if not isinstance(pattern, EdgePattern):
        raise ValueError("pygat_amd spmm: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)")
    for name, t in (("values", values), ("b", b)):
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError(f"pygat_amd spmm: {name} must be a tensor on the GPU (there is no CPU path)")
        if t.dtype != torch.float32:
            raise ValueError(f"pygat_amd spmm: {name} must be float32, not {t.dtype}")
        if t.device != pattern.device:
            raise ValueError(f"pygat_amd spmm: {name} lives on {t.device}, the pattern on {pattern.device}")
    if values.dim() == 1 and b.dim() == 2:
        H, F = 1, int(b.shape[1])
    elif values.dim() == 2 and b.dim() == 3 and values.shape[1] == b.shape[1]:
        H, F = int(b.shape[1]), int(b.shape[2])
    else:
        raise ValueError(f"pygat_amd spmm: values [E] with b [M, F], or values [E, H] with b [M, H, F], expected; got values "
                         f"{tuple(values.shape)} and b {tuple(b.shape)}")
    if values.shape[0] != pattern.nnz:
        raise ValueError(f"pygat_amd spmm: values has {values.shape[0]} rows but the pattern has {pattern.nnz} entries")
    if b.shape[0] != pattern.n_cols:
        raise ValueError(f"pygat_amd spmm: b has {b.shape[0]} rows but the pattern has {pattern.n_cols} columns")
    if not (1 <= H <= MAX_HEADS) or F < 1 or H * F > MAX_ROW_FLOATS:
        raise ValueError(f"pygat_amd spmm: H = {H} heads of F = {F} columns: the limits are 1 <= H <= {MAX_HEADS}, F >= 1 and "
                         f"H * F <= {MAX_ROW_FLOATS} floats per row")
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
    if G.dtype != torch.float32:
        raise ValueError(f"pygat_amd spmm: the gradient of the output must be float32, not {G.dtype}")
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
