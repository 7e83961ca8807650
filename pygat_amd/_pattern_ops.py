"""What the pattern ops share (spmm.py, edge_softmax.py, dot_attention.py, additive_attention.py, gatv2_attention.py): the pattern
itself, the refusals that look at nothing but the arguments, worded once, the front of the three dropout ops, the opening of the three
attention backwards and the buffers of a pass.  Private, at the bottom of the family's import order, and without a call into the
library: every launch stays in the op's own module, the public names too.  Each op keeps its own ORDER of refusals -- it calls these
one by one."""
from __future__ import annotations

import math
from typing import Optional, Tuple

import torch

MAX_ROW_FLOATS = 1024      # H * F of one call (csrc/k17_spmm.hip)
MAX_HEADS = 64
MIN_F, MAX_F = 4, 256      # a head's width in the attention ops: a power of two in this range (csrc/da_family.h)

_E_WANT = "; e [E, H, F] (or [E, F] without a head axis), a row per entry at the caller's entry index, expected"


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


# ---------------------------------------------------------------------------------------------------------------- the refusals
def _require_pattern(op: str, pattern):
    if not isinstance(pattern, EdgePattern):
        raise ValueError(f"pygat_amd {op}: an EdgePattern expected (EdgePattern.from_indices, CSRGraph.edge_pattern)")


def _require_tensor(op: str, pattern, name: str, t, dtype=torch.float32, want: str = ""):
    """The refusals of one tensor that look at nothing but it and the pattern: a tensor on the GPU, of `dtype` (float32, or bfloat16:
    a table of an inference forward), on the pattern's device.  want: what the message adds."""
    _require_pattern(op, pattern)
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"pygat_amd {op}: {name} must be a tensor on the GPU (there is no CPU path){want}")
    if t.dtype != dtype:
        like = "float32" if dtype == torch.float32 else "bfloat16 like the other table"
        raise ValueError(f"pygat_amd {op}: {name} must be {like}, not {t.dtype}{want}")
    if t.device != pattern.device:
        raise ValueError(f"pygat_amd {op}: {name} lives on {t.device}, the pattern on {pattern.device}{want}")


def _require_rows(op: str, named):
    """named = ((name, tensor, rows, side), ...): every table has the rows of its side of the pattern."""
    for name, t, rows, side in named:
        if t.shape[0] != rows:
            raise ValueError(f"pygat_amd {op}: {name} has {t.shape[0]} rows but the pattern has {rows} {side}")


def _require_row_floats(op: str, H: int, F: int):
    """The row shapes the K17 kernels take (spmm, edge_dot): any F."""
    if not (1 <= H <= MAX_HEADS) or F < 1 or H * F > MAX_ROW_FLOATS:
        raise ValueError(f"pygat_amd {op}: H = {H} heads of F = {F} columns: the limits are 1 <= H <= {MAX_HEADS}, F >= 1 and "
                         f"H * F <= {MAX_ROW_FLOATS} floats per row")


def _require_heads(op: str, H: int, F: int, pad_hint: str):
    """The row shapes the K19, K20 and K21 kernels take (csrc/da_family.h); pad_hint: how the op's caller reaches an allowed F."""
    if not (1 <= H <= MAX_HEADS):
        raise ValueError(f"pygat_amd {op}: H = {H} heads: the limits are 1 <= H <= {MAX_HEADS}")
    if not (MIN_F <= F <= MAX_F) or F & (F - 1):
        raise ValueError(f"pygat_amd {op}: F = {F}: a head's width must be a power of two in {MIN_F}..{MAX_F}; {pad_hint}")
    if H * F > MAX_ROW_FLOATS:
        raise ValueError(f"pygat_amd {op}: H * F = {H} * {F} = {H * F} floats per row: the limit is H * F <= {MAX_ROW_FLOATS}; "
                         f"{pad_hint}")


def _head_stride(op: str, pattern, name: str, t, H: int, flat: bool) -> int:
    """The head stride of a per-entry scalar term (bias, edge_logit) -> 1: one value per entry and head ([E, H]; [E] where the tables
    have no head axis); 0: one per entry, shared by the heads."""
    E = pattern.nnz
    if tuple(t.shape) == (E,):
        return 1 if flat else 0
    if not flat and tuple(t.shape) == (E, H):
        return 1
    want = f"[E] = [{E}]" if flat else f"[E, H] = [{E}, {H}] or [E] = [{E}]"
    raise ValueError(f"pygat_amd {op}: {name} {want} expected for E = {E} entries and H = {H} heads, got {tuple(t.shape)}")


def _require_entry_rows(op: str, pattern, name: str, e, table_name: str, table):
    """The shape of the per-entry rows e (e16): a row per entry, shaped like a row of `table` (q, x_dst)."""
    if tuple(e.shape) != (pattern.nnz,) + tuple(table.shape[1:]):
        raise ValueError(f"pygat_amd {op}: {name} {[pattern.nnz] + list(table.shape[1:])} expected for E = {pattern.nnz} entries and "
                         f"{table_name} {tuple(table.shape)} -- (E,) + {table_name}.shape[1:], a row per entry -- got {tuple(e.shape)}")


def _slope(op: str, negative_slope) -> float:
    """The negative slope of additive_attention's and gatv2_attention's LeakyReLU: a finite float."""
    if isinstance(negative_slope, bool) or not isinstance(negative_slope, (int, float)) or not math.isfinite(negative_slope):
        raise ValueError(f"pygat_amd {op}: negative_slope = {negative_slope!r}: a finite float expected")
    return float(negative_slope)


def _require_inference(op: str, f32_op: str, tensors):
    """The bf16-table siblings of additive_attention and gatv2_attention are forward only: with grad mode on, an argument that
    requires grad is refused, and the message names both ways out."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in tensors):
        raise ValueError(f"pygat_amd {op}: bfloat16 tables are for inference (there is no backward through this op) and an argument "
                         f"requires grad: call it under torch.no_grad(), or use {f32_op} on float32 tables")


def _require_dtypes(op: str, named):
    """named = ((name, tensor | None, dtype), ...) of a bf16-table op: which of its tensors are bfloat16 tables and which stay
    float32.  A tensor of the other kind is refused in words that name it and both dtypes (anything that is no tensor is left to
    _require_tensor)."""
    for name, t, dtype in named:
        if isinstance(t, torch.Tensor) and t.dtype != dtype:
            role = ("a bfloat16 table of this op (make it once: t.bfloat16())" if dtype == torch.bfloat16 else
                    "float32 in this op: only the row tables of H * F values are bfloat16")
            raise ValueError(f"pygat_amd {op}: {name} must be {dtype}, not {t.dtype}: it is {role}")


def _require_float32_grad(op: str, G):
    if G.dtype != torch.float32:
        raise ValueError(f"pygat_amd {op}: the gradient of the output must be float32, not {G.dtype}")


# ------------------------------------------------------------------------------------------------------------------ the dropout ops
def _drop_p(op: str, p) -> float:
    if isinstance(p, bool) or not isinstance(p, (int, float)) or not 0.0 <= p <= 1.0:          # (a NaN is outside)
        raise ValueError(f"pygat_amd {op}: p = {p!r}: a dropout probability in [0, 1] expected")
    return float(p)


def _drop_seed(op: str, pattern, seed):
    _require_pattern(op, pattern)
    if not isinstance(seed, torch.Tensor) or seed.dtype != torch.int64 or tuple(seed.shape) != (1,) or seed.device != pattern.device:
        got = f"{seed.dtype} {tuple(seed.shape)} on {seed.device}" if isinstance(seed, torch.Tensor) else type(seed).__name__
        raise ValueError(f"pygat_amd {op}: seed must be an int64 tensor of shape [1] on the pattern's device {pattern.device} (the "
                         f"kernels read it there, so a captured graph replays with the value it finds), got {got}")
    return seed.contiguous()


def _draw_seed(device, generator) -> torch.Tensor:
    """The seed of a call that was given none."""
    return torch.randint(0, 2 ** 62, (1,), dtype=torch.int64, device=device, generator=generator)


def _dropout_front(op: str, pattern, floats, bf16_refusal: str, p, negative_slope, seed, generator, training: bool, checked):
    """What the three *_dropout ops do before their autograd function, in their order: bfloat16 among `floats` is refused in the op's
    own words, then p, the slope (None: the op has none), a seed that was given and -- checked() -- every refusal of the plain op
    under this op's name, before anything touches the device.  -> (slope, drop): drop None where the call is the plain op's
    (training=False or p == 0), else (p, seed), the seed drawn where none was given."""
    if any(isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 for t in floats):
        raise ValueError(f"pygat_amd {op}: {bf16_refusal}")
    p = _drop_p(op, p)
    slope = None if negative_slope is None else _slope(op, negative_slope)
    if seed is not None:
        seed = _drop_seed(op, pattern, seed)
    checked()
    if not training or p == 0.0:
        return slope, None
    return slope, (p, _draw_seed(pattern.device, generator) if seed is None else seed)


# ------------------------------------------------------------------------------------------------ the passes of the attention ops
def _forward_buffers(n: int, H: int, F: int, dev, state: bool = True):
    """-> (out [n, H * F], m, Z): m and Z [n, H] what a backward reads (None without state: an inference forward keeps nothing)."""
    out = torch.empty(n, H * F, dtype=torch.float32, device=dev)
    m, Z = (torch.empty(n, H, dtype=torch.float32, device=dev) for _ in range(2)) if state else (None, None)
    return out, m, Z


def _entry_buffers(nnz: int, H: int, dev):
    """-> (P, S), [E, H] each: what the row pass of a backward leaves for the passes on the transposed pattern."""
    return torch.empty(nnz, H, dtype=torch.float32, device=dev), torch.empty(nnz, H, dtype=torch.float32, device=dev)


def _backward_opening(op: str, G, out, n_args: int, grads):
    """How the three attention backwards open.  grads = {the place among forward's n_args arguments: (tensor, needed)} of those that
    take a gradient, in the order of the places.  A gradient that is not float32 is refused; -> what backward returns where no launch
    is due -- Nones when nothing is needed, zeros when the pattern has no entries (forward kept no out) -- or None: go on."""
    _require_float32_grad(op, G)
    if out is not None and any(need for _, need in grads.values()):
        return None
    early = [None] * n_args
    for place, (t, need) in grads.items():
        if need:
            early[place] = torch.zeros_like(t)
    return tuple(early)
