"""Dot-product attention over the entries of a sparse pattern -- the hot path of graph-transformer layers (TransformerConv / UniMP) -- and
its score as an op of its own.

  edge_dot       u[e, h] = scale * <q[row_e, h], k[col_e, h]>                 the SDDMM of csrc/k17_spmm.hip with a public face
  dot_attention  out[i, h, :] = sum over the entries e = (i, j) of row i of  softmax_row(scale * q_i . k_j)[e, h] * v[j, h, :]
                 fused, on the K19 kernels (csrc/k19_dot_attention.hip): an online softmax per row, nothing written per entry

    pattern = graph.edge_pattern()                       # or EdgePattern.from_indices(indices [2, E], (n_rows, n_cols))
    out = dot_attention(pattern, q, k, v)                # q [n_rows, H, F]; k, v [n_cols, H, F]; scale = 1 / sqrt(F)
    out = spmm(pattern, edge_softmax(pattern, edge_dot(pattern, q, k, scale)), v)       # the same, from parts, with [E, H] tensors
    out = dot_attention(pattern, q, k, v, bias=emb(edge_type))    # a per-entry term on the score, [E, H] or [E]; differentiable too
    with torch.no_grad():                                         # inference: bf16 tables, made once -- half the gathered bytes, the
        out = dot_attention(pattern, q, k16, v16)                 # bits of dot_attention(pattern, q, k16.float(), v16.float())
    out = dot_attention_dropout(pattern, q, k, v, p, bias=b, training=self.training)    # training: dropout p on the coefficients, after
                                                                  # the softmax, drawn in the kernels from a seed on the device
    out = dot_attention_edge(pattern, q, k, v, e, bias=b)         # edge features: e [E, H, F] joins k[col] in the score and v[col] in
                                                                  # the sum (the EDGE instantiations); differentiable in e too

A row's softmax runs over exactly its entries; repeated (row, col) pairs are separate entries; entries may be unsorted and the
pattern rectangular.  To attend over columns instead of rows, build the pattern from swapped indices.  Both ops are differentiable
in every tensor.  The backward of dot_attention keeps out and (m, Z) per row; its two per-entry tensors P and S ([E, H] each) live
only inside backward, between the row pass and the two transposed SpMMs that form dk and dv.  fp32, no float atomics, a fixed
summation order: two runs give the same bits.  Nothing is read back to the host.  There is no CPU path and no fallback to torch.
dot_attention also takes k and v as bfloat16 tables for inference (the bf16-table instantiations of the K19 forward kernels): no
backward, no fp32 copy of either table, the float32 op's result on the widened tables bit for bit.  edge_dot stays float32 only.
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check
from .dropout import STREAM_ATT
from ._pattern_ops import (EdgePattern, MAX_HEADS, _E_WANT, _backward_opening, _drop_p, _drop_seed, _dropout_front, _entry_buffers,
                           _forward_buffers, _head_stride, _ptr, _require_entry_rows, _require_float32_grad, _require_heads,
                           _require_pattern, _require_row_floats, _require_rows, _require_tensor, _stream)
from .spmm import _launch_spmm

_PAD_HINT = ("zero-padding the columns of q, k and v to the next allowed F leaves the first F columns of the result unchanged "
             "(pass scale yourself: the default follows the padded F)")


def _tables(op: str, pattern, q, others, bf16_others: bool = False):
    """The refusals both ops share -> (H, F, no head axis): q [n_rows, (H,) F]; others = ((name, tensor), ...) over the columns,
    float32 like q, or bfloat16 where bf16_others (dot_attention's inference forward)."""
    _require_pattern(op, pattern)
    named = (("q", q, pattern.n_rows, "rows"),) + tuple((name, t, pattern.n_cols, "columns") for name, t in others)
    for name, t, _, _ in named:
        _require_tensor(op, pattern, name, t, torch.bfloat16 if bf16_others and name != "q" else torch.float32)
    if q.dim() not in (2, 3):
        raise ValueError(f"pygat_amd {op}: q [n_rows, F] or [n_rows, H, F] expected, got {tuple(q.shape)}")
    for name, t in others:
        if t.dim() != q.dim() or t.shape[1:] != q.shape[1:]:
            raise ValueError(f"pygat_amd {op}: {name} {tuple(t.shape)} does not match q {tuple(q.shape)}: the same number of heads "
                             f"and the same F expected")
    _require_rows(op, named)
    H, F = (1, int(q.shape[1])) if q.dim() == 2 else (int(q.shape[1]), int(q.shape[2]))
    return H, F, q.dim() == 2


# ------------------------------------------------------------------------------------------------------------------------ edge_dot
def _sddmm(pattern: EdgePattern, H: int, F: int, a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """u [E, H], u[e, h] = <a[row_e, h], b[col_e, h]>: one pygat_spmm_grad_values launch with G := a."""
    u = torch.empty(pattern.nnz, H, dtype=torch.float32, device=a.device)
    if pattern.nnz:
        with torch.cuda.device(a.device):
            check(lib.pygat_spmm_grad_values(pattern.nnz, _ptr(pattern.edge_rc), H, F, _ptr(a), H * F, _ptr(b), H * F, _ptr(u),
                                             _stream()), "spmm_grad_values")
    return u


class _EdgeDotFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pattern, q, k, scale):
        H, F, flat = _tables("edge_dot", pattern, q, (("k", k),))
        _require_row_floats("edge_dot", H, F)
        u = _sddmm(pattern, H, F, q.detach().contiguous(), k.detach().contiguous())
        if scale != 1.0:
            u.mul_(scale)
        ctx.pattern, ctx.scale, ctx.hf = pattern, scale, (H, F)
        ctx.save_for_backward(q, k)
        return u.view(pattern.nnz) if flat else u

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, k = ctx.saved_tensors
        pattern, (H, F) = ctx.pattern, ctx.hf
        _require_float32_grad("edge_dot", g)
        dq = dk = None
        gs = (g if ctx.scale == 1.0 else g * ctx.scale).contiguous().view(pattern.nnz, H)
        if ctx.needs_input_grad[1]:
            dq = _launch_spmm(pattern.n_rows, pattern.nnz, pattern.rowptr, pattern.col, pattern.perm, H, F, gs,
                              k.detach().contiguous()).view(q.shape)
        if ctx.needs_input_grad[2]:
            rowptr_t, row_t, perm_t = pattern.transposed()
            dk = _launch_spmm(pattern.n_cols, pattern.nnz, rowptr_t, row_t, perm_t, H, F, gs, q.detach().contiguous()).view(k.shape)
        return None, dq, dk, None


def edge_dot(pattern: EdgePattern, q: torch.Tensor, k: torch.Tensor, scale: float = 1.0) -> torch.Tensor:
    """u [E, H] (q [n_rows, H, F], k [n_cols, H, F]) or u [E] (q [n_rows, F], k [n_cols, F]): u[e] = scale * <q[row_e], k[col_e]> per
    head, in the caller's entry order, as spmm's values.  Differentiable in q and k.  float32 GPU tensors; H <= 64, H * F <= 1024,
    any F >= 1."""
    return _EdgeDotFn.apply(pattern, q, k, float(scale))


# ------------------------------------------------------------------------------------------------------------------- dot_attention
def _checked(op: str, pattern, q, k, v, bias, e=None, bf16_tables: bool = False):
    """Every refusal that looks at the pattern and the tensors, those of e and bias alone first -> (H, F, no head axis, the bias's
    head stride | None)."""
    if e is not None:
        _require_tensor(op, pattern, "e", e, want=_E_WANT)
    if bias is not None:
        _require_tensor(op, pattern, "bias", bias)
    H, F, flat = _tables(op, pattern, q, (("k", k), ("v", v)), bf16_tables)
    _require_heads(op, H, F, _PAD_HINT)
    bhs = None if bias is None else _head_stride(op, pattern, "bias", bias, H, flat)
    if e is not None:
        _require_entry_rows(op, pattern, "e", e, "q", q)
    return H, F, flat, bhs


def _launch(pattern, which: str, H: int, F: int, scale: float, qc, kc, vc, ec, bc, bhs, drop, rest, bf16: bool = False):
    """One K19 launcher call, `which` "forward" or "backward_rows", at the entry point of what is present -- bf16 tables, e rows, a
    dropout (p, seed), a bias, or none of them -- on its argument list: the pattern's arrays, the three tables, the groups of e, bias
    and dropout, then `rest`, the pass's own arguments up to the workspace."""
    kind = "bf16_" if bf16 else "edge_" if ec is not None else "dropout_" if drop is not None else "bias_" if bc is not None else ""
    HF = H * F
    args = (pattern.n_rows, pattern.nnz, _ptr(pattern.rowptr), _ptr(pattern.col))
    if kind or which != "forward":                                 # (the forward without a flag walks in CSR order alone)
        args += (_ptr(pattern.perm),)
    args += (H, F, scale, _ptr(qc), HF, _ptr(kc), HF, _ptr(vc), HF)
    if ec is not None:
        args += (_ptr(ec), HF)
    if kind:
        args += (_ptr(bc), bhs or 0)
    if drop is not None:
        args += (drop[0], _ptr(drop[1]), STREAM_ATT)
    ws = torch.empty(_lib.dot_attn_workspace_bytes(pattern.nnz, H, F), dtype=torch.uint8, device=qc.device)
    check(getattr(lib, f"pygat_dot_attn_{kind}{which}")(*args, *rest, _ptr(ws), _stream()), f"dot_attn_{kind}{which}")


def _forward(pattern, H: int, F: int, scale: float, q, k, v, e, bias, bhs, drop, bf16: bool = False):
    """The forward launch on the tensors as they are -> (out [n_rows, H * F], m, Z), m and Z [n_rows, H] what a backward reads (None
    on bf16 tables: nothing is kept for one)."""
    qc, kc, vc, ec, bc = (None if t is None else t.detach().contiguous() for t in (q, k, v, e, bias))
    with torch.cuda.device(qc.device):
        out, m, Z = _forward_buffers(pattern.n_rows, H, F, qc.device, state=not bf16)
        _launch(pattern, "forward", H, F, scale, qc, kc, vc, ec, bc, bhs, drop,
                (_ptr(out), H * F) + (() if bf16 else (_ptr(m), _ptr(Z))), bf16)
    return out, m, Z


class _DotAttentionFn(torch.autograd.Function):
    """dot_attention, dot_attention_dropout and dot_attention_edge.  e: None or the [E, H, F] rows of dot_attention_edge; drop: None or
    (p, seed) of dot_attention_dropout: the mask of the coefficients, drawn in the kernels of both passes from the int64 [1] seed
    tensor on the device."""

    @staticmethod
    def forward(ctx, pattern, q, k, v, e, scale, bias, drop):
        op = "dot_attention_edge" if e is not None else "dot_attention" if drop is None else "dot_attention_dropout"
        H, F, flat, bhs = _checked(op, pattern, q, k, v, bias, e)
        scale = 1.0 / math.sqrt(F) if scale is None else float(scale)
        p, seed = (None, None) if drop is None else drop
        ctx.pattern, ctx.scale, ctx.hf, ctx.bhs, ctx.op, ctx.p = pattern, scale, (H, F), bhs, op, p
        if pattern.nnz == 0 and op != "dot_attention":             # every row is without entries: zeros, and nothing is launched
            ctx.save_for_backward(q, k, v, e, None, None, None, bias, None)
            return torch.zeros(q.shape, dtype=torch.float32, device=q.device)
        out, m, Z = _forward(pattern, H, F, scale, q, k, v, e, bias, bhs, drop)
        out = out.view(q.shape)
        ctx.save_for_backward(q, k, v, e, out, m, Z, bias, seed)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        q, k, v, e, out, m, Z, bias, seed = ctx.saved_tensors
        pattern, scale, (H, F), bhs = ctx.pattern, ctx.scale, ctx.hf, ctx.bhs
        need_q, need_k, need_v = ctx.needs_input_grad[1:4]
        need_e, need_b = e is not None and ctx.needs_input_grad[4], bias is not None and ctx.needs_input_grad[6]
        early = _backward_opening(ctx.op, G, out, 8, {1: (q, need_q), 2: (k, need_k), 3: (v, need_v), 4: (e, need_e), 6: (bias, need_b)})
        if early is not None:
            return early
        n, nnz, HF = pattern.n_rows, pattern.nnz, H * F
        qc, kc, vc, ec, bc = (None if t is None else t.detach().contiguous() for t in (q, k, v, e, bias))
        Gc = G.contiguous().view(n, HF)
        with torch.cuda.device(qc.device):
            dq = torch.empty(n, HF, dtype=torch.float32, device=qc.device)
            P, S = _entry_buffers(nnz, H, qc.device)
            de = torch.empty(nnz, HF, dtype=torch.float32, device=qc.device) if need_e else None      # (every row is written once)
            db = torch.empty(nnz, H, dtype=torch.float32, device=qc.device) if need_b else None
            rest = (_ptr(out), HF, _ptr(m), _ptr(Z), _ptr(Gc), HF, _ptr(dq), HF, _ptr(P), _ptr(S))
            if e is not None:
                rest += (_ptr(de), HF)
            if e is not None or bias is not None or seed is not None:      # (every entry point but the one without a flag)
                rest += (_ptr(db),)
            _launch(pattern, "backward_rows", H, F, scale, qc, kc, vc, ec, bc, bhs, None if seed is None else (ctx.p, seed), rest)
            if need_b:                          # [E, H] -> the bias's own shape: a [E] bias shared by H heads gets the sum over them
                db = db.sum(1) if bhs == 0 else db.view(bias.shape)
        dk = dv = None
        if need_k or need_v:
            rowptr_t, row_t, perm_t = pattern.transposed()
            if need_k:
                dk = _launch_spmm(pattern.n_cols, nnz, rowptr_t, row_t, perm_t, H, F, S, qc.view(n, HF)).view(k.shape)
            if need_v:
                dv = _launch_spmm(pattern.n_cols, nnz, rowptr_t, row_t, perm_t, H, F, P, Gc).view(v.shape)
        return None, dq.view(q.shape) if need_q else None, dk, dv, de.view(e.shape) if need_e else None, None, db, None


def _bf16_tables(k, v) -> bool:
    """k and v are both bfloat16 (the inference forward); one of them alone is refused."""
    kb, vb = (isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 for t in (k, v))
    if kb != vb:
        kd, vd = (getattr(t, "dtype", type(t).__name__) for t in (k, v))
        raise ValueError(f"pygat_amd dot_attention: k is {kd} and v is {vd}: the inference forward takes both k and v as bfloat16 "
                         f"tables (k.bfloat16(), v.bfloat16()); otherwise both are float32")
    return kb


def _dot_attention_bf16(pattern, q, k, v, scale, bias):
    """The inference forward on bfloat16 k and v: one pygat_dot_attn_bf16_forward launch on the tables as they are -- nothing is
    widened, nothing is kept for a backward."""
    if torch.is_grad_enabled() and any(isinstance(t, torch.Tensor) and t.requires_grad for t in (q, k, v, bias)):
        raise ValueError("pygat_amd dot_attention: bfloat16 k and v are for inference (there is no backward through them): call it "
                         "under torch.no_grad(), or pass float32 tables")
    H, F, flat, bhs = _checked("dot_attention", pattern, q, k, v, bias, bf16_tables=True)
    scale = 1.0 / math.sqrt(F) if scale is None else float(scale)
    if pattern.nnz == 0:                        # every row is without entries
        return torch.zeros(q.shape, dtype=torch.float32, device=q.device)
    return _forward(pattern, H, F, scale, q, k, v, None, bias, 1 if bias is None else bhs, None, bf16=True)[0].view(q.shape)


def dot_attention(pattern: EdgePattern, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, scale: Optional[float] = None,
                  bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out like q ([n_rows, H, F], or [n_rows, F] with k, v [n_cols, F]): out[i] = sum over the entries (i, j) of row i of
    softmax_j(scale * <q[i], k[j]> + bias[e]) * v[j], per head; scale defaults to 1 / sqrt(F).  A row without entries gets zeros.
    bias (optional): a per-entry term on the score, at the caller's entry index -- [E, H], or [E] for one value per entry shared by
    the heads (and where q, k and v have no head axis) -- taken into the softmax as (scale * <q, k>) - (m - bias), m the running
    maximum, so a bias of zeros changes no bit of the result.  Its values must be finite (nothing is read back to check them); a large negative finite one such as -9e15 masks an entry exactly: its
    coefficient, its share of out and every gradient that passes through it are exact zeros, provided the row keeps at least one
    unmasked entry.  Differentiable in q, k, v and bias (the gradient of a [E] bias is the sum over the heads).  float32 GPU tensors;
    1 <= H <= 64, F a power of two in 4..256, H * F <= 1024.
    Inference on bfloat16 tables: k and v may both be torch.bfloat16 (made once, e.g. k.bfloat16(); q, bias and the result stay
    float32).  The result is that of the float32 op on k.float() and v.float(), bit for bit -- the rows are widened in registers and
    all arithmetic stays fp32 -- at half the gathered bytes and half the memory of the two tables.  There is no backward: with grad
    mode on and a tensor that requires grad it raises; call it under torch.no_grad(), or pass float32 tables."""
    if _bf16_tables(k, v):
        return _dot_attention_bf16(pattern, q, k, v, scale, bias)
    return _DotAttentionFn.apply(pattern, q, k, v, None, scale, bias, None)


# ----------------------------------------------------------------------------------------------------------- dot_attention_dropout
def attention_dropout_mask(pattern: EdgePattern, H: int, p: float, seed: torch.Tensor) -> torch.Tensor:
    """The mask dot_attention_dropout(pattern, ..., p, seed=seed) draws in its kernels, as a tensor: [E, H] float32, 0 or 1 / (1 - p),
    row e the caller's entry e -- one pygat_dropout_mask launch over E * H elements (stream STREAM_ATT of the seed).  For tests and for
    composing the op from parts: spmm(pattern, edge_softmax(pattern, scores) * attention_dropout_mask(pattern, H, p, seed), v)."""
    op = "attention_dropout_mask"
    p, seed = _drop_p(op, p), _drop_seed(op, pattern, seed)
    if isinstance(H, bool) or not isinstance(H, int) or not 1 <= H <= MAX_HEADS:
        raise ValueError(f"pygat_amd {op}: H = {H!r} heads: the limits are 1 <= H <= {MAX_HEADS}")
    mask = torch.empty(pattern.nnz, H, dtype=torch.float32, device=pattern.device)
    if pattern.nnz:
        with torch.cuda.device(pattern.device):
            check(lib.pygat_dropout_mask(pattern.nnz * H, p, _ptr(seed), STREAM_ATT, _ptr(mask), _stream()), "dropout_mask")
    return mask


def dot_attention_dropout(pattern: EdgePattern, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, p: float,
                          scale: Optional[float] = None, bias: Optional[torch.Tensor] = None, *, seed: Optional[torch.Tensor] = None,
                          generator=None, training: bool = True) -> torch.Tensor:
    """dot_attention with dropout p on the attention coefficients, as a graph-transformer layer trains (F.dropout on alpha):
    out[i] = sum over the entries e = (i, j) of row i of  softmax_row(scale * <q[i], k[j]> + bias)[e] * mask[e] * v[j], per head, mask
    in {0, 1 / (1 - p)}.  The softmax runs over all entries of the row -- a dropped entry keeps its share of the denominator -- so this
    is dropout after the softmax, not masking before it.  Fused on the DROP instantiations of the K19 kernels: the decision for (entry,
    head) is drawn in registers (Philox-4x32-10) in the forward and again in the backward, and no [E, H] tensor exists outside backward.
    seed: an int64 [1] tensor on the pattern's device, read by the kernels (refill it in place between replays of a captured graph);
    None draws one with torch.randint(0, 2**62, ..., generator=generator).  The mask is attention_dropout_mask(pattern, H, p, seed), at
    the caller's entry index; the same seed gives the same bits.  training=False or p == 0 is dot_attention itself; p == 1 gives zeros.
    Differentiable in q, k, v and bias.  float32 GPU tensors with dot_attention's limits; bfloat16 tables are refused (they are for
    inference)."""
    op = "dot_attention_dropout"
    _, drop = _dropout_front(op, pattern, (k, v), "k and v must be float32: there is no training path on bfloat16 tables (they are for "
                             "dot_attention's inference forward)", p, None, seed, generator, training,
                             lambda: _checked(op, pattern, q, k, v, bias))
    if drop is None:
        return dot_attention(pattern, q, k, v, scale, bias)
    return _DotAttentionFn.apply(pattern, q, k, v, None, scale, bias, drop)


# -------------------------------------------------------------------------------------------------------------- dot_attention_edge
def dot_attention_edge(pattern: EdgePattern, q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, e: torch.Tensor,
                       scale: Optional[float] = None, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dot_attention with a feature row per entry on the key and the value side, as a graph-transformer layer uses its edge features
    (TransformerConv with edge_dim: e = lin_edge(edge_attr).view(E, H, F)):
    out[i] = sum over the entries c = (i, j) of row i of  softmax_j(scale * <q[i], k[j] + e[c]> + bias[c]) * (v[j] + e[c]), per head.
    e is [E, H, F] ([E, F] where q, k and v have no head axis) at the caller's entry index, as bias and spmm's values; scale and bias
    are dot_attention's.  Fused on the EDGE instantiations of the K19 kernels: a lane reads its 16 bytes of the e row with the k and v
    rows of the entry, k[j] + e[c] and v[j] + e[c] are one rounded add per element in both passes -- e = 0 gives dot_attention's
    values -- and the gradient of e, de[c] = ds * q[i] + alpha * G[i], is written by the row pass of the backward, once per entry: no
    transposed pass, no atomics, two runs give the same bits.  Differentiable in q, k, v, e and bias; when e does not require grad,
    no [E, H, F] tensor is made in backward.  A row without entries gets zeros; a row of one entry (i, j) gets v[j] + e[c] bit for bit.
    float32 GPU tensors with dot_attention's limits (1 <= H <= 64, F a power of two in 4..256, H * F <= 1024); bfloat16 k, v or e are
    refused: there is no inference variant and no dropout variant of this op."""
    op = "dot_attention_edge"
    if any(isinstance(t, torch.Tensor) and t.dtype == torch.bfloat16 for t in (k, v, e)):
        raise ValueError(f"pygat_amd {op}: k, v and e must be float32: bfloat16 tables are for dot_attention's inference forward")
    _require_tensor(op, pattern, "e", e, want=_E_WANT)             # (a None here would be dot_attention)
    return _DotAttentionFn.apply(pattern, q, k, v, e, scale, bias, None)
