"""The GAT score over the entries of a sparse pattern whose two sides are different tables -- a sampled block of a large graph
(destination nodes x sampled sources: what pygat_amd.sample_neighbors returns), attention from one node set to another, a GAT head inside a model built from the pattern ops.

  additive_attention  out[i, h, :] = sum over the entries e = (i, j) of row i of
                      softmax_row(LeakyReLU(s_dst[i, h] + s_src[j, h] (+ edge_logit[e, h])))[e, h] * v[j, h, :]
                      fused, on the K20 kernels (csrc/k20_additive_attention.hip): an online softmax per row, nothing written per entry

    pattern = EdgePattern.from_indices(indices [2, E], (n_dst, n_src))      # or graph.edge_pattern()
    out = additive_attention(pattern, s_dst, s_src, v)                      # s_dst [n_dst, H], s_src [n_src, H], v [n_src, H, F]
    out = spmm(pattern, edge_softmax(pattern, F.leaky_relu(s_dst[row] + s_src[col], 0.2)), v)      # the same, from parts
    out = additive_attention(pattern, s_dst, s_src, v, 0.2, edge_logit=emb(edge_type))             # gat_level's edge_logit, [E, H] | [E]
    out = additive_attention_dropout(pattern, s_dst, s_src, v, 0.6, training=self.training)        # training: dropout p on the coefficients,
                                                                # after the softmax, drawn in the kernels from a seed on the device
    with torch.no_grad():                                       # inference: a bf16 v table, made once -- half the gathered bytes, the
        out = additive_attention_bf16(pattern, s_dst, s_src, v16)    # bits of additive_attention(pattern, s_dst, s_src, v16.float())

A row's softmax runs over exactly its entries; repeated (row, col) pairs are separate entries; entries may be unsorted and the pattern
rectangular.  Differentiable in every tensor.  The backward keeps out and (m, Z) per row; its two per-entry tensors P and S ([E, H]
each) live only inside backward, between the row pass and the transposed SpMMs that form dv and ds_src.  fp32, no float atomics, a
fixed summation order: two runs give the same bits.  Nothing is read back to the host.  There is no CPU path and no fallback to torch.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from ._lib import lib, check
from ._pattern_ops import (EdgePattern, _backward_opening, _dropout_front, _entry_buffers, _forward_buffers, _head_stride, _ptr,
                           _require_dtypes, _require_heads, _require_inference, _require_pattern, _require_rows, _require_tensor, _slope,
                           _stream)
from .dropout import STREAM_ATT
from .spmm import _launch_spmm

_OP = "additive_attention"
_OP_DROP = "additive_attention_dropout"
_OP_BF16 = "additive_attention_bf16"
_PAD_HINT = ("zero-padding the columns of v to the next allowed F leaves the first F columns of the result unchanged (no scale "
             "depends on F)")


def _checked(pattern, s_dst, s_src, v, edge_logit, op: str = _OP, bf16: bool = False):
    """Every refusal that looks at the pattern and the tensors, those of edge_logit alone first, under the op's name -> (H, F, no
    head axis, the logit's head stride | None).  bf16: v is the bfloat16 table v16 of additive_attention_bf16 (its dtype was looked at
    by _require_dtypes)."""
    if edge_logit is not None:
        _require_tensor(op, pattern, "edge_logit", edge_logit)
    _require_pattern(op, pattern)
    vn = "v16" if bf16 else "v"
    for name, t in (("s_dst", s_dst), ("s_src", s_src), (vn, v)):
        _require_tensor(op, pattern, name, t, torch.bfloat16 if name == "v16" else torch.float32)
    named = (("s_dst", s_dst, pattern.n_rows, "rows"), ("s_src", s_src, pattern.n_cols, "columns"), (vn, v, pattern.n_cols, "columns"))
    if s_dst.dim() not in (1, 2):
        raise ValueError(f"pygat_amd {op}: s_dst [n_rows] or [n_rows, H] expected, got {tuple(s_dst.shape)}")
    if s_src.dim() != s_dst.dim() or s_src.shape[1:] != s_dst.shape[1:]:
        raise ValueError(f"pygat_amd {op}: s_src {tuple(s_src.shape)} does not match s_dst {tuple(s_dst.shape)}: the same number of "
                         f"heads expected")
    if v.dim() != s_dst.dim() + 1 or v.shape[1:-1] != s_dst.shape[1:]:
        raise ValueError(f"pygat_amd {op}: {vn} {tuple(v.shape)} does not match s_dst {tuple(s_dst.shape)}: {vn} [n_cols, F] with s_dst "
                         f"[n_rows], or {vn} [n_cols, H, F] with s_dst [n_rows, H] and the same number of heads, expected")
    _require_rows(op, named)
    flat = s_dst.dim() == 1
    H, F = (1 if flat else int(s_dst.shape[1])), int(v.shape[-1])
    _require_heads(op, H, F, _PAD_HINT)
    return H, F, flat, None if edge_logit is None else _head_stride(op, pattern, "edge_logit", edge_logit, H, flat)


def _launch(pattern, which: str, H: int, F: int, slope: float, sd, ss, vc, uc, uhs, drop, rest, bf16: bool = False):
    """One K20 launcher call, `which` "forward" or "backward_rows", at the entry point of what is present -- a bf16 v table, a dropout
    (p, seed) or none: the pattern's arrays, the three tables, the logit (None: the kernels without the term, which without dropout
    need no permutation in the forward), the dropout group, then `rest`, the pass's own arguments up to the workspace."""
    kind = "bf16_" if bf16 else "" if drop is None else "dropout_"
    group = () if drop is None else (drop[0], _ptr(drop[1]), STREAM_ATT)
    ws = torch.empty(_lib.add_attn_workspace_bytes(pattern.nnz, H, F), dtype=torch.uint8, device=vc.device)
    check(getattr(lib, f"pygat_add_attn_{kind}{which}")(pattern.n_rows, pattern.nnz, _ptr(pattern.rowptr), _ptr(pattern.col),
                                                         _ptr(pattern.perm), H, F, slope, _ptr(sd), _ptr(ss), _ptr(vc), H * F,
                                                         _ptr(uc), uhs or 0, *group, *rest, _ptr(ws), _stream()),
          f"add_attn_{kind}{which}")


class _AdditiveAttentionFn(torch.autograd.Function):
    """additive_attention and additive_attention_dropout.  drop: None or (p, seed) of additive_attention_dropout: the mask of the
    coefficients, drawn in the kernels of both passes from the int64 [1] seed tensor on the device."""

    @staticmethod
    def forward(ctx, pattern, s_dst, s_src, v, slope, edge_logit, drop=None):
        op = _OP if drop is None else _OP_DROP
        H, F, flat, uhs = _checked(pattern, s_dst, s_src, v, edge_logit, op)
        p, seed = (None, None) if drop is None else drop
        ctx.pattern, ctx.slope, ctx.hf, ctx.uhs, ctx.op, ctx.p = pattern, slope, (H, F), uhs, op, p
        if pattern.nnz == 0:                                       # every row is without entries: zeros, and nothing is launched
            ctx.save_for_backward(s_dst, s_src, v, edge_logit, None, None, None, None)
            return torch.zeros((pattern.n_rows,) + tuple(v.shape[1:]), dtype=torch.float32, device=v.device)
        sd, ss, vc, uc = (None if t is None else t.detach().contiguous() for t in (s_dst, s_src, v, edge_logit))
        n, dev = pattern.n_rows, vc.device
        with torch.cuda.device(dev):
            out, m, Z = _forward_buffers(n, H, F, dev)
            _launch(pattern, "forward", H, F, slope, sd, ss, vc, uc, uhs, drop, (_ptr(out), H * F, _ptr(m), _ptr(Z)))
        out = out.view((n,) + tuple(v.shape[1:]))
        ctx.save_for_backward(s_dst, s_src, v, edge_logit, out, m, Z, seed)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, G):
        s_dst, s_src, v, edge_logit, out, m, Z, seed = ctx.saved_tensors
        pattern, slope, (H, F), uhs = ctx.pattern, ctx.slope, ctx.hf, ctx.uhs
        need_d, need_s, need_v = ctx.needs_input_grad[1:4]
        need_u = edge_logit is not None and ctx.needs_input_grad[5]
        early = _backward_opening(ctx.op, G, out, 7, {1: (s_dst, need_d), 2: (s_src, need_s), 3: (v, need_v), 5: (edge_logit, need_u)})
        if early is not None:
            return early
        n, nnz, HF, dev = pattern.n_rows, pattern.nnz, H * F, v.device
        sd, ss, vc, uc = (None if t is None else t.detach().contiguous() for t in (s_dst, s_src, v, edge_logit))
        Gc = G.contiguous().view(n, HF)
        with torch.cuda.device(dev):
            dd = torch.empty(n, H, dtype=torch.float32, device=dev)
            P, S = _entry_buffers(nnz, H, dev)
            _launch(pattern, "backward_rows", H, F, slope, sd, ss, vc, uc, uhs, None if seed is None else (ctx.p, seed),
                    (_ptr(out), HF, _ptr(m), _ptr(Z), _ptr(Gc), HF, _ptr(dd), _ptr(P), _ptr(S)))
            du = None
            if need_u:                          # S is the gradient of an [E, H] logit; an [E] one shared by H heads gets the sum over them
                du = S.sum(1) if uhs == 0 else S.view(edge_logit.shape)
            ds = dv = None
            if need_s or need_v:
                rowptr_t, row_t, perm_t = pattern.transposed()
                if need_s:                      # the column sums of S: K17's F = 1 path against a table of ones
                    ones = torch.ones(n, H, dtype=torch.float32, device=dev)
                    ds = _launch_spmm(pattern.n_cols, nnz, rowptr_t, row_t, perm_t, H, 1, S, ones).view(s_src.shape)
                if need_v:
                    dv = _launch_spmm(pattern.n_cols, nnz, rowptr_t, row_t, perm_t, H, F, P, Gc).view(v.shape)
        return None, dd.view(s_dst.shape) if need_d else None, ds, dv, None, du, None


def additive_attention(pattern: EdgePattern, s_dst: torch.Tensor, s_src: torch.Tensor, v: torch.Tensor, negative_slope: float = 0.2,
                       edge_logit: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [n_rows, H, F] (s_dst [n_rows, H], s_src [n_cols, H], v [n_cols, H, F]) or out [n_rows, F] (s_dst [n_rows], s_src [n_cols],
    v [n_cols, F]): out[i] = sum over the entries (i, j) of row i of softmax_j(LeakyReLU(s_dst[i] + s_src[j] + edge_logit[e])) * v[j],
    per head -- the attention of a GAT level with the row side and the column side as different tables (for a level on one node set:
    s_dst = Wh . a_dst, s_src = Wh . a_src, v = Wh).  z = (s_dst[i] + s_src[j]) + edge_logit[e] is two rounded adds in this order;
    LeakyReLU has the slope negative_slope (a finite float) for z <= 0, and its derivative at z == 0 is negative_slope, as torch's.
    A row without entries gets zeros; a pattern without entries launches nothing.
    edge_logit (optional): a per-entry term in front of the LeakyReLU, gat_level's edge_logit, at the caller's entry index -- [E, H], or
    [E] for one value per entry shared by the heads (and where the tensors have no head axis).  A logit of zeros changes no bit of the
    result.  Its values must be finite (nothing is read back to check them); a large negative finite one such as -9e15 masks an entry
    exactly -- its coefficient, its share of out and every gradient that passes through it are exact zeros -- provided the row keeps at
    least one unmasked entry and negative_slope > 0.  It does not mask at negative_slope == 0: LeakyReLU then sends every negative z to 0.
    Differentiable in s_dst, s_src, v and edge_logit (the gradient of an [E] logit is the sum over the heads); a gradient that is not
    asked for costs no launch.  float32 GPU tensors on the pattern's device; 1 <= H <= 64, F a power of two in 4..256, H * F <= 1024;
    for another F zero-pad the columns of v: the first F columns of the result are unchanged.
    Not provided: dropout on the coefficients (that is the sibling op's, additive_attention_dropout), a fused column pass (dv and
    ds_src are two K17 launches on the transposed pattern).  Inference on a bfloat16 v table is the sibling op's,
    additive_attention_bf16."""
    return _AdditiveAttentionFn.apply(pattern, s_dst, s_src, v, _slope(_OP, negative_slope), edge_logit)


def additive_attention_dropout(pattern: EdgePattern, s_dst: torch.Tensor, s_src: torch.Tensor, v: torch.Tensor, p: float,
                               negative_slope: float = 0.2, edge_logit: Optional[torch.Tensor] = None, *,
                               seed: Optional[torch.Tensor] = None, generator=None, training: bool = True) -> torch.Tensor:
    """additive_attention with dropout p on the attention coefficients, as a GAT trains (the reference's dropout after the
    normalisation, PyG's GATConv): out[i] = sum over the entries e = (i, j) of row i of
    softmax_row(LeakyReLU(s_dst[i] + s_src[j] + edge_logit[e]))[e] * mask[e] * v[j], per head, mask in {0, 1 / (1 - p)}.  The softmax
    runs over all entries of the row -- a dropped entry keeps its share of the denominator -- so this is dropout after the softmax, not
    masking before it.  Fused on the DROP instantiations of the K20 kernels: the decision for (entry, head) is drawn in registers
    (Philox-4x32-10) in the forward and again in the backward, and no [E, H] mask exists outside backward.
    seed: an int64 [1] tensor on the pattern's device, read by the kernels (refill it in place between replays of a captured graph);
    None draws one with torch.randint(0, 2**62, ..., generator=generator).  The mask is attention_dropout_mask(pattern, H, p, seed), at
    the caller's entry index -- the mask dot_attention_dropout and gatv2_attention_dropout draw from the same seed; the same seed gives
    the same bits.  training=False or p == 0 is additive_attention itself; p == 1 gives zeros; a row whose entries are all dropped
    gets exact zeros.  Differentiable in s_dst, s_src, v and edge_logit; a gradient that is not asked for costs no launch.  float32 GPU
    tensors with additive_attention's limits; bfloat16 tensors are refused."""
    op = _OP_DROP
    slope, drop = _dropout_front(op, pattern, (s_dst, s_src, v, edge_logit), "s_dst, s_src, v and edge_logit must be float32: there is no "
                                 "training path on bfloat16 tensors", p, negative_slope, seed, generator, training,
                                 lambda: _checked(pattern, s_dst, s_src, v, edge_logit, op))
    if drop is None:
        return additive_attention(pattern, s_dst, s_src, v, slope, edge_logit)
    return _AdditiveAttentionFn.apply(pattern, s_dst, s_src, v, slope, edge_logit, drop)


def additive_attention_bf16(pattern: EdgePattern, s_dst: torch.Tensor, s_src: torch.Tensor, v16: torch.Tensor,
                            negative_slope: float = 0.2, edge_logit: Optional[torch.Tensor] = None) -> torch.Tensor:
    """additive_attention for inference on a bfloat16 value table: v16 [n_cols, H, F] (or [n_cols, F]) is torch.bfloat16, made once
    (v.bfloat16()); s_dst, s_src, edge_logit and the result stay float32.  The result is additive_attention(pattern, s_dst, s_src,
    v16.float(), negative_slope, edge_logit) bit for bit: on the BF16 instantiations of the K20 forward kernels a lane loads the same
    4 row elements as 8 bytes and widens them in registers, and everything after the load is the float32 kernels' arithmetic in their
    order -- at half the gathered bytes of v and half the memory of the table; no float32 copy of it is made.  Forward only: nothing
    is saved, no per-row softmax state is written and no transpose of the pattern is built.  With grad mode on and an argument that
    requires grad it raises: call it under torch.no_grad(), or use additive_attention on float32 tables.  A float32 v16, or a bfloat16
    tensor in any other place, is refused.  A row without entries gets zeros; a pattern without entries launches nothing.  The limits
    are additive_attention's: 1 <= H <= 64, F a power of two in 4..256, H * F <= 1024.
    Not provided: a backward, dropout, bfloat16 s_dst, s_src, edge_logit or results."""
    op = _OP_BF16
    slope = _slope(op, negative_slope)
    _require_inference(op, _OP, (s_dst, s_src, v16, edge_logit))
    _require_dtypes(op, (("s_dst", s_dst, torch.float32), ("s_src", s_src, torch.float32), ("v16", v16, torch.bfloat16),
                         ("edge_logit", edge_logit, torch.float32)))
    H, F, flat, uhs = _checked(pattern, s_dst, s_src, v16, edge_logit, op, bf16=True)
    n, dev = pattern.n_rows, v16.device
    if pattern.nnz == 0:                                           # every row is without entries: zeros, and nothing is launched
        return torch.zeros((n,) + tuple(v16.shape[1:]), dtype=torch.float32, device=dev)
    sd, ss, vc, uc = (None if t is None else t.detach().contiguous() for t in (s_dst, s_src, v16, edge_logit))
    with torch.cuda.device(dev):
        out = _forward_buffers(n, H, F, dev, state=False)[0]
        _launch(pattern, "forward", H, F, slope, sd, ss, vc, uc, uhs, None, (_ptr(out), H * F), bf16=True)
    return out.view((n,) + tuple(v16.shape[1:]))
